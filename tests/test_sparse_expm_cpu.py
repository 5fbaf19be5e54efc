"""`sparse_expm_mm` without a GPU: the coefficient rule against the exponential it expands, the torch-op path on CPU tensors in fp64
against `torch.linalg.matrix_exp` and `torch.autograd.gradcheck`, layouts, index types, every refusal, the staged header
csrc/tsgu_hip_expm.h against its ctypes table and the library, and the host refusals of the launchers (fake pointers, device = -1:
nothing is dereferenced).

Bounds.  The coefficient test holds Σ_k c_k T_k(x) against exp(t(ρx + mid)) on 2001 points of [−1, 1] within the method's own
bound, tolerance·S with S = e^{max(t·lo, t·hi)} (|T_k| ≤ 1 and Σ_{k>K} |c_k| ≤ tolerance·S), plus 8·(K + 1)·eps·S for the float64
evaluation of Σ_k c_k cos(k·acos x): k·π·eps in every cosine's argument, the sum of K + 1 terms whose absolute values add up to S
(Σ_k |c_k| = S·(ive_0 + 2 Σ ive_k) = S) and the rounding of the exponential it is compared with.  The torch-op path runs at tolerance
1e-13; its error against the dense exponential is held to the bounds of tests/test_gpu_sparse_expm.py (derived in that file's
docstring) evaluated at tolerance + 4·(K + 1)²·eps: the three-term recurrence amplifies a rounding made at step j by at most
|U_{k−j}| ≤ k − j + 1 at step k, so K + 1 steps of relative size eps against Σ|c_k| = S leave at most (K + 1)²·eps·S per unit of ‖b‖,
taken four times for the products and the sums of one step.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _expm_ref as ER
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_expm_mm
from torchsparsegradutils_amd.sparse_expm import SparseExpmMM, _coefficients, _ive

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_expm.h")
ENTRIES = ("tsgu_expm_geometry", "tsgu_cheb_step", "tsgu_cheb_combine")
F64 = torch.float64
EPS = float(np.finfo(np.float64).eps)
TOL = 1e-13


def _sparse(M, layout="csr", itype=torch.int64, dtype=F64):
    crow, col, val = ER.csr_arrays(M)
    n = M.shape[0]
    if layout == "csr":
        return torch.sparse_csr_tensor(torch.from_numpy(crow).to(itype), torch.from_numpy(col).to(itype), torch.from_numpy(val).to(dtype),
                                       (n, n))
    rows = np.repeat(np.arange(n), np.diff(crow))
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, col))).to(itype), torch.from_numpy(val).to(dtype), (n, n)).coalesce()


# ---- the coefficients ---------------------------------------------------------------------------------------------------------------

def test_ive_matches_the_restatement_and_the_term_counts():
    for x, K in ((1.0, 7), (10.0, 17), (100.0, 49), (1000.0, 155), (5000.0, 346)):
        f, k = _ive(x, 1e-6)
        g, k_ref = ER.ive(x, 1e-6)
        assert k == k_ref == K
        assert np.abs(f - g).max() <= 1e-15
        assert abs(f[0] + 2.0 * f[1:].sum() - 1.0) <= 1e-14 and np.all(f >= 0) and np.all(np.diff(f[: k + 1]) < 0)
    assert _ive(0.0, 1e-6)[1] == 0 and _ive(0.0, 1e-6)[0].tolist() == [1.0]


@pytest.mark.parametrize("sign", [-1.0, 1.0])
@pytest.mark.parametrize("z", [0.0, 0.5, 10.0, 100.0, 1000.0])
@pytest.mark.parametrize("tolerance", [1e-6, 1e-12])
def test_coefficients_expand_the_exponential(z, sign, tolerance):
    # an interval off the origin where e^{t·hi} fits float64; for |z| >= 100 the end the sign of t weighs is put at 0
    lo, hi = (-1.0, 3.0) if z <= 10.0 else (0.0, 4.0) if sign < 0 else (-4.0, 0.0)
    rho, mid = 2.0, 0.5 * (lo + hi)
    t = sign * z / rho
    c, a, b, K = _coefficients("test", np.array([[t]]), lo, hi, tolerance, 4096)
    assert c.shape == (K + 1, 1, 1) and a == 0.5 and b == -mid / rho
    c = c[:, 0, 0]
    ref, ra, rb = ER.coefficients(t, lo, hi, tolerance)
    assert ref.shape == c.shape and np.allclose(c, ref, rtol=1e-13, atol=0) and (ra, rb) == (a, b)
    x = np.linspace(-1.0, 1.0, 2001)
    S = np.exp(max(t * lo, t * hi))
    err = np.abs(ER.chebyshev_sum(c, x) - np.exp(t * (rho * x + mid))).max()
    print(f"z {sign * z:g} tolerance {tolerance:g}: K {K}, max error / S = {err / S:.2e}")
    assert err <= (tolerance + 8.0 * (K + 1) * EPS) * S
    # K is minimal: one term fewer leaves a tail above the tolerance
    f, _ = ER.ive(abs(z), tolerance)
    if K > 0:
        assert 2.0 * f[K:].sum() > tolerance >= 2.0 * f[K + 1:].sum()
    else:
        assert 2.0 * f[1:].sum() <= tolerance


def test_many_distinct_times_take_the_vectorised_recurrence_and_agree():
    """From 48 distinct |t|·ρ on, one recurrence runs for all of them from the start index of the largest: the same table to rounding
    (the backward recurrence is stable from any start beyond x), the same K, zero and tiny arguments included."""
    from torchsparsegradutils_amd.sparse_expm import _VECTOR_FROM, _ive_many

    xs = np.concatenate(([0.0, 1e-9, 1e-3], np.geomspace(0.05, 300.0, 61)))
    assert xs.size >= _VECTOR_FROM
    table, K = _ive_many(xs, 1e-10)
    for u, x in enumerate(xs):
        f, k = ER.ive(x, 1e-10)
        assert K[u] == k, x
        assert np.allclose(table[: k + 1, u], f[: k + 1], rtol=1e-13, atol=0), x
    t = -xs.reshape(1, -1) / 4.0
    c, a, b, Kc = _coefficients("test", t, 0.0, 8.0, 1e-10, 4096)
    assert Kc == K.max() and c.shape == (Kc + 1, 1, xs.size) and c.flags["C_CONTIGUOUS"]
    for u in (0, 1, 5, 40, xs.size - 1):
        ref, _, _ = ER.coefficients(t[0, u], 0.0, 8.0, 1e-10, K=Kc)
        # (S <= 1 here.  Far beyond an argument's own K the restatement, which starts at ITS x + 60, is still in its start-up, and
        # both lose what is below 1e-250 to their rescaling: entries below 1e-30 are 1e-20 of the tolerance and compared absolutely)
        assert np.allclose(c[:, 0, u], ref, rtol=1e-13, atol=1e-30), u


def test_coefficients_of_several_times_share_one_length():
    t = np.array([[-1.0, 0.0, 0.25], [0.5, -0.125, 2.0]])
    c, a, b, K = _coefficients("test", t, 0.0, 8.0, 1e-10, 4096)
    assert c.shape == (K + 1, 2, 3) and c.flags["C_CONTIGUOUS"], "the kernels read the table [k][time][column] through its pointer"
    for j in range(2):
        for col in range(3):
            ref, _, _ = ER.coefficients(t[j, col], 0.0, 8.0, 1e-10, K=K)
            assert np.allclose(c[:, j, col], ref, rtol=1e-13, atol=1e-300)
    assert K == max(ER.ive(abs(x) * 4.0, 1e-10)[1] for x in t.reshape(-1))
    assert c[:, 0, 1].tolist() == [1.0] + [0.0] * K, "t = 0: the identity"
    point = _coefficients("test", t, 2.0, 2.0, 1e-10, 4096)
    assert point[1:] == (0.0, 0.0, 0) and np.array_equal(point[0][0], np.exp(2.0 * t))


# ---- the torch-op path ----------------------------------------------------------------------------------------------------------------

TIMES = {"float": -0.7, "0-d": 0.4, "(T,)": [-1.0, 0.3, -0.1], "(T, p)": [[-0.9, 0.2, -0.05], [0.1, 0.5, -0.4]]}


@pytest.fixture(scope="module")
def cases():
    """(matrix, times) -> the float64 truth (tests/_expm_ref.py), computed once, never written to."""
    out = {}
    for name in ("lap6x5x4", "random200"):
        M = ER.MATRICES[name]()
        lo, hi = ER.gershgorin(M)
        for key, times in TIMES.items():
            rng = np.random.default_rng(len(out) + 3)
            T = 1 if np.ndim(times) == 0 else len(times)
            out[name, key] = ER.make_case(M, rng.standard_normal((M.shape[0], 3)), rng.standard_normal((T, M.shape[0], 3)), times, lo, hi)
    return out


def _run(c, key, layout, itype=torch.int64):
    S = _sparse(c["M"], layout, itype).requires_grad_(True)
    B = torch.from_numpy(c["B"].copy()).requires_grad_(True)
    t = TIMES[key] if key == "float" else torch.tensor(TIMES[key], dtype=F64, requires_grad=True)
    out, info = sparse_expm_mm(S, B, t, tolerance=TOL, return_info=True)
    out.backward(torch.from_numpy(c["G"]).reshape(out.shape))
    gA = S.grad.values() if layout == "csr" else S.grad._values()
    return out, B.grad, gA, (None if key == "float" else t.grad), info, S


@pytest.mark.parametrize("key", list(TIMES))
@pytest.mark.parametrize("layout,itype", [("csr", torch.int64), ("csr", torch.int32), ("coo", torch.int64)])
@pytest.mark.parametrize("name", ["lap6x5x4", "random200"])
def test_cpu_path_against_the_dense_exponential(cases, name, layout, itype, key):
    c = cases[name, key]
    out, gB, gA, gt, info, S = _run(c, key, layout, itype)
    K = info["terms"]
    T = c["G"].shape[0]
    assert info["fused"] is False and info["chunk"] == 1 and info["bounds"] == pytest.approx((c["lo"], c["hi"]), rel=1e-14)
    assert out.shape == ((T,) if np.ndim(TIMES[key]) > 0 else ()) + c["B"].shape and out.dtype == F64
    assert gt is None or gt.shape == np.shape(TIMES[key])
    g = S.grad
    assert g.layout == S.layout and g.shape == S.shape
    if layout == "csr":
        assert torch.equal(g.crow_indices(), S.crow_indices()) and g.col_indices().dtype == itype
    else:
        assert g._indices().data_ptr() == S._indices().data_ptr(), "the gradient is built on A's own index tensor"
    err = ER.errors(c, out.detach().numpy().reshape(c["Y"].shape), gB.numpy(), gA.numpy(), None if gt is None else gt.numpy())
    bound = ER.error_bounds(c, K, 2.0 / (c["hi"] - c["lo"]), TOL + 4.0 * (K + 1) ** 2 * EPS)
    for k, e in err.items():
        print(f"{name} {layout} {key} K {K}: {k} {float(e.max()):.2e} of {float(np.max(bound[k])):.2e}")
        assert np.all(e <= bound[k]), k


def test_against_torch_matrix_exp_autograd():
    """The same check through torch's own dense exponential and autograd, on the small random pattern of the method's derivation."""
    torch.manual_seed(0)
    n, p = 12, 3
    R = torch.randn(n, n, dtype=F64)
    mask = (torch.rand(n, n) < 0.4) | torch.eye(n, dtype=torch.bool)
    mask = mask | mask.T
    Md = ((R + R.T) * mask).requires_grad_(True)
    B = torch.randn(n, p, dtype=F64, requires_grad=True)
    t = torch.tensor([-0.7, 0.3], dtype=F64, requires_grad=True)
    G = torch.randn(2, n, p, dtype=F64)
    want = torch.stack([torch.linalg.matrix_exp(t[j] * Md) @ B for j in range(2)])
    wA, wB, wt = torch.autograd.grad((want * G).sum(), (Md, B, t))
    S = Md.detach().to_sparse_csr().requires_grad_(True)
    Bs, ts = B.detach().clone().requires_grad_(True), t.detach().clone().requires_grad_(True)
    got, info = sparse_expm_mm(S, Bs, ts, tolerance=TOL, return_info=True)
    gA, gB, gt = torch.autograd.grad((got * G).sum(), (S, Bs, ts))
    rows = np.repeat(np.arange(n), np.diff(S.crow_indices().numpy()))
    cols = S.col_indices().numpy()
    lo, hi = info["bounds"]
    scale = float(np.exp(np.maximum(t.detach().numpy() * lo, t.detach().numpy() * hi)).max())
    tol_eff = TOL + 4.0 * (info["terms"] + 1) ** 2 * EPS
    nB, nG = float(B.detach().norm()), float(G.norm())
    print(f"K {info['terms']} S {scale:.3g}: fwd {float((got - want).abs().max()):.2e} gB {float((gB - wB).abs().max()):.2e} "
          f"gA {float((gA.values() - wA[rows, cols]).abs().max()):.2e} gt {float((gt - wt).abs().max()):.2e}")
    assert float((got - want).norm()) <= 10.0 * tol_eff * scale * nB * np.sqrt(2)
    assert float((gB - wB).norm()) <= 10.0 * tol_eff * scale * nG * np.sqrt(2)
    assert float((gt - wt).abs().max()) <= 10.0 * tol_eff * scale * nB * nG * max(abs(lo), abs(hi))
    assert float((gA.values() - wA[rows, cols]).norm()) <= 120.0 * (info["terms"] + 1) ** 2 * (2.0 / (hi - lo)) * tol_eff * scale * nB * nG * 2


def test_gradients_are_exact_for_the_approximant():
    """At a coarse tolerance (1e-4: K = 9) the values are 1e-5 from the exponential, yet values and gradients equal the dense
    expansion and its adjoint recurrence (tests/_expm_ref.py) at the same K to rounding: 4·(K + 1)²·eps of S·‖b‖ (the file's docstring)."""
    M = ER.MATRICES["lap6x5x4"]()
    lo, hi = ER.gershgorin(M)
    rng = np.random.default_rng(12)
    Bn, Gn = rng.standard_normal((120, 2)), rng.standard_normal((120, 2))
    t, tol = -0.7, 1e-4
    c, a, b = ER.coefficients(t, lo, hi, tol)
    K = len(c) - 1
    want, W = ER.expansion(M, Bn, c, a, b)
    want_gB, want_gA = ER.adjoint(M, Gn, c, a, b, W)
    S = _sparse(M).requires_grad_(True)
    B = torch.from_numpy(Bn.copy()).requires_grad_(True)
    got, info = sparse_expm_mm(S, B, t, tolerance=tol, return_info=True)
    got.backward(torch.from_numpy(Gn))
    assert info["terms"] == K
    crow, col, _ = ER.csr_arrays(M)
    rows = np.repeat(np.arange(120), np.diff(crow))
    scale = 4.0 * (K + 1) ** 2 * EPS * np.exp(max(t * lo, t * hi))
    nB, nG = np.linalg.norm(Bn), np.linalg.norm(Gn)
    assert np.linalg.norm(got.detach().numpy() - want) <= scale * nB
    assert np.linalg.norm(B.grad.numpy() - want_gB) <= scale * nG
    assert np.linalg.norm(S.grad.values().numpy() - want_gA[rows, col]) <= scale * (K + 1) * 2.0 * a * nB * nG
    assert np.linalg.norm(got.detach().numpy() - ER.dense_expm(M, t) @ Bn) > 1e3 * scale * nB, "the truncation is visible at this tolerance"


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_gradcheck(layout):
    M = ER.MATRICES["lap6x5x4"]()
    n = M.shape[0]
    S = _sparse(M, layout)
    kw = dict(tolerance=TOL)
    rng = np.random.default_rng(8)
    B = torch.from_numpy(rng.standard_normal((n, 2))).requires_grad_(True)
    t = torch.tensor([-0.3, 0.2], dtype=F64, requires_grad=True)
    tp = torch.tensor([[-0.3, 0.2]], dtype=F64, requires_grad=True)
    t0 = torch.tensor(0.25, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda b, s: sparse_expm_mm(S, b, s, **kw), (B, t), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda b, s: sparse_expm_mm(S, b[:, 0], s, **kw), (B, t0), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda s: sparse_expm_mm(S, B.detach(), s, **kw), (tp,), eps=1e-6, atol=1e-7, rtol=1e-6)
    crow, col, _ = ER.csr_arrays(M)
    rows = np.repeat(np.arange(n), np.diff(crow))
    mirror = torch.from_numpy(np.searchsorted(rows * n + col, col * n + rows))       # position of (j, i) for the entry (i, j)
    # the expansion is that of a symmetric matrix: every perturbation is made symmetric, (v + v mirrored) / 2, and the chain rule
    # tests the stored-entry gradient g through (g_ij + g_ji) / 2.  The bounds are given: Gershgorin's would move with the values.
    lo, hi = ER.gershgorin(M)
    kw["bounds"] = (lo - 0.5, hi + 0.5)
    if layout == "csr":
        ci, cc = S.crow_indices(), S.col_indices()
        rebuild = lambda v: torch.sparse_csr_tensor(ci, cc, 0.5 * (v + v[mirror]), (n, n))              # noqa: E731
    else:
        idx = S.indices()
        rebuild = lambda v: torch.sparse_coo_tensor(idx, 0.5 * (v + v[mirror]), (n, n)).coalesce()      # noqa: E731
    values = S.values().clone().requires_grad_(True)
    Bc = B.detach()[:, :1].contiguous()
    assert torch.autograd.gradcheck(lambda v: sparse_expm_mm(rebuild(v), Bc, -0.3, **kw), (values,), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- layouts, shapes and other paths -----------------------------------------------------------------------------------------------------

def test_vector_b_zero_time_bounds_and_the_one_by_one_matrix(cases):
    c = cases["lap6x5x4", "float"]
    S = _sparse(c["M"])
    B = torch.from_numpy(c["B"].copy())
    vec = sparse_expm_mm(S, B[:, 0].contiguous(), -0.7, tolerance=TOL)
    assert vec.shape == (120,) and np.linalg.norm(vec.numpy() - c["Y"][0, :, 0]) <= 1e-11 * np.linalg.norm(c["B"][:, 0])
    many = sparse_expm_mm(S, B[:, 0].contiguous(), torch.tensor([-0.7, 0.0], dtype=F64), tolerance=TOL)
    assert many.shape == (2, 120) and torch.equal(many[1], B[:, 0])
    assert torch.equal(sparse_expm_mm(S, B, 0.0), B), "t = 0 returns B's bits"
    assert torch.equal(sparse_expm_mm(S, B, torch.tensor(0.0)), B)
    assert torch.equal(sparse_expm_mm(S, B, -0.7, tolerance=TOL), sparse_expm_mm(S, B, -0.7, tolerance=TOL))
    lam = np.linalg.eigvalsh(c["M"])
    tight, info_t = sparse_expm_mm(S, B, -0.7, bounds=(float(lam[0]), float(lam[-1])), tolerance=TOL, return_info=True)
    loose, info_l = sparse_expm_mm(S, B, -0.7, tolerance=TOL, return_info=True)
    assert info_t["bounds"] == (float(lam[0]), float(lam[-1])) and info_l["bounds"] == pytest.approx(ER.gershgorin(c["M"]), rel=1e-14)
    assert info_t["terms"] < info_l["terms"], "a loose interval only costs terms"
    assert set(info_t) == {"terms", "bounds", "chunk", "fused"}
    nb = np.linalg.norm(c["B"], axis=0)
    for got in (tight, loose):
        assert np.all(np.linalg.norm(got.numpy() - c["Y"][0], axis=0) <= 1e-11 * nb)
    # a degenerate interval: e^{t lo} B; the 1 x 1 matrix is one by Gershgorin
    got, info = sparse_expm_mm(_sparse(ER.MATRICES["one"](), "coo"), torch.tensor([[2.0, -3.0]], dtype=F64), 0.5, return_info=True)
    assert info["terms"] == 0 and info["bounds"] == (0.75, 0.75)
    assert np.allclose(got.numpy(), np.exp(0.375) * np.array([[2.0, -3.0]]), rtol=1e-15)
    ident = _sparse(2.0 * np.eye(5))
    assert np.allclose(sparse_expm_mm(ident, torch.ones(5, dtype=F64), -1.5).numpy(), np.exp(-3.0), rtol=1e-15)


def test_uncoalesced_coo_is_coalesced_first(cases):
    c = cases["lap6x5x4", "float"]
    C = _sparse(c["M"], "coo")
    U = torch.sparse_coo_tensor(torch.cat((C.indices(), C.indices()), dim=1), torch.cat((0.25 * C.values(), 0.75 * C.values())), C.shape)
    assert not U.is_coalesced()
    got = sparse_expm_mm(U, torch.from_numpy(c["B"].copy()), -0.7, tolerance=TOL)
    assert np.abs(got.numpy() - c["Y"][0]).max() <= 1e-11 * np.abs(c["Y"][0]).max()


def test_surface_and_refusals():
    assert {"sparse_expm_mm", "SparseExpmMM"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_expm import __all__ as mod_all

    assert sorted(mod_all) == ["SparseExpmMM", "sparse_expm_mm"]
    assert tsgu.SparseExpmMM is SparseExpmMM and issubclass(SparseExpmMM, torch.autograd.Function)
    assert "heat-kernel diffusion" in sparse_expm_mm.__doc__ and "Gershgorin" in sparse_expm_mm.__doc__
    M = ER.laplacian7(3, 2, 2)
    S = _sparse(M)
    ones = torch.ones(12, dtype=F64)
    who, fn = "sparse_expm_mm", sparse_expm_mm
    with pytest.raises(ValueError, match=f"{who}: A should be an instance of torch.Tensor"):
        fn(3, ones)
    with pytest.raises(ValueError, match=f"{who}: A should be in either COO or CSR sparse format"):
        fn(torch.from_numpy(M), ones)
    with pytest.raises(ValueError, match=rf"{who}: A must be a 2-D sparse matrix \(batched operands are not supported\), got 3 dimensions"):
        fn(torch.stack((torch.from_numpy(M), torch.from_numpy(M))).to_sparse(), ones)
    with pytest.raises(ValueError, match=rf"{who}: A must be a 2-D sparse matrix \(hybrid operands are not supported\), got 1 dense"):
        fn(torch.ones(12, 12, 2, dtype=F64).to_sparse(2), ones)
    with pytest.raises(ValueError, match=rf"{who}: A must be square, got \(3, 4\)"):
        fn(torch.ones(3, 4, dtype=F64).to_sparse(), ones)
    with pytest.raises(ValueError, match=f"{who}: float32 and float64 operands only, got torch.bfloat16"):
        fn(torch.from_numpy(M).to(torch.bfloat16).to_sparse(), ones)
    with pytest.raises(ValueError, match=rf"{who}: B must be a dense \(strided\) tensor"):
        fn(S, None)
    with pytest.raises(ValueError, match=rf"{who}: B must be a dense \(strided\) tensor"):
        fn(S, S)
    with pytest.raises(ValueError, match=rf"{who}: B must have shape \(12,\) or \(12, p\), got \(11,\)"):
        fn(S, torch.ones(11, dtype=F64))
    with pytest.raises(ValueError, match=rf"{who}: B must have shape \(12,\) or \(12, p\), got \(12, 0\)"):
        fn(S, torch.ones(12, 0, dtype=F64))
    with pytest.raises(ValueError, match=rf"{who}: B must have shape \(12,\) or \(12, p\), got \(12, 2, 2\)"):
        fn(S, torch.ones(12, 2, 2, dtype=F64))
    with pytest.raises(ValueError, match=f"{who}: B must have A's dtype, got torch.float32 and torch.float64"):
        fn(S, torch.ones(12))
    for bad in ("soon", None, torch.ones(2, dtype=torch.int64), S):
        with pytest.raises(ValueError, match=f"{who}: t must be a float or a dense floating-point tensor"):
            fn(S, ones, bad)
    for bad, p in ((torch.ones(2, 3, dtype=F64), 1), (torch.ones(1, 1, 1, dtype=F64), 1), (torch.ones(0, dtype=F64), 1)):
        with pytest.raises(ValueError, match=rf"{who}: t must be a scalar, have shape \(T,\) or \(T, {p}\), got"):
            fn(S, ones, bad)
    with pytest.raises(ValueError, match=rf"{who}: t must be a scalar, have shape \(T,\) or \(T, 2\), got \(1, 3\)"):
        fn(S, torch.ones(12, 2, dtype=F64), torch.ones(1, 3, dtype=F64))
    with pytest.raises(ValueError, match=f"{who}: at most 8 times per call, got 9"):
        fn(S, ones, torch.ones(9, dtype=F64))
    with pytest.raises(ValueError, match=f"{who}: max_terms must not be negative, got -1"):
        fn(S, ones, max_terms=-1)
    with pytest.raises(ValueError, match=f"{who}: tolerance must be positive, got 0"):
        fn(S, ones, tolerance=0.0)
    with pytest.raises(ValueError, match=rf"{who}: bounds must be a pair \(lo, hi\) of floats or None"):
        fn(S, ones, bounds=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match=rf"{who}: bounds must be a pair \(lo, hi\) of floats or None"):
        fn(S, ones, bounds=3.0)
    for bad in ((3.0, 2.0), (1.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match=rf"{who}: bounds must satisfy lo <= hi and be finite"):
            fn(S, ones, bounds=bad)
    assert fn(S, ones, bounds=(-1.0, 12.0)).shape == (12,), "no definiteness is needed"


def test_max_terms_refusal_names_the_product_and_the_terms():
    S = _sparse(ER.laplacian7(3, 2, 2))
    ones = torch.ones(12, dtype=F64)
    K = ER.ive(100.0, 1e-6)[1]
    with pytest.raises(ValueError, match=rf"sparse_expm_mm: \|t\|·ρ = 100 needs K = {K} terms at tolerance 1e-06, above max_terms = 20"):
        sparse_expm_mm(S, ones, -20.0, bounds=(0.0, 10.0), max_terms=20)
    out, info = sparse_expm_mm(S, ones, -20.0, bounds=(0.0, 10.0), max_terms=K, return_info=True)
    assert info["terms"] == K and bool(torch.isfinite(out).all())
    with pytest.raises(ValueError, match=r"sparse_expm_mm: \|t\|·ρ = 5e\+09 needs about K = \d+ terms at tolerance 1e-06, above max_terms = 4096"):
        sparse_expm_mm(S, ones, -1e9, bounds=(0.0, 10.0))


def test_double_backward_raises():
    S = _sparse(ER.laplacian7(3, 2, 2), "coo")
    B = torch.ones(12, dtype=F64, requires_grad=True)
    out = sparse_expm_mm(S, B, -0.5)
    (g,) = torch.autograd.grad((out * out).sum(), B, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- the staged header --------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_EXPM == {"tsgu_hip_expm.h": _backend.SIGNATURES_EXPM}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR, _backend.STAGED_QUADRATURE,
              _backend.STAGED_CIQ)
    assert len(others) + 1 == 8, "the eight registries"
    assert not any(set(_backend.STAGED_EXPM) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_EXPM)
    assert not any(names & set(table) for reg in others for table in reg.values())
    every = [name for reg in others for table in reg.values() for name in table]
    assert len(every) == len(set(every)), "the eight registries are disjoint"
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_expm.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_EXPM)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_EXPM[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION
    src = os.path.join(os.path.dirname(STAGED_HEADER), "expm.hip")
    assert os.path.exists(src) and '#include "tsgu_hip_expm.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"


def test_geometry():
    tcap, ccap, align, rows, groups = _backend.expm_geometry(torch.float32, 1025, 16)
    assert tcap >= 8 and ccap >= 16 and align == 4 and rows > 0 and groups == -(-1025 // rows)
    assert _backend.expm_geometry(F64, 37, 3)[2] == 2
    assert _backend.expm_geometry(torch.float32, 10, 1024)[:2] == (tcap, ccap) == _backend.expm_geometry(F64, 10, 512)[:2]
    for dtype, p in ((torch.float32, 257), (torch.float32, 1028), (F64, 259), (F64, 514)):
        with pytest.raises(RuntimeError, match="simultaneous right-hand sides are not supported"):
            _backend.expm_geometry(dtype, 10, p)
    lib = _backend.load_library()
    slots = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64())
    refs = [ctypes.byref(x) for x in slots]
    assert lib.tsgu_expm_geometry(0, 10, 4, *refs) == A.OK
    assert lib.tsgu_expm_geometry(2, 10, 4, *refs) == A.BAD_DTYPE and lib.tsgu_expm_geometry(7, 10, 4, *refs) == A.BAD_DTYPE
    assert lib.tsgu_expm_geometry(0, 0, 4, *refs) == A.BAD_ARG and lib.tsgu_expm_geometry(0, 10, 0, *refs) == A.BAD_ARG
    for k in range(5):
        assert lib.tsgu_expm_geometry(0, 10, 4, *(None if j == k else r for j, r in enumerate(refs))) == A.BAD_ARG


# ---- host refusals: every call below is refused before the device is touched (the base call only by set_device(-1)) ------------------

BASE = {
    "tsgu_cheb_step": dict(vtype=0, n=100, p=16, prod=0x10000, x=0x20000, prev=0x30000, alpha=0.5, beta=0.5, gamma=1.0, src=0x40000,
                           src_slots=4, src_slot=1, chunk=0x50000, chunk_slots=4, slot=3, flags=0x60000),
    "tsgu_cheb_combine": dict(vtype=0, mode=0, accumulate=0, n=100, p=16, m=4, T=2, chunk=0x10000, coef=0x20000, planes=0x30000,
                              plane_stride=1600, flags=0x40000),
}
OPTIONAL = {"prod", "src", "chunk"}


def _call(name, **changes):
    a = dict(BASE[name])
    a.update(changes)
    return getattr(_backend.load_library(), name)(*a.values(), -1, None)


@pytest.mark.parametrize("name", list(BASE))
def test_host_refusals(name):
    params = dict(A.prototypes(STAGED_HEADER))[name]
    assert [q[0] for q in params[:-2]] == list(BASE[name]), "the base call names the header's parameters"
    tcap, ccap = _backend.expm_geometry(torch.float32, 100, 16)[:2]
    assert _call(name) == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    step = name == "tsgu_cheb_step"
    for pn, pt in params[:-2]:
        if pt.endswith("*") and not (step and pn in OPTIONAL):
            assert _call(name, **{pn: None}) == A.BAD_ARG, (name, pn)
    assert _call(name, vtype=2) == A.BAD_DTYPE and _call(name, vtype=7) == A.BAD_DTYPE
    assert _call(name, n=0) == A.BAD_ARG and _call(name, n=-1) == A.BAD_ARG
    assert _call(name, p=0) == A.BAD_ARG and _call(name, p=-1) == A.BAD_ARG
    assert _call(name, flags=BASE[name]["flags"] + 2) == A.BAD_ARG
    huge = dict(n=1 << 42, p=1) if step else dict(n=1 << 42, p=1, plane_stride=1 << 42)
    assert _call(name, **huge) == A.TOO_LARGE, "more workgroups than a grid holds"
    if step:
        for pn in ("prod", "x", "prev", "src", "chunk"):
            assert _call(name, **{pn: BASE[name][pn] + 4}) == A.BAD_ARG, f"{pn} must be 16-byte aligned"
        assert _call(name, prod=None) == A.BAD_ARG, "a NULL prod needs alpha == 0 ..."
        assert _call(name, prod=None, alpha=0.0) == A.BAD_ARG, "... and then reaches set_device, as a NULL src or chunk does"
        for ch in (dict(src_slots=0), dict(src_slot=-1), dict(src_slot=4), dict(chunk_slots=0), dict(slot=-1), dict(slot=4)):
            assert _call(name, **ch) == A.BAD_ARG, ch
        assert _call(name, src=None, src_slots=0, src_slot=9) == A.BAD_ARG, "the slot arguments of a NULL array are not read"
        assert _call(name, src_slots=ccap + 1) == A.TOO_LARGE and _call(name, chunk_slots=ccap + 1) == A.TOO_LARGE
        assert _call(name, p=257) == A.TOO_LARGE and _call(name, p=1028) == A.TOO_LARGE and _call(name, vtype=1, p=514) == A.TOO_LARGE
    else:
        for pn in ("chunk", "planes"):
            assert _call(name, **{pn: BASE[name][pn] + 4}) == A.BAD_ARG, f"{pn} must be 16-byte aligned"
        assert _call(name, coef=0x20002) == A.BAD_ARG and _call(name, vtype=1, coef=0x20004) == A.BAD_ARG, "coef: element alignment"
        for ch in (dict(m=0), dict(T=0), dict(mode=2), dict(mode=-1), dict(accumulate=2), dict(accumulate=-1), dict(mode=1, accumulate=1),
                   dict(plane_stride=1599), dict(plane_stride=1602), dict(vtype=1, plane_stride=1601)):
            assert _call(name, **ch) == A.BAD_ARG, ch
        assert _call(name, m=ccap + 1) == A.TOO_LARGE and _call(name, T=tcap + 1) == A.TOO_LARGE
        assert _call(name, p=257, plane_stride=25700) == A.TOO_LARGE and _call(name, vtype=1, p=514, plane_stride=51400) == A.TOO_LARGE
