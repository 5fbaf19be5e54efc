"""`sparse_logdet` / `sparse_inv_quad_logdet` without a GPU: the public surface and every refusal, the staged header
csrc/tsgu_hip_quadrature.h against its ctypes table and the library, the host refusals of both launchers (fake pointers,
device = -1: nothing is dereferenced), the probe function against its mirror, and the torch-op path on CPU tensors in fp64 against
`slogdet`, `inv` and `torch.autograd.gradcheck`.

Bounds.  With probes = I and 48 steps the quadrature of every column is exact (its Krylov space is exhausted before that: the
lengths are 19 to 35), so the value differs from `slogdet` by summation order only: 1e-9 relative is the margin, 5e-16 the
measurement.  A gradient entry is the (i, j) entry of the solution block U = A⁻¹ I: CG stops a column at a normalised residual below
`cg_tolerance`, so |U - A⁻¹|_max <= |A⁻¹|_2 cg_tolerance = cg_tolerance / λ_min.  The Rademacher case is a condition, not a
tolerance: |estimate - exact| <= 4 stderr fails for a correct estimator with probability below 1e-4, and the seed is fixed.
"""

import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import _abi_cases as A
import _quadrature_ref as QR
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _cpu, sparse_inv_quad_logdet, sparse_logdet
from torchsparsegradutils_amd.utils._operator import LAST_SOLVE

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_quadrature.h")
ENTRIES = ("tsgu_quadrature_geometry", "tsgu_tridiag_quadrature", "tsgu_rademacher_fill")
F64 = torch.float64


def _sparse(M, layout="csr", itype=torch.int64, dtype=F64):
    crow, col, val = QR.csr_arrays(M)
    n = M.shape[0]
    if layout == "csr":
        return torch.sparse_csr_tensor(torch.from_numpy(crow).to(itype), torch.from_numpy(col).to(itype), torch.from_numpy(val).to(dtype),
                                       (n, n))
    rows = np.repeat(np.arange(n), np.diff(crow))
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, col))), torch.from_numpy(val).to(dtype), (n, n)).coalesce()


@pytest.fixture(scope="module")
def matrices():
    out = {}
    for name, make in QR.MATRICES.items():
        M = make()
        lam = np.linalg.eigvalsh(M)
        out[name] = (M, float(np.linalg.slogdet(M)[1]), np.linalg.inv(M), float(lam[0]))
    return out


# ---- surface ----------------------------------------------------------------------------------------------------------------------

def test_surface_and_refusals():
    assert {"sparse_logdet", "sparse_inv_quad_logdet", "SparseLogDet"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_logdet import __all__ as mod_all

    assert sorted(mod_all) == ["SparseLogDet", "sparse_inv_quad_logdet", "sparse_logdet"]
    M = QR.laplacian5(3, 4, 0.5)
    S = _sparse(M)
    cap = _backend.quadrature_geometry()[0]
    eye = torch.eye(12, dtype=F64)
    out = sparse_logdet(S, probes=eye, lanczos_steps=12)
    assert out.shape == () and out.dtype == F64
    iq, ld = sparse_inv_quad_logdet(S, torch.ones(12, dtype=F64), probes=eye, lanczos_steps=12)
    assert iq.shape == () and ld.shape == ()
    iq, ld, info = sparse_inv_quad_logdet(S, torch.ones(12, 3, dtype=F64), probes=eye, lanczos_steps=12, return_info=True)
    assert iq.shape == (3,) and set(info) == {"estimates", "lengths", "iterations", "residual_norms", "stderr"}
    assert info["estimates"].shape == (12,) and info["lengths"].shape == (12,) and info["residual_norms"].shape == (15,)
    assert len(info["iterations"]) == 1 and LAST_SOLVE.info["sparse_logdet"]["iterations"] == info["iterations"][0]
    ones = torch.ones(12, dtype=F64)       # (A is checked before B)
    for fn in (sparse_logdet, lambda a, **kw: sparse_inv_quad_logdet(a, ones, **kw)):
        with pytest.raises(ValueError, match="A should be an instance of torch.Tensor"):
            fn(3)
        with pytest.raises(ValueError, match="A should be in either COO or CSR sparse format"):
            fn(torch.from_numpy(M))
        with pytest.raises(ValueError, match=r"A must be a 2-D sparse matrix \(batched operands are not supported\), got 3 dimensions"):
            fn(torch.stack((torch.from_numpy(M), torch.from_numpy(M))).to_sparse())
        with pytest.raises(ValueError, match=r"A must be square, got \(3, 4\)"):
            fn(torch.ones(3, 4, dtype=F64).to_sparse())
        with pytest.raises(ValueError, match="float32 and float64 operands only, got torch.bfloat16"):
            fn(torch.from_numpy(M).to(torch.bfloat16).to_sparse())
        for steps in (0, -1, cap + 1):
            with pytest.raises(ValueError, match=rf"lanczos_steps must lie in \[1, {cap}\], got {steps}"):
                fn(S, lanczos_steps=steps)
        with pytest.raises(ValueError, match="num_probes must be at least 1, got 0"):
            fn(S, num_probes=0)
        with pytest.raises(ValueError, match="max_cg_iter must be at least 1, got 0"):
            fn(S, max_cg_iter=0)
        with pytest.raises(ValueError, match=r"probes must be a dense \(12, k\) block, got \(11, 2\)"):
            fn(S, probes=torch.ones(11, 2, dtype=F64))
        with pytest.raises(ValueError, match="probes must have A's dtype, got torch.float32 and torch.float64"):
            fn(S, probes=torch.ones(12, 2))
    with pytest.raises(ValueError, match=r"sparse_inv_quad_logdet: B must have shape \(12,\) or \(12, m\), got \(11,\)"):
        sparse_inv_quad_logdet(S, torch.ones(11, dtype=F64))
    with pytest.raises(ValueError, match="sparse_inv_quad_logdet: B must have A's dtype, got torch.float32 and torch.float64"):
        sparse_inv_quad_logdet(S, torch.ones(12))
    with pytest.raises(ValueError, match=r"sparse_inv_quad_logdet: B must be a dense \(strided\) tensor"):
        sparse_inv_quad_logdet(S, None)
    with pytest.raises(RuntimeError, match=r"sparse_logdet: A is not positive definite \(a Lanczos tridiagonal has a non-positive "
                                           r"eigenvalue\)"):
        sparse_logdet(_sparse(M - 5.0 * np.eye(12)), probes=eye, lanczos_steps=12)
    with pytest.warns(UserWarning, match="CG terminated in 3 iterations with average residual norm"):
        sparse_logdet(S, probes=eye, lanczos_steps=2, max_cg_iter=3, cg_tolerance=1e-30)
    assert LAST_SOLVE.info["sparse_logdet"]["tolerance_reached"] is False


def test_double_backward_raises():
    S = _sparse(QR.laplacian5(3, 4, 0.5), "coo").requires_grad_(True)
    out = sparse_logdet(S, probes=torch.eye(12, dtype=F64), lanczos_steps=12)
    (g,) = torch.autograd.grad(out * out, S, create_graph=True)       # (the upstream gradient 2·out carries a graph)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.coalesce().values().sum().backward()


# ---- the staged header --------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_QUADRATURE == {"tsgu_hip_quadrature.h": _backend.SIGNATURES_QUADRATURE}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR)
    assert not any(set(_backend.STAGED_QUADRATURE) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_QUADRATURE)
    assert not any(names & set(table) for reg in others for table in reg.values())
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_quadrature.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_QUADRATURE)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_QUADRATURE[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION


def test_geometry():
    cap, work = _backend.quadrature_geometry()
    assert cap >= 128 and work == 3 * 8 * cap
    lib = _backend.load_library()
    a, b = ctypes.c_int(), ctypes.c_int64()
    assert lib.tsgu_quadrature_geometry(ctypes.byref(a), ctypes.byref(b)) == A.OK and (a.value, b.value) == (cap, work)
    assert lib.tsgu_quadrature_geometry(None, ctypes.byref(b)) == A.BAD_ARG
    assert lib.tsgu_quadrature_geometry(ctypes.byref(a), None) == A.BAD_ARG


# ---- host refusals: every call below is refused before the device is touched (the base call only by set_device(-1)) ------------------

BASE = {
    "tsgu_tridiag_quadrature": dict(vtype=0, kind=0, fn=0, r=30, p=16, coef=0x10000, scale=0x20000, out=0x30000, info=0x40000,
                                    work=0x50000),
    "tsgu_rademacher_fill": dict(vtype=0, n=100, p=16, seed=0, out=0x10000),
}
OPTIONAL = {"scale", "work"}


def _call(name, **changes):
    a = dict(BASE[name])
    a.update(changes)
    return getattr(_backend.load_library(), name)(*a.values(), -1, None)


@pytest.mark.parametrize("name", list(BASE))
def test_host_refusals(name):
    params = dict(A.prototypes(STAGED_HEADER))[name]
    assert [q[0] for q in params[:-2]] == list(BASE[name]), "the base call names the header's parameters"
    cap = _backend.quadrature_geometry()[0]
    assert _call(name) == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    for pn, pt in params[:-2]:
        if pt.endswith("*") and pn not in OPTIONAL:
            assert _call(name, **{pn: None}) == A.BAD_ARG, (name, pn)
    assert _call(name, vtype=2) == A.BAD_DTYPE and _call(name, vtype=7) == A.BAD_DTYPE
    assert _call(name, p=0) == A.BAD_ARG and _call(name, p=-1) == A.BAD_ARG
    if name == "tsgu_tridiag_quadrature":
        for ch in (dict(r=0), dict(r=-1), dict(kind=-1), dict(kind=2), dict(fn=-1), dict(fn=4)):
            assert _call(name, **ch) == A.BAD_ARG, ch
        assert _call(name, r=cap + 1) == A.TOO_LARGE
        # `work` and `scale` are optional up to 64 rows; above, a launch without `work` (or with a misaligned one) is refused as such
        assert _call(name, scale=None, work=None) == A.BAD_ARG and _call(name, r=64, work=None) == A.BAD_ARG
        for r in (65, cap):
            for work in (None, 0x50004):
                assert _call(name, r=r, work=work, vtype=1) == A.BAD_ARG, (r, work)
    else:
        assert _call(name, n=0) == A.BAD_ARG and _call(name, n=-1) == A.BAD_ARG
        assert _call(name, n=1 << 32) == A.TOO_LARGE and _call(name, n=1 << 31, p=1 << 10) == A.TOO_LARGE
        assert _call(name, seed=-1) == A.BAD_ARG and _call(name, seed=(1 << 63) - 1) == A.BAD_ARG      # any seed is a seed


# ---- the probe function -------------------------------------------------------------------------------------------------------------

def test_probe_function():
    # the mirror's values for a few (seed, i, c), written out: a change of the hash is a change of every seeded result
    want = {(0, 0, 0): 1, (0, 0, 2): -1, (0, 1, 1): -1, (0, 4, 0): -1, (0, 4, 3): -1}
    Z = _cpu.rademacher_fill(5, 4, 0, F64)
    for (seed, i, c), v in want.items():
        assert QR.rademacher(seed, 5, 4)[i, c] == v == float(Z[i, c]), (seed, i, c)
    for seed in (0, 1, 12345, -1, (1 << 40) + 3, 1 << 63):
        for n, p in ((1, 1), (7, 3), (130, 65)):
            got = _cpu.rademacher_fill(n, p, seed, torch.float32)
            assert got.dtype == torch.float32 and got.shape == (n, p)
            assert torch.equal(got.abs(), torch.ones(n, p)), "±1 only"
            assert np.array_equal(got.numpy().astype(np.float64), QR.rademacher(seed, n, p)), (seed, n, p)
    Z = QR.rademacher(3, 4096, 8)
    assert abs(Z.mean()) < 4 / np.sqrt(Z.size), "balanced"
    assert all(0.3 < (Z[:, a] != Z[:, b]).mean() < 0.7 for a in range(8) for b in range(a)), "distinct columns differ"
    assert all(0.3 < (QR.rademacher(s, 4096, 1) != QR.rademacher(s + 1, 4096, 1)).mean() < 0.7 for s in (0, 1, 7)), "distinct seeds differ"
    assert np.array_equal(_backend.rademacher_fill(9, 2, 5, F64, "cpu").numpy(), QR.rademacher(5, 9, 2))


# ---- the torch-op quadrature against the mirror ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", [0, 1, 2, 3])
def test_cpu_quadrature_matches_the_mirror(fn):
    M = QR.MATRICES["lap7x9"]()
    hist = QR.cg_history(M, np.eye(63), 48, np.float64)
    hist[:, :, 5] = 0.0                      # r_c = 0
    hist[7, 1, 6] = 0.0                      # a beta = 0 in the middle: only the leading block counts
    hist[9, 0, 7] = np.inf                   # an alpha that is not finite ends the matrix before its row
    scale = np.linspace(0.5, 2.0, 63)
    want, winfo, bound = QR.quadrature(hist, QR.KIND_CG, fn, scale)
    got, info = _cpu.tridiag_quadrature(torch.from_numpy(hist), 0, fn, scale=torch.from_numpy(scale))
    assert np.array_equal(info.numpy(), winfo) and winfo[5] == 0 and winfo[6] == 8 and winfo[7] == 9
    assert got[5] == 0 and np.all(np.abs(got.numpy() - want) <= bound)
    if fn == 3:
        assert np.allclose(got.numpy()[winfo > 0], scale[winfo > 0], rtol=1e-13)


# ---- the CPU path -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("name", list(QR.MATRICES))
def test_exact_with_identity_probes(matrices, name, layout):
    M, exact, inv, lam_min = matrices[name]
    n = M.shape[0]
    S = _sparse(M, layout, torch.int32 if layout == "csr" else torch.int64).requires_grad_(True)
    tol = 1e-10
    ld, info = sparse_logdet(S, probes=torch.eye(n, dtype=F64), lanczos_steps=48, cg_tolerance=tol, return_info=True)
    print(f"{name} {layout}: |logdet - slogdet| / |logdet| = {abs(float(ld) - exact) / abs(exact):.3e}, lengths "
          f"{int(info['lengths'].min())}..{int(info['lengths'].max())}, iterations {info['iterations']}")
    assert abs(float(ld) - exact) <= 1e-9 * abs(exact)
    assert abs(float(info["estimates"].sum()) - exact) <= 1e-9 * abs(exact)
    ld.backward()
    g = S.grad
    assert g.layout == S.layout
    if layout == "csr":
        assert g.crow_indices().dtype == torch.int32 and torch.equal(g.crow_indices(), S.crow_indices())
        assert torch.equal(g.col_indices(), S.col_indices())
    else:
        assert torch.equal(g._indices(), S._indices())
    mask = M != 0
    err = np.abs(g.to_dense().numpy() - inv)[mask].max()
    print(f"{name} {layout}: max gradient error on the pattern {err:.3e}, bound {tol / lam_min:.3e}")
    assert err <= tol / lam_min
    assert np.all(g.to_dense().numpy()[~mask] == 0)


def test_inv_quad_and_its_gradients(matrices):
    M, exact, inv, lam_min = matrices["rand96"]
    n = M.shape[0]
    rng = np.random.default_rng(3)
    Bn = rng.standard_normal((n, 3))
    S = _sparse(M).requires_grad_(True)
    B = torch.from_numpy(Bn).requires_grad_(True)
    tol = 1e-10
    iq, ld = sparse_inv_quad_logdet(S, B, probes=torch.eye(n, dtype=F64), lanczos_steps=48, cg_tolerance=tol)
    X = inv @ Bn
    assert abs(float(ld) - exact) <= 1e-9 * abs(exact)
    # x_j is off by at most |b_j| tol / λ_min in the 2-norm
    bn = np.linalg.norm(Bn, axis=0)
    assert np.all(np.abs(iq.detach().numpy() - (Bn * X).sum(0)) <= bn * bn * tol / lam_min)
    w = torch.tensor([0.5, -2.0, 1.0], dtype=F64)
    (iq * w).sum().backward()
    assert np.all(np.abs(B.grad.numpy() - 2 * X * w.numpy()) <= 2 * np.abs(w.numpy()) * bn * tol / lam_min)
    want = -(X * w.numpy()) @ X.T
    mask = M != 0
    xmax = np.abs(X).max()
    assert np.abs(S.grad.to_dense().numpy() - want)[mask].max() <= 3 * np.abs(w.numpy()).sum() * 2 * xmax * bn.max() * tol / lam_min


def _symmetric_parameterisation(M):
    """(indices (2, nnz), map (nnz,), theta0): values = theta[map], one theta per unordered pair, so that every perturbation gradcheck
    makes keeps A symmetric (CG is not defined otherwise)."""
    rows, cols = np.nonzero(M)
    pairs = {}
    pmap = np.array([pairs.setdefault((min(i, j), max(i, j)), len(pairs)) for i, j in zip(rows, cols)])
    theta = np.zeros(len(pairs))
    theta[pmap] = M[rows, cols]
    return torch.from_numpy(np.stack((rows, cols))), torch.from_numpy(pmap), torch.from_numpy(theta)


def test_gradcheck():
    M = QR.laplacian5(3, 4, 0.5)
    n = 12
    idx, pmap, theta = _symmetric_parameterisation(M)
    eye = torch.eye(n, dtype=F64)
    B0 = torch.from_numpy(np.random.default_rng(5).standard_normal((n, 2)))
    kw = dict(probes=eye, lanczos_steps=12, cg_tolerance=1e-13)

    def matrix(th):
        return torch.sparse_coo_tensor(idx, th[pmap], (n, n))

    def logdet(th):
        return sparse_logdet(matrix(th), **kw)

    def both(th, B):
        iq, ld = sparse_inv_quad_logdet(matrix(th), B, **kw)
        return iq.sum() + 0.5 * iq[1] + 2.0 * ld

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert torch.autograd.gradcheck(logdet, (theta.clone().requires_grad_(True),), eps=1e-6, atol=1e-7, rtol=1e-6)
        assert torch.autograd.gradcheck(both, (theta.clone().requires_grad_(True), B0.clone().requires_grad_(True)), eps=1e-6, atol=1e-7,
                                        rtol=1e-6)


def test_rademacher_estimate_within_four_standard_errors():
    M = QR.laplacian5(32, 32, 0.5)
    exact = float(np.linalg.slogdet(M)[1])
    S = _sparse(M)
    est, info = sparse_logdet(S, num_probes=64, lanczos_steps=30, seed=0, return_info=True)
    stderr = float(info["stderr"])
    print(f"Rademacher fp64: estimate {float(est):.6f}, exact {exact:.6f}, stderr {stderr:.4f}, |error| / stderr "
          f"{abs(float(est) - exact) / stderr:.3f}")
    assert info["estimates"].shape == (64,) and abs(float(info["estimates"].mean()) - float(est)) <= 1e-12 * abs(exact)
    assert abs(float(est) - exact) <= 4 * stderr
    again = sparse_logdet(S, num_probes=64, lanczos_steps=30, seed=0)
    assert float(again) == float(est), "a seed reproduces an estimate"
    assert float(sparse_logdet(S, num_probes=64, lanczos_steps=30, seed=1)) != float(est)
    Z = _cpu.rademacher_fill(1024, 64, 0, F64)
    assert float(sparse_logdet(S, probes=Z, lanczos_steps=30)) == pytest.approx(float(est), rel=1e-13)
