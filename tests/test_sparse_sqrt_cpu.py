"""`sparse_inv_sqrt_mm` / `sparse_sqrt_mm` without a GPU: the quadrature rule against scipy and against its own scalar error, the
torch-op path on CPU tensors in fp64 against dense `eigh` and `torch.autograd.gradcheck`, the bounds estimate, every refusal, the
staged header csrc/tsgu_hip_ciq.h against its ctypes table and the library, and the host refusals of the launchers (fake pointers,
device = -1: nothing is dereferenced).

Bounds.  The rule's nodes and weights match scipy's elliptic functions to 1e-12 relative (both evaluate (u | m') for the same rounded
m' = 1 - lo/hi and the nodes u_q = (q - 1/2)·K'/N rounded left to right, as the formula is written).  At (0.3, 7e6, 15), m' = 1 - 4e-8,
that margin is scipy's own: measured 2.2e-13 (sigma) and 2.5e-13 (omega), but scipy's ellipj moves by 1.9e-12 when one u is changed
by one ulp there and is 1.3e-12 from a 40-digit evaluation, the package's recurrence 1.2e-13 and 5.4e-13.  The scalar error bounds are ten times the float64 measurements of the method's own table.  The
forward bound, 1e-10 relative to the largest entry, is the issue's: the rule's error on the exact spectrum is 1.4e-15 at N = 12 and
MINRES at tolerance 1e-13 leaves 1e-13·sqrt(kappa) at most.  Estimated bounds were checked for the seeds 0 ... 7.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _ciq_ref as CR
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_inv_sqrt_mm, sparse_sqrt_mm
from torchsparsegradutils_amd.sparse_sqrt import SparseInvSqrtMM, _ciq_rule

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_ciq.h")
ENTRIES = ("tsgu_ciq_geometry", "tsgu_ciq_update", "tsgu_ciq_stop")
F64 = torch.float64
SEEDS = tuple(range(8))


def _sparse(M, layout="csr", itype=torch.int64, dtype=F64):
    crow, col, val = CR.csr_arrays(M)
    n = M.shape[0]
    if layout == "csr":
        return torch.sparse_csr_tensor(torch.from_numpy(crow).to(itype), torch.from_numpy(col).to(itype), torch.from_numpy(val).to(dtype),
                                       (n, n))
    rows = np.repeat(np.arange(n), np.diff(crow))
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, col))).to(itype), torch.from_numpy(val).to(dtype), (n, n)).coalesce()


@pytest.fixture(scope="module")
def cases():
    """name -> (M, M^-1/2, M^1/2, eigenvalues, B (n, 3)): computed once, never written to."""
    rng = np.random.default_rng(5)
    out = {}
    for name, make in CR.MATRICES.items():
        M = make()
        inv_sqrt, lam = CR.dense_power(M, -0.5)
        sqrt, _ = CR.dense_power(M, 0.5)
        out[name] = (M, inv_sqrt, sqrt, lam, rng.standard_normal((M.shape[0], 3)))
    return out


# ---- the rule -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lo,hi,N", [(1.0, 1e2, 8), (1.0, 1e4, 12), (0.3, 7e6, 15)])
def test_rule_matches_scipy(lo, hi, N):
    special = pytest.importorskip("scipy.special")
    sigma, omega = _ciq_rule(lo, hi, N)
    want_s, want_w = CR.rule(lo, hi, N, functions=(special.ellipk, special.ellipj))
    print(f"rule ({lo}, {hi}, {N}): sigma {np.abs(sigma / want_s - 1).max():.2e}  omega {np.abs(omega / want_w - 1).max():.2e}")
    assert sigma.dtype == np.float64 and omega.dtype == np.float64 and sigma.shape == omega.shape == (N,)
    assert np.all(np.abs(sigma / want_s - 1.0) <= 1e-12) and np.all(np.abs(omega / want_w - 1.0) <= 1e-12)


@pytest.mark.parametrize("kappa,N,bound", [(1e4, 12, 1e-7), (1e6, 15, 1e-6), (1e2, 12, 1e-12)])
def test_rule_scalar_error(kappa, N, bound):
    sigma, omega = _ciq_rule(1.0, kappa, N)
    err = CR.scalar_error(sigma, omega, np.geomspace(1.0, kappa, 2001))
    print(f"kappa {kappa:g} N {N}: max |r(x) sqrt(x) - 1| = {err:.2e}")
    assert err <= bound
    mirror_s, mirror_w = CR.rule(1.0, kappa, N)
    assert np.allclose(sigma, mirror_s, rtol=1e-13, atol=0) and np.allclose(omega, mirror_w, rtol=1e-13, atol=0)


@pytest.mark.parametrize("lo,hi,N", [(1.0, 1e2, 8), (1.0, 1e4, 12), (0.3, 7e6, 15), (1e-3, 1e3, 32), (2.0, 2.0, 1), (0.65, 7.95, 12)])
def test_rule_is_positive_and_ordered(lo, hi, N):
    sigma, omega = _ciq_rule(lo, hi, N)
    assert np.all(sigma > 0) and np.all(np.diff(sigma) > 0) and np.all(omega > 0)
    assert np.all(np.isfinite(sigma)) and np.all(np.isfinite(omega))


def test_rule_refuses_bad_intervals():
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (2.0, 1.0), (1.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="0 < lo <= hi expected"):
            _ciq_rule(lo, hi, 8)


# ---- the torch-op path ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.MATRICES))
@pytest.mark.parametrize("layout", ["coo", "csr"])
@pytest.mark.parametrize("p", [1, 3])
def test_cpu_forward(cases, name, layout, p):
    M, inv_sqrt, sqrt, lam, B = cases[name]
    S = _sparse(M, layout)
    Bt = torch.from_numpy(B[:, 0].copy() if p == 1 else B.copy())     # p = 1: a vector B
    kw = dict(bounds=(float(lam[0]), float(lam[-1])), tolerance=1e-13, num_quad=12)
    for fn, dense in ((sparse_inv_sqrt_mm, inv_sqrt), (sparse_sqrt_mm, sqrt)):
        want = dense @ Bt.numpy()
        got = fn(S, Bt, **kw)
        assert got.shape == Bt.shape and got.dtype == F64
        err = float(np.abs(got.numpy() - want).max() / np.abs(want).max())
        print(f"{fn.__name__} {name} {layout} p {p}: rel err {err:.2e}")
        assert err <= 1e-10
    again = sparse_inv_sqrt_mm(S, Bt, **kw)
    assert torch.equal(again, sparse_inv_sqrt_mm(S, Bt, **kw))


def test_zero_column_and_info(cases):
    M, inv_sqrt, _, lam, B = cases["lap6x7"]
    Bz = B.copy()
    Bz[:, 1] = 0.0
    out, info = sparse_inv_sqrt_mm(_sparse(M), torch.from_numpy(Bz), bounds=(float(lam[0]), float(lam[-1])), tolerance=1e-13,
                                   return_info=True)
    assert torch.equal(out[:, 1], torch.zeros(42, dtype=F64))
    assert np.abs(out.numpy() - inv_sqrt @ Bz).max() <= 1e-10 * np.abs(inv_sqrt @ Bz).max()
    assert set(info) == {"iterations", "converged", "bounds", "num_quad", "residual_estimates", "fused"}
    assert info["bounds"] == (float(lam[0]), float(lam[-1])) and info["num_quad"] == 12 and info["fused"] is False
    assert info["residual_estimates"].shape == (3,) and float(info["residual_estimates"][1]) == 0.0


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_gradcheck(layout):
    M = CR.laplacian5(3, 4, 0.3)                                       # n = 12
    lam = np.linalg.eigvalsh(M)
    S = _sparse(M, layout)
    kw = dict(bounds=(float(lam[0]), float(lam[-1])), tolerance=1e-13, num_quad=12)
    B = torch.randn(12, 2, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda b: sparse_inv_sqrt_mm(S, b, **kw), (B,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda b: sparse_sqrt_mm(S, b[:, 0], **kw), (B,), eps=1e-6, atol=1e-7, rtol=1e-6)
    crow, col, _ = CR.csr_arrays(M)
    rows = np.repeat(np.arange(12), np.diff(crow))
    mirror = torch.from_numpy(np.searchsorted(rows * 12 + col, col * 12 + rows))       # position of (j, i) for the entry (i, j)
    # MINRES is a solver for symmetric matrices: a finite difference in ONE stored value would hand it an unsymmetric matrix, for
    # which it does not compute r(A) B.  The wrapper rebuilds A from (v + v mirrored) / 2, so every perturbation is symmetric and
    # the chain rule tests the stored-entry gradient g through (g_ij + g_ji) / 2.
    if layout == "csr":
        ci, cc = S.crow_indices(), S.col_indices()
        rebuild = lambda v: torch.sparse_csr_tensor(ci, cc, 0.5 * (v + v[mirror]), (12, 12))              # noqa: E731
    else:
        idx = S.indices()
        rebuild = lambda v: torch.sparse_coo_tensor(idx, 0.5 * (v + v[mirror]), (12, 12)).coalesce()      # noqa: E731
    values = S.values().clone().requires_grad_(True)
    Bc = B.detach()
    for fn in (sparse_inv_sqrt_mm, sparse_sqrt_mm):
        assert torch.autograd.gradcheck(lambda v: fn(rebuild(v), Bc, **kw), (values,), eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_grad_a_matches_the_dense_formula_on_as_own_indices(cases, layout):
    M, _, _, lam, B = cases["lap6x7"]
    S = _sparse(M, layout, itype=torch.int32 if layout == "csr" else torch.int64).requires_grad_(True)
    Bt = torch.from_numpy(B.copy()).requires_grad_(True)
    G = np.random.default_rng(9).standard_normal(B.shape)
    bounds = (float(lam[0]), float(lam[-1]))
    out = sparse_inv_sqrt_mm(S, Bt, bounds=bounds, tolerance=1e-13)
    out.backward(torch.from_numpy(G))
    sigma, omega = _ciq_rule(*bounds, 12)
    dense = CR.grad_a_dense(M, B, G, sigma, omega)
    g = S.grad
    assert g.layout == S.layout and g.shape == S.shape
    if layout == "csr":
        assert torch.equal(g.crow_indices(), S.crow_indices()) and torch.equal(g.col_indices(), S.col_indices())
        assert g.col_indices().dtype == torch.int32 and g.crow_indices().dtype == torch.int32
        rows = np.repeat(np.arange(42), np.diff(S.crow_indices().numpy()))
        cols = S.col_indices().numpy()
        got = g.values().detach().numpy()
    else:
        assert g._indices().data_ptr() == S._indices().data_ptr(), "the gradient is built on A's own index tensor"
        rows, cols = S._indices().numpy()
        got = g._values().detach().numpy()
    want = dense[rows, cols]
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    rA, _ = CR.dense_power(M, -0.5)
    assert np.abs(Bt.grad.numpy() - rA @ G).max() <= 1e-10 * np.abs(rA @ G).max()


def test_uncoalesced_coo_is_coalesced_first(cases):
    M, inv_sqrt, _, lam, B = cases["lap6x7"]
    C = _sparse(M, "coo")
    idx = torch.cat((C.indices(), C.indices()), dim=1)
    val = torch.cat((0.25 * C.values(), 0.75 * C.values()))
    U = torch.sparse_coo_tensor(idx, val, C.shape)
    assert not U.is_coalesced()
    got = sparse_inv_sqrt_mm(U, torch.from_numpy(B.copy()), bounds=(float(lam[0]), float(lam[-1])), tolerance=1e-13)
    assert np.abs(got.numpy() - inv_sqrt @ B).max() <= 1e-10 * np.abs(inv_sqrt @ B).max()


# ---- estimated bounds -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.MATRICES))
def test_estimated_bounds_enclose_the_spectrum(cases, name):
    M, inv_sqrt, _, lam, B = cases[name]
    S = _sparse(M)
    Bt = torch.from_numpy(B.copy())
    want = inv_sqrt @ B
    for seed in SEEDS:
        out, info = sparse_inv_sqrt_mm(S, Bt, seed=seed, tolerance=1e-13, return_info=True)
        lo, hi = info["bounds"]
        print(f"{name} seed {seed}: bounds ({lo:.4f}, {hi:.4f}) for a spectrum in [{lam[0]:.4f}, {lam[-1]:.4f}]")
        assert lo <= lam[0] * 1.0 and hi >= lam[-1]
        assert lo >= 0.25 * lam[0] and hi <= 1.2 * lam[-1], "half / 1.1 times a Ritz value inside the spectrum"
        # a rule for the widened interval (kappa below 50): 1e-9 covers N = 12 there (the table: 4.6e-14 at kappa 1e2)
        assert np.abs(out.numpy() - want).max() <= 1e-9 * np.abs(want).max()
    a = sparse_inv_sqrt_mm(S, Bt, seed=3)
    assert torch.equal(a, sparse_inv_sqrt_mm(S, Bt, seed=3)), "the same seed gives the same bits"


def test_not_positive_definite_raises(cases):
    M = cases["lap6x7"][0]
    with pytest.raises(ValueError, match=r"sparse_inv_sqrt_mm: A is not positive definite \(a Lanczos tridiagonal has a non-positive "
                                         r"eigenvalue\)"):
        sparse_inv_sqrt_mm(_sparse(M - 5.0 * np.eye(42)), torch.ones(42, dtype=F64))
    with pytest.raises(ValueError, match="sparse_sqrt_mm: A is not positive definite"):
        sparse_sqrt_mm(_sparse(-M), torch.ones(42, dtype=F64))


# ---- surface ----------------------------------------------------------------------------------------------------------------------------

def test_surface_and_refusals():
    assert {"sparse_inv_sqrt_mm", "sparse_sqrt_mm", "SparseInvSqrtMM"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_sqrt import __all__ as mod_all

    assert sorted(mod_all) == ["SparseInvSqrtMM", "sparse_inv_sqrt_mm", "sparse_sqrt_mm"]
    assert tsgu.SparseInvSqrtMM is SparseInvSqrtMM and issubclass(SparseInvSqrtMM, torch.autograd.Function)
    for fn in (sparse_inv_sqrt_mm, sparse_sqrt_mm):
        assert "GMRF" in fn.__doc__ or "draw from" in fn.__doc__
        assert "Preconditioning is not supported" in fn.__doc__
    assert "whitens" in sparse_inv_sqrt_mm.__doc__
    M = CR.laplacian5(3, 4, 0.5)
    S = _sparse(M)
    ones = torch.ones(12, dtype=F64)
    for fn in (sparse_inv_sqrt_mm, sparse_sqrt_mm):
        who = fn.__name__
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
        for nq in (0, -1, 33):
            with pytest.raises(ValueError, match=rf"{who}: num_quad must lie in \[1, 32\], got {nq}"):
                fn(S, ones, num_quad=nq)
        with pytest.raises(ValueError, match=f"{who}: max_iter must be at least 1, got 0"):
            fn(S, ones, max_iter=0)
        with pytest.raises(ValueError, match=f"{who}: tolerance must be positive, got 0"):
            fn(S, ones, tolerance=0.0)
        with pytest.raises(ValueError, match=f"{who}: lanczos_steps must be at least 1, got 0"):
            fn(S, ones, lanczos_steps=0)
        with pytest.raises(ValueError, match=rf"{who}: bounds must be a pair \(lo, hi\) of floats or None"):
            fn(S, ones, bounds=(1.0, 2.0, 3.0))
        with pytest.raises(ValueError, match=rf"{who}: bounds must be a pair \(lo, hi\) of floats or None"):
            fn(S, ones, bounds=3.0)
        for bad in ((0.0, 1.0), (-1.0, 2.0), (3.0, 2.0), (1.0, float("inf"))):
            with pytest.raises(ValueError, match=rf"{who}: bounds must satisfy 0 < lo <= hi"):
                fn(S, ones, bounds=bad)
    rand = torch.from_numpy(np.random.default_rng(2).standard_normal(12))      # (the ones vector lies in a 4-dimensional Krylov space)
    out, info = sparse_inv_sqrt_mm(S, rand, max_iter=3, tolerance=1e-14, bounds=(0.5, 8.5), return_info=True)
    assert info["converged"] is False and out.shape == (12,), "a run that ends at max_iter reports it and does not raise"


def test_double_backward_raises():
    S = _sparse(CR.laplacian5(3, 4, 0.5), "coo")
    B = torch.ones(12, dtype=F64, requires_grad=True)
    out = sparse_inv_sqrt_mm(S, B, bounds=(0.5, 8.5))
    (g,) = torch.autograd.grad((out * out).sum(), B, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- the staged header --------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_CIQ == {"tsgu_hip_ciq.h": _backend.SIGNATURES_CIQ}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR, _backend.STAGED_QUADRATURE)
    assert not any(set(_backend.STAGED_CIQ) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_CIQ)
    assert not any(names & set(table) for reg in others for table in reg.values())
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_ciq.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_CIQ)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_CIQ[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION
    src = os.path.join(os.path.dirname(STAGED_HEADER), "ciq.hip")
    assert os.path.exists(src) and '#include "tsgu_hip_ciq.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"


def test_geometry():
    cap, align, rows, groups = _backend.ciq_geometry(torch.float32, 1025, 16)
    assert cap >= 32 and align == 4 and rows > 0 and groups == -(-1025 // rows)
    assert _backend.ciq_geometry(F64, 37, 3)[1] == 2
    assert _backend.ciq_geometry(torch.float32, 10, 1024)[0] == cap and _backend.ciq_geometry(F64, 10, 512)[0] == cap
    for dtype, p in ((torch.float32, 257), (torch.float32, 1028), (F64, 259), (F64, 514)):
        with pytest.raises(RuntimeError, match="simultaneous right-hand sides are not supported"):
            _backend.ciq_geometry(dtype, 10, p)
    lib = _backend.load_library()
    a, b, c, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    refs = [ctypes.byref(x) for x in (a, b, c, d)]
    assert lib.tsgu_ciq_geometry(0, 10, 4, *refs) == A.OK
    assert lib.tsgu_ciq_geometry(2, 10, 4, *refs) == A.BAD_DTYPE and lib.tsgu_ciq_geometry(7, 10, 4, *refs) == A.BAD_DTYPE
    assert lib.tsgu_ciq_geometry(0, 0, 4, *refs) == A.BAD_ARG and lib.tsgu_ciq_geometry(0, 10, 0, *refs) == A.BAD_ARG
    for k in range(4):
        assert lib.tsgu_ciq_geometry(0, 10, 4, *(None if j == k else r for j, r in enumerate(refs))) == A.BAD_ARG


# ---- host refusals: every call below is refused before the device is touched (the base call only by set_device(-1)) ------------------

BASE = {
    "tsgu_ciq_update": dict(vtype=0, n=100, p=16, n_shift=12, zc=0x10000, zp=0x20000, wpp=0x30000, wp=0x40000, shift_stride=1600,
                            acc=0x50000, keep=0x60000, scal=0x70000, omega=0x80000, done=0x90000, flags=0xA0000),
    "tsgu_ciq_stop": dict(vtype=0, p=16, n_shift=12, scal=0x10000, tol=1e-4, est=0x20000, done=0x30000, flags=0x40000),
}
OPTIONAL = {"keep"}


def _call(name, **changes):
    a = dict(BASE[name])
    a.update(changes)
    return getattr(_backend.load_library(), name)(*a.values(), -1, None)


@pytest.mark.parametrize("name", list(BASE))
def test_host_refusals(name):
    params = dict(A.prototypes(STAGED_HEADER))[name]
    assert [q[0] for q in params[:-2]] == list(BASE[name]), "the base call names the header's parameters"
    cap = _backend.ciq_geometry(torch.float32, 100, 16)[0]
    assert _call(name) == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    for pn, pt in params[:-2]:
        if pt.endswith("*") and pn not in OPTIONAL:
            assert _call(name, **{pn: None}) == A.BAD_ARG, (name, pn)
    assert _call(name, vtype=2) == A.BAD_DTYPE and _call(name, vtype=7) == A.BAD_DTYPE
    assert _call(name, p=0) == A.BAD_ARG and _call(name, p=-1) == A.BAD_ARG
    assert _call(name, n_shift=0) == A.BAD_ARG and _call(name, n_shift=-1) == A.BAD_ARG
    assert _call(name, n_shift=cap + 1) == A.TOO_LARGE
    if name == "tsgu_ciq_update":
        assert _call(name, n=0) == A.BAD_ARG and _call(name, n=-1) == A.BAD_ARG
        for pn in ("zc", "zp", "wpp", "wp", "acc", "keep"):
            assert _call(name, **{pn: BASE[name][pn] + 4}) == A.BAD_ARG, f"{pn} must be 16-byte aligned"
        for pn in ("scal", "omega", "done", "flags"):
            assert _call(name, **{pn: BASE[name][pn] + 2}) == A.BAD_ARG, f"{pn} must be aligned to its element"
        assert _call(name, vtype=1, scal=0x70004) == A.BAD_ARG and _call(name, vtype=1, omega=0x80004) == A.BAD_ARG
        assert _call(name, shift_stride=1599) == A.BAD_ARG, "planes may not overlap"
        assert _call(name, shift_stride=1602) == A.BAD_ARG and _call(name, vtype=1, shift_stride=1601) == A.BAD_ARG, "16-byte planes"
        assert _call(name, keep=None) == A.BAD_ARG, "keep is optional: this reaches set_device"
        assert _call(name, p=257, shift_stride=25700) == A.TOO_LARGE, "above 256 columns only multiples of the 16-byte lane"
        assert _call(name, p=1028, shift_stride=102800) == A.TOO_LARGE and _call(name, vtype=1, p=514, shift_stride=51400) == A.TOO_LARGE
        assert _call(name, n=1 << 42, p=1, shift_stride=1 << 42) == A.TOO_LARGE, "more workgroups than a grid holds"
    else:
        for pn in ("scal", "est", "done", "flags"):
            assert _call(name, **{pn: BASE[name][pn] + 2}) == A.BAD_ARG, f"{pn} must be aligned to its element"
        assert _call(name, vtype=1, est=0x20004) == A.BAD_ARG
