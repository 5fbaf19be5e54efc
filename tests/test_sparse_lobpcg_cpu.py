"""sparse_lobpcg without a GPU: the numpy restatement on every case, the public API on CPU operands against the float64 spectrum
(eigenvalues, orthonormality, gradient, gradcheck), the restart path, every refusal, the staged C-ABI header against
`_backend.SIGNATURES_LOBPCG`, and the host-side refusals of the three launchers."""

import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _lobpcg_ref as lr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_lobpcg, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED_HEADER = os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "tsgu_hip_lobpcg.h")
DTYPES = {"float32": (torch.float32, np.float32), "float64": (torch.float64, np.float64)}
OPERANDS = [("coo", torch.int64), ("csr", torch.int32), ("csr", torch.int64)]


def operand(name, dtype, layout="csr", itype=torch.int64, device="cpu"):
    ptr, idx, val, k, D, _ = lr.case(name)
    n = D.shape[0]
    csr = torch.sparse_csr_tensor(torch.from_numpy(ptr).to(itype), torch.from_numpy(idx).to(itype), torch.from_numpy(val).to(dtype), (n, n))
    return (csr if layout == "csr" else csr.to_sparse_coo().coalesce()).to(device)


@functools.lru_cache(maxsize=None)
def restated(name, dt, largest):
    _, _, _, k, D, _ = lr.case(name)
    return lr.lobpcg(D, lr.initial_block(D.shape[0], k), largest=largest, niter=lr.NITER, dtype=DTYPES[dt][1])


@functools.lru_cache(maxsize=None)
def solved(name, dt, largest, layout="csr", itype=torch.int64, device="cpu"):
    """(eigenvalues, eigenvectors as float64 numpy arrays, last_solve_info) of the package on a named case."""
    _, _, _, k, D, _ = lr.case(name)
    tdt = DTYPES[dt][0]
    X = torch.from_numpy(lr.initial_block(D.shape[0], k)).to(tdt).to(device)
    lam, V = sparse_lobpcg(operand(name, tdt, layout, itype, device), k, X=X, largest=largest, niter=lr.NITER)
    return lam.double().cpu().numpy(), V.double().cpu().numpy(), dict(utils.last_solve_info("lobpcg"))


def check_pairs(name, dt, largest, lam, V, info):
    """The eigenvalue criterion of the issue, per pair, and the reported residual of a converged solve."""
    _, _, _, k, D, spectrum = lr.case(name)
    u = lr.unit_roundoff(DTYPES[dt][1])
    err, bound = lr.eigenvalue_bounds(D, spectrum, lam, V, largest, u)
    print(f"{name} {dt} largest={largest}: iterations {info['iterations']}, restarts {info['restarts']}, |err| {err}, bound {bound}")
    assert np.all(np.isfinite(lam)) and np.all(err <= bound), (err, bound)
    assert info["converged"] and not info["breakdown"], info
    assert max(info["residual_norms"]) <= info["tolerance"] * info["a_norm"]
    if largest:
        assert np.all(np.diff(lam) <= 0)
    else:
        assert np.all(np.diff(lam) >= 0)
    return err, bound


def test_exports():
    assert {"sparse_lobpcg", "SparseLOBPCG"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_lobpcg import __all__ as mod_all

    assert mod_all == ["sparse_lobpcg", "SparseLOBPCG"]
    assert tsgu.sparse_lobpcg is sparse_lobpcg and issubclass(tsgu.SparseLOBPCG, torch.autograd.Function)
    assert callable(utils.lobpcg)
    solved("coupled", "float64", True)
    info = utils.last_solve_info("lobpcg")
    assert info["solver"] == "lobpcg" and {"iterations", "converged_columns", "residual_norms", "restarts"} <= set(info)


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_the_restatement_converges_within_niter(name, dt, largest):
    lam, V, info = restated(name, dt, largest)
    _, _, _, _, D, spectrum = lr.case(name)
    err, bound = lr.eigenvalue_bounds(D, spectrum, lam, V, largest, lr.unit_roundoff(DTYPES[dt][1]))
    assert info["converged"] and 2 * info["iterations"] <= lr.NITER, info
    assert np.all(err <= bound)


@pytest.mark.parametrize("layout,itype", OPERANDS)
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_eigenvalues_against_the_float64_spectrum(name, dt, largest, layout, itype):
    lam, V, info = solved(name, dt, largest, layout, itype)
    check_pairs(name, dt, largest, lam, V, info)


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_orthonormality_against_the_restatement(name, dt, largest):
    """‖V̂ᵀV̂ − I‖_max of the package against four times what the numpy restatement at the same dtype leaves on the same input, plus
    k·u.  Measured on the CPU path over the twenty cases: float32 5.0e-8 … 7.1e-7 against 3.9e-8 … 5.2e-7 of the restatement,
    float64 4.4e-16 … 1.3e-15 against 2.2e-16 … 1.3e-15."""
    k = lr.CASES[name][1]
    u = lr.unit_roundoff(DTYPES[dt][1])
    got = lr.orthonormality(solved(name, dt, largest)[1])
    ref = lr.orthonormality(restated(name, dt, largest)[1])
    print(f"{name} {dt} largest={largest}: package {got:.3e}, restatement {ref:.3e}")
    assert got <= 4 * ref + k * u


def gradient_case(name, dt, largest, device="cpu"):
    """(gradient values at A's stored positions, the reference's, the per-entry tolerance of the issue, A, A.grad)."""
    ptr, idx, val, k, D, spectrum = lr.case(name)
    tdt, ndt = DTYPES[dt]
    u = lr.unit_roundoff(ndt)
    n = D.shape[0]
    w = torch.from_numpy(np.random.default_rng(7).standard_normal(k))
    Asp = operand(name, tdt, device=device).requires_grad_(True)
    X = torch.from_numpy(lr.initial_block(n, k)).to(tdt).to(device)
    lam, V = sparse_lobpcg(Asp, k, X=X, largest=largest, niter=lr.NITER)
    assert not V.requires_grad and lam.requires_grad
    (w.to(tdt).to(device) * lam).sum().backward()
    Ad = torch.from_numpy(D).clone().requires_grad_(True)
    ev = torch.linalg.eigvalsh(Ad)
    (w * (ev.flip(0)[:k] if largest else ev[:k])).sum().backward()
    rows = np.repeat(np.arange(n), np.diff(ptr))
    want = Ad.grad.numpy()[rows, idx]
    res = lr.pair_residuals(D, lam.detach().double().cpu().numpy(), V.double().cpu().numpy())
    aw = np.abs(w.numpy())
    tol = float(np.sum(aw * 2 * res / lr.gaps(spectrum, k, largest)) + 8 * k * u * aw.sum())
    return Asp.grad.values().double().cpu().numpy(), want, tol, Asp


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", ["coupled", "stencil27"])
def test_gradient_against_dense_eigvalsh(name, dt, largest):
    got, want, tol, Asp = gradient_case(name, dt, largest)
    print(f"{name} {dt} largest={largest}: max |err| {np.abs(got - want).max():.3e}, tolerance {tol:.3e}")
    assert np.all(np.abs(got - want) <= tol)
    g = Asp.grad
    assert g.layout == torch.sparse_csr and g.dtype == Asp.dtype and g.shape == Asp.shape
    assert torch.equal(g.crow_indices(), Asp.crow_indices()) and torch.equal(g.col_indices(), Asp.col_indices())
    assert g.crow_indices().dtype == Asp.crow_indices().dtype


def test_gradient_keeps_a_coo_operands_layout_and_indices():
    Asp = operand("coupled", torch.float64, "coo").requires_grad_(True)
    X = torch.from_numpy(lr.initial_block(200, 3))
    lam, _ = sparse_lobpcg(Asp, 3, X=X, largest=False, niter=lr.NITER)
    lam.sum().backward()
    assert Asp.grad.layout == torch.sparse_coo and torch.equal(Asp.grad._indices(), Asp._indices())


def test_gradcheck_float64_on_12_rows():
    """Through one parameter per unordered pair {i, j}, so that every perturbed matrix is symmetric — the operand the function is
    defined for; a one-sided perturbation has no eigenpair the residual test could accept."""
    ptr, idx = lr.band(12, 2)
    rows = np.repeat(np.arange(12), np.diff(ptr))
    val = lr.dominant_values(ptr, idx, seed=2, symmetric=True) + np.where(idx == rows, 2.0 * rows, 0.0)      # (well separated eigenvalues)
    pairs, rep = np.unique(np.minimum(rows, idx) * 12 + np.maximum(rows, idx), return_inverse=True)
    theta0 = np.zeros(len(pairs))
    theta0[rep] = val
    crow, col, rep = torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(rep)
    X = torch.from_numpy(lr.initial_block(12, 2))
    seen = []

    def f(theta):
        lam = sparse_lobpcg(torch.sparse_csr_tensor(crow, col, theta[rep], (12, 12)), 2, X=X, largest=False, niter=500, tol=1e-12)[0]
        seen.append(utils.last_solve_info("lobpcg")["converged"])
        return lam

    theta = torch.from_numpy(theta0).requires_grad_(True)
    assert torch.autograd.gradcheck(f, (theta,), eps=1e-6, atol=1e-7)
    assert all(seen)


def test_a_rank_deficient_start_and_preconditioner_never_raise():
    """An initial block with two equal columns is perturbed (counted under `perturbations`, not `restarts`); a rank-2 projector as
    the preconditioner of three columns then ends the loop on the Cholesky of W's Gram matrix, with finite pairs and a flag."""
    n, k = 200, 3
    Asp = operand("coupled", torch.float64)
    X = torch.from_numpy(lr.initial_block(n, k))
    X[:, 1] = X[:, 0]
    Q = torch.linalg.qr(torch.from_numpy(np.random.default_rng(1).standard_normal((n, 2)))).Q
    lam, V = sparse_lobpcg(Asp, k, X=X, preconditioner=Q @ Q.t(), largest=False, niter=50)
    info = utils.last_solve_info("lobpcg")
    assert bool(torch.isfinite(lam).all()) and bool(torch.isfinite(V).all())
    assert info["perturbations"] >= 1 and info["restarts"] == 0 and info["breakdown"]
    assert lam.shape == (k,) and V.shape == (n, k)


def restart_case(device="cpu"):
    """A full-rank SPD preconditioner M = Z·Zᵀ + 1e-6·I (Z: three orthonormal columns) sends every residual block to nearly the
    same three directions: from the second iteration on W is within 1e-6 of the span of P, the Cholesky factor of the scaled SᵀS
    has a pivot below the floor of float32, and the iteration is redone without P.  W itself keeps full rank."""
    n, k = 200, 3
    Asp = operand("coupled", torch.float32, device=device)
    X = torch.from_numpy(lr.initial_block(n, k)).float().to(device)
    Z = torch.linalg.qr(torch.from_numpy(np.random.default_rng(1).standard_normal((n, k)))).Q
    M = (Z @ Z.t() + 1e-6 * torch.eye(n, dtype=torch.float64)).float().to(device)
    lam, V = sparse_lobpcg(Asp, k, X=X, preconditioner=M, largest=False, niter=30)
    return lam, V, dict(utils.last_solve_info("lobpcg")), M


def check_restart_case(lam, V, info, M):
    print(f"iterations {info['iterations']}, restarts {info['restarts']}, perturbations {info['perturbations']}")
    assert info["iterations"] > 0 and not info["breakdown"] and info["perturbations"] == 0
    assert info["restarts"] >= 1, "the Cholesky of SᵀS with P present never failed: the restart branch did not run"
    assert bool(torch.isfinite(lam).all()) and bool(torch.isfinite(V).all())
    # the pairs that come out of restarted iterations are Ritz pairs of an orthonormal block all the same
    _, _, _, _, D, spectrum = lr.case("coupled")
    Vd = V.double().cpu().numpy()
    assert lr.orthonormality(Vd) <= 1e-4
    ritz = np.linalg.eigvalsh(Vd.T @ D @ Vd)
    assert np.all(np.abs(ritz - lam.double().cpu().numpy()) <= 1e-3 * spectrum[-1])
    assert np.all(ritz >= spectrum[:3] - 1e-3) and np.all(ritz <= spectrum[-1])


def test_restart_without_p_inside_the_loop():
    lam, V, info, M = restart_case()
    check_restart_case(lam, V, info, M)
    # the numpy restatement restarts on the same input
    _, _, _, _, D, _ = lr.case("coupled")
    Mn = M.double().numpy()
    ref = lr.lobpcg(D, lr.initial_block(200, 3), largest=False, niter=30, dtype=np.float32, precondition=lambda R: Mn.astype(np.float32) @ R)[2]
    assert ref["restarts"] >= 1 and not ref["breakdown"] and ref["iterations"] > 0


@pytest.mark.parametrize("kind", ["lambda", "tensor", "fsai", "ic0", "ilu0"])
def test_preconditioners_are_applied(kind):
    Asp = operand("stencil27", torch.float64)
    _, _, _, k, D, spectrum = lr.case("stencil27")
    M = {"lambda": lambda: (lambda R: R / torch.from_numpy(np.diag(D).copy())[:, None]), "tensor": lambda: torch.from_numpy(np.linalg.inv(D)),
         "fsai": lambda: tsgu.sparse_fsai(Asp), "ic0": lambda: tsgu.sparse_ic0(Asp), "ilu0": lambda: tsgu.sparse_ilu0(Asp)}[kind]()
    X = torch.from_numpy(lr.initial_block(D.shape[0], k))
    lam, V = sparse_lobpcg(Asp, k, X=X, preconditioner=M, largest=False, niter=lr.NITER)
    info = dict(utils.last_solve_info("lobpcg"))
    print(kind, "iterations", info["iterations"], "against", solved("stencil27", "float64", False)[2]["iterations"], "without")
    check_pairs("stencil27", "float64", False, lam.numpy(), V.numpy(), info)


def test_refusals():
    Asp = operand("coupled", torch.float64)
    X = torch.from_numpy(lr.initial_block(200, 3))
    eye = torch.eye(120, dtype=torch.float64).to_sparse_csr()
    with pytest.raises(ValueError, match="square"):
        sparse_lobpcg(torch.sparse_csr_tensor(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.ones(2, dtype=torch.float64), (2, 3)), 1)
    with pytest.raises(ValueError, match="3k <= n.*k = 3 and n = 8"):
        sparse_lobpcg(torch.eye(8, dtype=torch.float64).to_sparse_csr(), 3)
    kmax = _backend.tall_geometry(torch.float64)[0]
    with pytest.raises(ValueError, match=f"at most {kmax} eigenpairs.*k = {kmax + 1}"):
        sparse_lobpcg(eye, kmax + 1)
    with pytest.raises(TypeError, match="float32 and float64"):
        sparse_lobpcg(torch.eye(16, dtype=torch.bfloat16).to_sparse_coo(), 1)
    with pytest.raises(ValueError, match="batched"):
        sparse_lobpcg(torch.stack([torch.eye(9, dtype=torch.float64)] * 2).to_sparse_coo(), 1)
    with pytest.raises(ValueError, match="BSR"):
        sparse_lobpcg(torch.eye(16, dtype=torch.float64).to_sparse_bsr((2, 2)), 1)
    with pytest.raises(ValueError, match="COO or CSR"):
        sparse_lobpcg(torch.eye(16, dtype=torch.float64), 1)
    with pytest.raises(ValueError, match=r"X must be a dense \(200, 3\)"):
        sparse_lobpcg(Asp, 3, X=X[:, :2])
    with pytest.raises(TypeError, match="X must have A's dtype"):
        sparse_lobpcg(Asp, 3, X=X.float())
    with pytest.raises(ValueError, match="device of A"):
        sparse_lobpcg(Asp, 3, X=torch.empty((200, 3), dtype=torch.float64, device="meta"))
    with pytest.raises(ValueError, match="preconditioner"):
        sparse_lobpcg(Asp, 3, X=X, preconditioner="jacobi")


# ---- the staged header ------------------------------------------------------------------------------------------------------------

ENTRIES = ("tsgu_tall_geometry", "tsgu_tall_gram", "tsgu_tall_combine", "tsgu_lobpcg_residual")


def test_the_staged_header_is_bound():
    assert _backend.STAGED == {"tsgu_hip_lobpcg.h": _backend.SIGNATURES_LOBPCG}
    assert not set(_backend.STAGED) & set(_backend.ABI) and not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_lobpcg.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_LOBPCG)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_LOBPCG[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7


def test_geometry():
    kmax, wmax, rows, nbytes = _backend.tall_geometry(torch.float32, 10 * 2048 + 1, 96, 96)
    assert (kmax, wmax, rows) == (32, 96, 2048) and nbytes == 11 * 96 * 96 * 4
    fold = 256
    assert _backend.tall_geometry(torch.float64, (fold + 1) * rows, 3, 5)[3] == (fold + 1 + 2) * 15 * 8
    lib = _backend.load_library()
    outs = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tsgu_tall_geometry(2, 8, 8, 8, *refs) == A.BAD_DTYPE and lib.tsgu_tall_geometry(7, 8, 8, 8, *refs) == A.BAD_DTYPE
    assert lib.tsgu_tall_geometry(0, 8, 97, 8, *refs) == A.TOO_LARGE and lib.tsgu_tall_geometry(0, -1, 8, 8, *refs) == A.BAD_ARG
    assert lib.tsgu_tall_geometry(0, 8, 8, 8, None, *refs[1:]) == A.BAD_ARG


# ---- host refusals: fake pointers that are never dereferenced, device = -1 (refused by set_device behind every other check) ----------

def _gram(**ch):
    a = dict(vtype=0, n=8, a=8, b=8, y=0x10000, ldy=8, z=0x20000, ldz=8, c=0x30000, ldc=8, workspace=0x40000, workspace_bytes=8 * 8 * 4,
             workgroups=0)
    a.update(ch)
    return _backend.load_library().tsgu_tall_gram(*a.values(), -1, None)


def _residual(**ch):
    a = dict(vtype=0, n=8, k=8, ax=0x10000, ldax=8, x=0x20000, ldx=8, lam=0x30000, r=0x40000, ldr=8, sumsq=0x50000, workspace=0x60000,
             workspace_bytes=8 * 4, workgroups=0)
    a.update(ch)
    return _backend.load_library().tsgu_lobpcg_residual(*a.values(), -1, None)


def _combine(vtype=0, n=8, s=(0x10000, 0x20000), s_width=(8, 8), s_ld=(8, 8), out=(0x30000,), out_width=(8,), out_ld=(8,), beta=(0.0,),
             coef=(0x40000, 0x50000), coef_ld=(8, 8), workgroups=0, n_in=None, n_out=None, null=()):
    ptrs = lambda xs: (ctypes.c_void_p * len(xs))(*xs)       # noqa: E731
    ints = lambda xs: (ctypes.c_int64 * len(xs))(*xs)        # noqa: E731
    host = dict(s=ptrs(s), s_width=ints(s_width), s_ld=ints(s_ld), out=ptrs(out), out_width=ints(out_width), out_ld=ints(out_ld),
                beta=(ctypes.c_double * len(beta))(*beta), coef=ptrs(coef), coef_ld=ints(coef_ld))
    h = {k: (None if k in null else ctypes.addressof(v)) for k, v in host.items()}
    return _backend.load_library().tsgu_tall_combine(vtype, n, len(s) if n_in is None else n_in, h["s"], h["s_width"], h["s_ld"],
                                                     len(out) if n_out is None else n_out, h["out"], h["out_width"], h["out_ld"], h["beta"],
                                                     h["coef"], h["coef_ld"], workgroups, -1, None)


def test_host_refusals_of_tall_gram():
    assert _gram() == A.BAD_ARG                                            # (the base call: refused by set_device only)
    assert [_gram(vtype=v) for v in (2, 7, -1)] == [A.BAD_DTYPE] * 3
    assert [_gram(n=v) for v in (-1, 0)] == [A.BAD_ARG] * 2
    assert [_gram(**{p: None}) for p in ("y", "z", "c", "workspace")] == [A.BAD_ARG] * 4
    for p, v in (("y", 0x10000), ("z", 0x20000), ("c", 0x30000), ("workspace", 0x40000)):
        assert _gram(**{p: v + 2}) == A.BAD_ARG and _gram(**{p: v + 4}, vtype=1, workspace_bytes=8 * 8 * 8) == A.BAD_ARG
    assert _gram(a=0) == A.BAD_ARG and _gram(b=0) == A.BAD_ARG
    assert _gram(a=97, ldy=97) == A.TOO_LARGE and _gram(b=97, ldz=97, ldc=97) == A.TOO_LARGE
    assert _gram(ldy=7) == A.BAD_ARG and _gram(ldz=7) == A.BAD_ARG and _gram(ldc=7) == A.BAD_ARG
    assert _gram(workspace_bytes=8 * 8 * 4 - 1) == A.BAD_ARG and _gram(workgroups=-1) == A.BAD_ARG
    # the order of the checks: the value type before everything, a width above the limit before the pointers
    assert _gram(vtype=7, n=0, y=None) == A.BAD_DTYPE and _gram(a=97, ldy=97, y=None) == A.TOO_LARGE
    # the workspace of a first fold level: one tile per chunk and one per group
    n = 257 * 2048
    assert _gram(n=n, a=1, b=1, workspace_bytes=(257 + 2) * 4 - 1) == A.BAD_ARG


def test_host_refusals_of_lobpcg_residual():
    assert _residual() == A.BAD_ARG
    assert [_residual(vtype=v) for v in (2, 7)] == [A.BAD_DTYPE] * 2
    assert [_residual(n=v) for v in (-1, 0)] == [A.BAD_ARG] * 2
    assert _residual(k=0) == A.BAD_ARG and _residual(k=33, ldax=33, ldx=33, ldr=33, workspace_bytes=33 * 4) == A.TOO_LARGE
    assert [_residual(**{p: 7}) for p in ("ldax", "ldx", "ldr")] == [A.BAD_ARG] * 3
    for p, v in (("ax", 0x10000), ("x", 0x20000), ("lam", 0x30000), ("r", 0x40000), ("sumsq", 0x50000), ("workspace", 0x60000)):
        assert _residual(**{p: None}) == A.BAD_ARG and _residual(**{p: v + 2}) == A.BAD_ARG
        assert _residual(**{p: v + 4}, vtype=1, workspace_bytes=8 * 8) == A.BAD_ARG
    assert _residual(workspace_bytes=8 * 4 - 1) == A.BAD_ARG
    assert _residual(r=0x10000) == A.BAD_ARG and _residual(r=0x20000 + 4 * 8) == A.BAD_ARG           # R on AX, R inside X
    assert _residual(vtype=7, k=33) == A.BAD_DTYPE


def test_host_refusals_of_tall_combine():
    assert _combine() == A.BAD_ARG
    assert [_combine(vtype=v) for v in (2, 7)] == [A.BAD_DTYPE] * 2
    assert [_combine(n=v) for v in (-1, 0)] == [A.BAD_ARG] * 2
    assert [_combine(n_in=v) for v in (0, 7)] == [A.BAD_ARG] * 2 and [_combine(n_out=v) for v in (0, 5)] == [A.BAD_ARG] * 2
    assert [_combine(null=(p,)) for p in ("s", "s_width", "s_ld", "out", "out_width", "out_ld", "coef", "coef_ld")] == [A.BAD_ARG] * 8
    assert _combine(s=(0, 0x20000)) == A.BAD_ARG and _combine(s=(0x10002, 0x20000)) == A.BAD_ARG
    assert _combine(out=(0,)) == A.BAD_ARG and _combine(out=(0x30002,)) == A.BAD_ARG and _combine(coef=(0x40002, 0)) == A.BAD_ARG
    assert _combine(vtype=1, s=(0x10004, 0x20000)) == A.BAD_ARG and _combine(vtype=1, out=(0x30004,)) == A.BAD_ARG
    assert _combine(s_width=(0, 8)) == A.BAD_ARG and _combine(out_width=(0,)) == A.BAD_ARG
    assert _combine(s_width=(33, 8), s_ld=(33, 8)) == A.TOO_LARGE and _combine(out_width=(33,), out_ld=(33,), coef_ld=(33, 33)) == A.TOO_LARGE
    assert _combine(s_ld=(7, 8)) == A.BAD_ARG and _combine(out_ld=(7,)) == A.BAD_ARG and _combine(coef_ld=(7, 8)) == A.BAD_ARG
    assert _combine(workgroups=-1) == A.BAD_ARG and _combine(vtype=7, n=0) == A.BAD_DTYPE
    # more than six distinct coefficient matrices
    six = dict(s=tuple(0x10000 + 0x1000 * i for i in range(6)), s_width=(8,) * 6, s_ld=(8,) * 6, out=(0x30000, 0x31000), out_width=(8, 8),
               out_ld=(8, 8), beta=(0.0, 0.0))
    assert _combine(**six, coef=tuple(0x40000 + 0x1000 * i for i in range(12)), coef_ld=(8,) * 12) == A.TOO_LARGE
    assert _combine(**six, coef=tuple(0x40000 + 0x1000 * (i % 6) for i in range(12)), coef_ld=(8,) * 12) == A.BAD_ARG      # (set_device)


def test_tall_combine_refuses_aliasing_on_the_host():
    """An output on an input, inside one, or on another output is refused.  Every call below carries a seventh distinct coefficient
    matrix, which the entry looks at AFTER the aliasing check (TSGU_ERR_TOO_LARGE): the interleaved blocks of one allocation reach
    it, an aliased output does not (TSGU_ERR_BAD_ARG)."""
    base = 0x100000
    blocks = lambda b: tuple(b + 4 * 8 * j for j in range(3))          # noqa: E731  (three 8-column blocks of a [n][24] fp32 allocation)
    seven = dict(coef=tuple(0x40000 + 0x1000 * i for i in range(7)) + (0,) * 5, coef_ld=(8,) * 12)
    ok = dict(s=blocks(base) + blocks(base + 0x10000), s_width=(8,) * 6, s_ld=(24,) * 6, out=(base + 0x20000, base + 0x20000 + 64),
              out_width=(8, 8), out_ld=(24, 24), beta=(0.0, 0.0))
    assert _combine(**ok, **seven) == A.TOO_LARGE                      # interleaved inputs and outputs pass the aliasing check
    for bad_out in ((base, base + 0x20000), (base + 0x20000, base + 0x20000), (base + 0x20000, base + 0x20000 + 16), (base + 96 * 3 + 32, base + 0x20000)):
        assert _combine(**dict(ok, out=bad_out), **seven) == A.BAD_ARG, [hex(x) for x in bad_out]
    assert _combine(**dict(ok, out_ld=(24, 25)), **seven) == A.BAD_ARG                # overlapping ranges with different strides
