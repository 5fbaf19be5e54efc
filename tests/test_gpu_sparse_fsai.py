"""sparse_fsai on the MI355X.

Backend level (tsgu_csr_fsai through `_backend.csr_fsai`), float32 and float64, int32 and int64.  The criterion is the residual of
every row, in float64 from the rounded inputs and the COMPUTED row ĝ:

    ‖A[J,J]·ĝ − e_m / ĝ_m‖₂  <=  (3m + 5)·m·u·‖A[J,J]‖₂·‖ĝ‖₂,      u = 2^-24 / 2^-53

the normwise backward-error bound of a Cholesky solve (Higham, Accuracy and Stability, Thm 10.4 with ‖|Rᵀ||R|‖₂ <= m·‖A‖₂) plus the
roundings of the scaling; it holds for any order of the sums.  A plain float32 Cholesky loop in numpy stays at or below 0.31 of
it on these patterns.  Beside it a sanity line against the float64 oracle (1e-4 / 1e-12 of the largest entry), and: one and eight
workgroups per CU, with and without the row order, give the same bits.

The patterns are the smallest on which each path of the kernel is taken: n = 1, 2; a diagonal with exact square roots; 1 025 rows of
two entries (eight rows per wave, several workgroups, a ragged last wave); truncated stencils with S = tril(A) and S = tril(A²) (S
holds positions A does not store); a random pattern with every size class and rows of different classes next to each other; dense
blocks up to the capacity that tsgu_csr_fsai_geometry reports; S = the diagonal alone (entries of A are skipped in the gather).

Public API: M(R) against Gᵀ·G·R in float64 from the computed G, FSAI-preconditioned CG with both patterns, MINRES and BiCGSTAB
with the same object, COO / unsorted input and check=False."""

import functools
import warnings

import numpy as np
import pytest
import torch

import _fsai_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {"f32": (torch.float32, np.float32, 2.0 ** -24), "f64": (torch.float64, np.float64, 2.0 ** -53)}
ITYPES = {"i32": torch.int32, "i64": torch.int64}
# case -> (pattern of A, power of the pattern whose lower triangle is S; 0: the diagonal alone)
CASES = ("n1", "n2", "chain1025", "stencil27", "stencil27_sq", "stencil7_sq", "random300", "random300_sq", "blocks", "stencil27_diag")


def _capacity(vn):
    from torchsparsegradutils_amd import _backend

    return _backend.fsai_geometry(DTYPES[vn][0])[0]


@functools.lru_cache(maxsize=None)
def _case(case, vn):
    """(lptr, lidx, lval rounded to the dtype, sptr, sidx, ptr, idx, val): tril(A), S and the whole of A."""
    power = 2 if case.endswith("_sq") else 0 if case.endswith("_diag") else 1
    base = case.split("_")[0]
    if base == "n1":
        ptr, idx = sr.band(1, 0)
    elif base == "n2":
        ptr, idx = sr.band(2, 1)
    elif base == "chain1025":
        ptr, idx = sr.band(1025, 1)
    elif base == "stencil27":
        ptr, idx = sr.stencil(6, 5, 4, 27)
    elif base == "stencil7":
        ptr, idx = sr.stencil(8, 8, 8, 7)
    elif base == "random300":
        ptr, idx = sr.random_pattern(300, 8, seed=11)
    elif base == "blocks":
        ptr, idx = sr.block_diagonal([max(64, _capacity(vn)), 5, 1, 33])
    else:
        raise KeyError(case)
    val = sr.dominant_values(ptr, idx, seed=len(idx), symmetric=True).astype(DTYPES[vn][1])
    lptr, lidx, lval, _ = sr.lower_csr(ptr, idx, val)
    sptr, sidx = sr.band(len(ptr) - 1, 0) if power == 0 else (lptr, lidx) if power == 1 else sr.power_lower_pattern(ptr, idx, power)
    return lptr, lidx, lval, sptr, sidx, ptr, idx, val


@functools.lru_cache(maxsize=None)
def _oracle(case, vn):
    lptr, lidx, lval, sptr, sidx = _case(case, vn)[:5]
    return sr.fsai(lptr, lidx, lval, sptr, sidx)


def _class_order(sptr):
    """The rows by size class (8 / 16 / 32 / 64 lanes), stable."""
    lens = np.diff(sptr)
    return np.argsort((lens > 8).astype(np.int64) + (lens > 16) + (lens > 32), kind="stable")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _run(lptr, lidx, lval, sptr, sidx, itype, wg=1, order=None):
    """(out as numpy, info as int) of one backend call."""
    from torchsparsegradutils_amd import _backend

    if sptr is lptr and sidx is lidx:                           # S = tril(A): the same arrays twice
        ap = sp = _dev(lptr, itype)
        ai = si = _dev(lidx, itype)
    else:
        ap, ai, sp, si = _dev(lptr, itype), _dev(lidx, itype), _dev(sptr, itype), _dev(sidx, itype)
    out, info = _backend.csr_fsai(ap, ai, _dev(lval), sp, si, len(sptr) - 1, order=None if order is None else _dev(order, itype), wg_per_cu=wg)
    assert out.is_cuda and info.is_cuda and info.dtype == torch.int64 and out.shape == (len(sidx),)
    return out.cpu().numpy(), int(info.item())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_every_row_solves_its_local_system(vn, it, case):
    dtype, npdt, u = DTYPES[vn]
    lptr, lidx, lval, sptr, sidx, ptr, idx, val = _case(case, vn)
    got, info = _run(lptr, lidx, lval, sptr, sidx, ITYPES[it])
    assert info == 0 and got.dtype == npdt and np.isfinite(got).all()
    res, bound, size = sr.row_residuals(lptr, lidx, lval, sptr, sidx, got, u)
    ratio = res / bound
    print(f"{case} {vn} {it}: m <= {size.max()}, worst row residual / bound = {ratio.max():.3f} (row {int(ratio.argmax())}, m = {size[ratio.argmax()]})")
    assert (res <= bound).all(), (case, int(ratio.argmax()), float(ratio.max()))
    g64, info64 = _oracle(case, vn)
    sanity = float(np.abs(got - g64).max() / np.abs(g64).max())
    print(f"{case} {vn} {it}: max|g - g64| / max|g64| = {sanity:.2e}")
    assert info64 == 0 and sanity < (1e-4 if vn == "f32" else 1e-12)
    # the grid and the order in which the rows are dealt change nothing
    order = _class_order(sptr)
    for wg, o in ((8, None), (1, order), (8, order), (1, order[::-1].copy())):
        again, info = _run(lptr, lidx, lval, sptr, sidx, ITYPES[it], wg=wg, order=o)
        assert info == 0 and _same_bits(again, got), (case, wg, o is not None)
    if case == "blocks":
        # the inverse Cholesky factor lies inside S: G·A·Gᵀ = I, to the bound above times the conditioning of the largest block
        m = int(size.max())
        A, G = sr.dense(ptr, idx, val.astype(np.float64)), sr.dense_lower(sptr, sidx, got)
        off = float(np.abs(G @ A @ G.T - np.eye(len(ptr) - 1)).max())
        allowed = (3 * m + 5) * m * u * float(np.linalg.cond(A[:m, :m]))
        print(f"blocks {vn} {it}: max|G·A·Gᵀ − I| = {off:.2e} (allowed {allowed:.2e})")
        assert m >= 64 and off <= allowed


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_exact_square_roots_give_exact_bits(vn, it):
    """band(37, 0) with powers of 4 on the diagonal: g_ii = 2^-k exactly."""
    npdt = DTYPES[vn][1]
    ptr, idx = sr.band(37, 0)
    k = (np.arange(37) % 9) - 4
    got, info = _run(ptr, idx, (4.0 ** k).astype(npdt), ptr, idx, ITYPES[it])
    assert info == 0 and _same_bits(got, (2.0 ** -k).astype(npdt))


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_breakdown_is_reported_and_touches_no_other_row(vn, it):
    """block_diagonal([40, 40, 40]) with a_41,41 = −1: info names row 41, the rows whose J does not contain 41 keep their bits."""
    npdt = DTYPES[vn][1]
    ptr, idx = sr.block_diagonal([40, 40, 40])
    val = sr.dominant_values(ptr, idx, seed=9, symmetric=True).astype(npdt)
    lptr, lidx, lval, _ = sr.lower_csr(ptr, idx, val)
    clean, info = _run(lptr, lidx, lval, lptr, lidx, ITYPES[it])
    assert info == 0
    rows = np.repeat(np.arange(120), np.diff(lptr))
    bad = lval.copy()
    bad[(rows == 41) & (lidx == 41)] = -1.0
    for wg in (1, 8):
        got, info = _run(lptr, lidx, bad, lptr, lidx, ITYPES[it], wg=wg)
        assert info == 42
        keep = (rows <= 40) | (rows >= 80)
        assert _same_bits(got[keep], clean[keep])
        assert not np.isfinite(got[rows == 41]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# public API


def _csr(ptr, idx, val, dtype, itype=torch.int32):
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(_dev(ptr, itype), _dev(idx, itype), _dev(val, dtype), (n, n))


@pytest.mark.parametrize("vn", DTYPES)
def test_the_preconditioner_applies_gt_g(vn):
    """M(R), M.solve(r), M.solve(R, transpose=True) and M.T(R) against Gᵀ·(G·R) in float64 from the COMPUTED G: normwise 1e-5
    (fp32; 1e-12 fp64), elementwise 8·ε·(|Gᵀ||G||R|)."""
    from torchsparsegradutils_amd import sparse_fsai

    dtype, npdt, _ = DTYPES[vn]
    eps = float(np.finfo(npdt).eps)
    ptr, idx, val = _case("stencil27", vn)[5:]
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype)
    M = sparse_fsai(A)
    assert int(M.info.item()) == 0 and M.values.dtype == dtype and M.values.is_cuda and M.shape == (n, n)
    G = M.G
    assert G.layout == torch.sparse_csr and G.is_cuda and G.col_indices().dtype == torch.int32
    Gd = G.to_dense()
    assert bool((torch.triu(Gd, 1) == 0).all()) and torch.equal(M.GT.to_dense(), Gd.T) and M.GT.layout == torch.sparse_csr
    assert M.T is M
    G64 = Gd.double().cpu().numpy()
    R = np.random.default_rng(0).standard_normal((n, 3)).astype(npdt)
    Rd = _dev(R)

    def check(got, r, what):
        r = r.astype(np.float64)
        want = G64.T @ (G64 @ r)
        mag = np.abs(G64.T) @ (np.abs(G64) @ np.abs(r))
        got = got.double().cpu().numpy()
        assert got.shape == want.shape
        norm = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        worst = float((np.abs(got - want) / (8 * eps * mag + 1e-300)).max())
        print(f"{what} {vn}: normwise {norm:.2e}, elementwise {worst:.3f} of the bound")
        assert norm < (1e-5 if vn == "f32" else 1e-12) and worst <= 1.0, (what, norm, worst)

    check(M(Rd), R, "M(R)")
    check(M.solve(Rd[:, 0].contiguous()), R[:, 0], "M.solve(r)")
    check(M.solve(Rd, transpose=True), R, "M.solve(R, transpose=True)")
    check(M.T(Rd), R, "M.T(R)")
    check(M.matmul(Rd), R, "M.matmul(R)")
    assert M(Rd).dtype == dtype and not M(Rd.requires_grad_(True)).requires_grad


def _anisotropic(nx, ny, nz, c):
    """7-point operator −∇·(diag(c)∇) with Dirichlet faces: SPD."""
    ptr, idx = sr.stencil(nx, ny, nz, 7)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    d = np.abs(idx - rows)
    return ptr, idx, np.where(d == 0, 2.0 * sum(c), np.where(d == 1, -c[2], np.where(d == nz, -c[1], -c[0])))


@pytest.mark.parametrize("vn", DTYPES)
def test_fsai_preconditioned_cg_takes_fewer_iterations(vn):
    """Coefficients 1 : 10 : 100 on 12³.  A numpy CG takes 56 / 29 / 20 iterations (plain / tril(A) / tril(A²)) in float64 at 1e-6
    and 37 / 20 / 14 in float32 at 1e-4; only the ordering is asserted."""
    from torchsparsegradutils_amd import sparse_fsai, sparse_spgemm
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    dtype, npdt, _ = DTYPES[vn]
    tol = 1e-6 if vn == "f64" else 1e-4
    ptr, idx, val = _anisotropic(12, 12, 12, (1.0, 10.0, 100.0))
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype)
    b = np.random.default_rng(0).standard_normal((n, 2)).astype(npdt)
    x64 = np.linalg.solve(sr.dense(ptr, idx, val), b.astype(np.float64))
    its = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, pre in (("plain", None), ("fsai(A)", sparse_fsai(A)), ("fsai(A²)", sparse_fsai(A, pattern=sparse_spgemm(A, A)))):
            x = linear_cg(A, _dev(b), tolerance=tol, eps=1e-20, stop_updating_after=1e-20, max_iter=500, max_tridiag_iter=0, preconditioner=pre)
            info = last_solve_info("linear_cg")
            its[name] = info["iterations"]
            err = float(np.linalg.norm(x.double().cpu().numpy() - x64) / np.linalg.norm(x64))
            print(f"{vn} {name}: {info['iterations']} iterations, relative error {err:.2e}")
            # a residual of `tol` relative to |b| is an error of at most cond(A)·tol relative to |x|; cond(A) < 200 here
            assert info["tolerance_reached"] and err < 200 * tol, (name, info, err)
    assert its["fsai(A²)"] < its["fsai(A)"] < its["plain"], its


@pytest.mark.parametrize("vn", DTYPES)
def test_minres_and_bicgstab_take_the_same_object(vn):
    from torchsparsegradutils_amd import sparse_fsai
    from torchsparsegradutils_amd.utils import BICGSTABSettings, MINRESSettings, bicgstab, minres

    dtype, npdt, _ = DTYPES[vn]
    tol = 1e-6 if vn == "f64" else 1e-4
    ptr, idx, val = _anisotropic(12, 12, 12, (1.0, 10.0, 100.0))
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype)
    M = sparse_fsai(A)
    b = np.random.default_rng(1).standard_normal((n, 2)).astype(npdt)
    x64 = np.linalg.solve(sr.dense(ptr, idx, val), b.astype(np.float64))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xm = minres(A, _dev(b), preconditioner=M, settings=MINRESSettings(max_cg_iterations=500, minres_tolerance=tol))
        xb = bicgstab(A, _dev(b), settings=BICGSTABSettings(reltol=tol, abstol=0.0, precon=M))
    for name, x in (("minres", xm), ("bicgstab", xb)):
        err = float(np.linalg.norm(x.double().cpu().numpy() - x64) / np.linalg.norm(x64))
        print(f"{vn} {name}: relative error {err:.2e}")
        assert err < 200 * tol, (name, err)


def test_coo_unsorted_and_check_false():
    from torchsparsegradutils_amd import sparse_fsai

    lptr, lidx, lval, _, _, ptr, idx, val = _case("random300", "f64")
    A = _csr(ptr, idx, val, torch.float64)
    want = sparse_fsai(A).values
    assert torch.equal(sparse_fsai(A.to_sparse_coo()).values, want)
    # the same matrix with every row's columns reversed
    n = len(ptr) - 1
    rev = np.concatenate([np.arange(ptr[i], ptr[i + 1])[::-1] for i in range(n)])
    M = sparse_fsai(_csr(ptr, idx[rev], val[rev], torch.float64))
    assert torch.equal(M.values, want) and torch.equal(M.col_indices.cpu(), torch.from_numpy(lidx).to(torch.int32))
    rows = np.repeat(np.arange(n), np.diff(ptr))
    bad = val.copy()
    bad[(rows == 0) & (idx == 0)] = -1.0
    with pytest.raises(RuntimeError, match="sparse_fsai: local matrix not positive definite in row 0"):
        sparse_fsai(_csr(ptr, idx, bad, torch.float64))
    M = sparse_fsai(_csr(ptr, idx, bad, torch.float64), check=False)
    assert M.info.is_cuda and int(M.info.item()) == 1
