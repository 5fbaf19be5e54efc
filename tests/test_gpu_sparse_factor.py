"""sparse_ilu0 / sparse_ic0 on the MI355X.

Backend level (tsgu_csr_ilu0 / tsgu_csr_ic0 through `_backend.csr_factor`), float32 and float64, int32 and int64:

  * ILU(0) bit for bit against the sequential IKJ loop of tests/_factor_ref.py in the SAME dtype — one division, multiplication
    and subtraction per update, every entry updated in ascending k, so there is nothing for a launch geometry to change;
  * both factors: for every stored (i, k), |Σ_j f_ij·g_jk − a_ik| <= (m_ik + 2)·u·Σ_j |f_ij·g_jk| with the sums formed from the
    COMPUTED factor (extended precision), m_ik the number of terms, u = 2^-24 / 2^-53: the componentwise backward-error bound of
    LU / Cholesky restricted to the pattern (each a_ik is reproduced by m_ik products, at most m_ik subtractions and one division
    or square root, whatever the order of the sum);
  * IC(0) bit for bit where every order of every sum is exact: A = L0·L0ᵀ with small integers off and powers of two on the
    diagonal of L0, on patterns without fill;
  * two runs and one / eight workgroups per CU give the same bits; a breakdown in the middle of the matrix is reported, does not
    stop the rows that do not depend on it, and leaves the error word of the bounded waits clear.

The patterns are the smallest on which each path of the kernel is taken: n = 1, 2; no dependencies at all (diagonal); a chain of
1 025 rows in which every row waits for the one before (the tickets wrap every class); a band of 2 048 rows (all 64 workgroup
classes draw rows); truncated stencils and a random pattern (fill is dropped); an arrow whose last rows are longer than the LDS
slice (sized from tsgu_csr_factor_geometry) and in which one early row has more than 64 upper entries.

Public API: M(R) and M.T against two substitutions in float64, IC(0)-preconditioned CG, ILU(0)-preconditioned BiCGSTAB inside
sparse_generic_solve with both gradients, and SparseMultivariateNormal(precision_tril = sparse_ic0(P).L)."""

import functools
import warnings

import numpy as np
import pytest
import torch

import _factor_ref as fr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = {"f32": (torch.float32, np.float32, 2.0 ** -24), "f64": (torch.float64, np.float64, 2.0 ** -53)}
ITYPES = {"i32": torch.int32, "i64": torch.int64}
CASES = ("n1", "n2", "diagonal", "chain1025", "band2048", "stencil27", "stencil7", "random300", "arrow")


def _capacity(vn):
    from torchsparsegradutils_amd import _backend

    return _backend.factor_geometry(DTYPES[vn][0])[0]


@functools.lru_cache(maxsize=None)
def _pattern(case, vn):
    if case == "n1":
        return fr.band(1, 0)
    if case == "n2":
        return fr.band(2, 1)
    if case == "diagonal":
        return fr.band(37, 0)
    if case == "chain1025":
        return fr.band(1025, 1)
    if case == "band2048":
        return fr.band(2048, 3)
    if case == "stencil27":
        return fr.stencil(6, 5, 4, 27)
    if case == "stencil7":
        return fr.stencil(8, 8, 8, 7)
    if case == "random300":
        return fr.random_pattern(300, 8, seed=11)
    if case == "arrow":
        # the last three rows are full: row_capacity + 3 entries (in tril(A): the last row); row 2 has 70 upper entries
        return fr.arrow(_capacity(vn) + 3, tail=3, early=2, early_len=70)
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def _matrix(case, vn, spd):
    """(ptr, idx, values rounded to the dtype (as that dtype)) — diagonally dominant, symmetric positive definite when `spd`."""
    ptr, idx = _pattern(case, vn)
    val = fr.dominant_values(ptr, idx, seed=len(idx) + 7 * spd, symmetric=spd)
    return ptr, idx, val.astype(DTYPES[vn][1])


@functools.lru_cache(maxsize=None)
def _ilu_oracle(case, vn):
    ptr, idx, val = _matrix(case, vn, False)
    return fr.ilu0(ptr, idx, val, dtype=DTYPES[vn][1])


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _run(kind, ptr, idx, val, itype, wg=1, shift=0.0, in_place=False):
    """(out as numpy, info as int) of one backend call."""
    from torchsparsegradutils_amd import _backend

    dpos = fr.diag_positions(ptr, idx)
    v = _dev(val)
    out, info = _backend.csr_factor(kind, _dev(ptr, itype), _dev(idx, itype), _dev(dpos, itype), v, len(ptr) - 1, shift=shift, wg_per_cu=wg,
                                    out=v if in_place else None)
    _backend.poll_errors(block=True)
    return out.cpu().numpy(), int(info.item())


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


def _assert_bound(ptr, idx, F, G, A, u, what):
    err, bound = fr.pattern_residual_bound(ptr, idx, F, G, A, u)
    worst = float((err / (bound + 1e-300)).max())
    print(f"{what}: worst |F·G − A| / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: an entry is {worst:.2f} x its bound (m + 2)·u·Σ|terms|"


# ---------------------------------------------------------------------------------------------------------------------------
# backend level


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_ilu0_is_the_sequential_loop_bit_for_bit(vn, it, case):
    _, npdt, u = DTYPES[vn]
    ptr, idx, val = _matrix(case, vn, False)
    want, want_info = _ilu_oracle(case, vn)
    assert want_info == 0
    got, info = _run("ilu0", ptr, idx, val, ITYPES[it])
    assert info == 0
    assert got.dtype == npdt and _same_bits(got, want), f"{int((got != want).sum())} of {got.size} entries differ from the sequential loop"
    again, _ = _run("ilu0", ptr, idx, val, ITYPES[it])
    wide, _ = _run("ilu0", ptr, idx, val, ITYPES[it], wg=8)
    assert _same_bits(again, got) and _same_bits(wide, got)
    L, U = fr.split_lu(ptr, idx, got)
    _assert_bound(ptr, idx, L, U, fr.dense(ptr, idx, val.astype(np.float64)), u, f"ilu0 {case} {vn}")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_ic0_reproduces_the_matrix_on_the_pattern(vn, it, case):
    _, npdt, u = DTYPES[vn]
    ptr, idx, val = _matrix(case, vn, True)
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, val)
    got, info = _run("ic0", lptr, lidx, lval, ITYPES[it])
    assert info == 0 and got.dtype == npdt
    again, _ = _run("ic0", lptr, lidx, lval, ITYPES[it])
    wide, _ = _run("ic0", lptr, lidx, lval, ITYPES[it], wg=8)
    assert _same_bits(again, got) and _same_bits(wide, got)
    L = fr.dense(lptr, lidx, got.astype(np.float64))
    _assert_bound(lptr, lidx, L, L.T, fr.dense(ptr, idx, val.astype(np.float64)), u, f"ic0 {case} {vn}")
    # and the float64 oracle, at the distance the two bounds allow: both factors reproduce A on the pattern, so they differ by
    # rounding amplified by the conditioning of these diagonally dominant matrices — a loose sanity line, not the criterion
    want, _ = fr.ic0(lptr, lidx, lval.astype(np.float64))
    assert float(np.abs(got - want).max() / np.abs(want).max()) < (1e-4 if vn == "f32" else 1e-12)


@pytest.mark.parametrize("pattern", ["tridiagonal", "blocks", "downward_arrow"])
@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_ic0_is_exact_on_integer_data_without_fill(vn, it, pattern):
    npdt = DTYPES[vn][1]
    ptr, idx = {"tridiagonal": lambda: fr.band(1025, 1), "blocks": lambda: fr.block_diagonal([5, 1, 70, 9, 33]),
                "downward_arrow": lambda: fr.downward_arrow(300)}[pattern]()
    lptr, lidx, a, l0 = fr.integer_cholesky_case(ptr, idx, seed=5)
    assert float(np.abs(a).max()) < 2 ** 20
    got, info = _run("ic0", lptr, lidx, a.astype(npdt), ITYPES[it])
    assert info == 0 and _same_bits(got, l0.astype(npdt))


@pytest.mark.parametrize("vn", DTYPES)
def test_in_place_and_shift(vn):
    """out == val is allowed; `shift` multiplies the diagonal by (1 + shift) before anything else (the oracle's first step)."""
    npdt = DTYPES[vn][1]
    ptr, idx, val = _matrix("stencil27", vn, False)
    want, _ = _ilu_oracle("stencil27", vn)
    got, info = _run("ilu0", ptr, idx, val, torch.int32, in_place=True)
    assert info == 0 and _same_bits(got, want)
    shifted, _ = fr.ilu0(ptr, idx, val, dtype=npdt, shift=0.25)
    got, _ = _run("ilu0", ptr, idx, val, torch.int32, shift=0.25)
    assert _same_bits(got, shifted) and not _same_bits(got, want)
    ptr, idx, val = _matrix("stencil27", vn, True)
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, val)
    plain, _ = _run("ic0", lptr, lidx, lval, torch.int32)
    got, info = _run("ic0", lptr, lidx, lval, torch.int32, in_place=True)
    assert info == 0 and _same_bits(got, plain)
    rows = np.repeat(np.arange(len(lptr) - 1), np.diff(lptr))
    scaled = np.where(lidx == rows, lval * npdt(1.25), lval).astype(npdt)          # (1.25 is exact: the same rounding as the kernel's)
    want, _ = _run("ic0", lptr, lidx, scaled, torch.int32)
    got, _ = _run("ic0", lptr, lidx, lval, torch.int32, shift=0.25)
    assert _same_bits(got, want) and not _same_bits(got, plain)


@pytest.mark.parametrize("it", ITYPES)
@pytest.mark.parametrize("vn", DTYPES)
def test_breakdown_in_the_middle_is_reported_and_stops_nothing(vn, it):
    """Three dense diagonal blocks of 40 rows; the second row of the middle block breaks down.  ILU: its pivot cancels exactly
    (a_11 = fl(fl(a_10 / a_00)·a_01)); IC: a negative diagonal.  The first and the last block do not depend on it: they equal the
    oracle bit for bit (ILU) / the undisturbed run (IC); the call returns and the error word of the waits stays clear (`_run`
    polls it)."""
    npdt = DTYPES[vn][1]
    ptr, idx = fr.block_diagonal([40, 40, 40])
    rows = np.repeat(np.arange(120), np.diff(ptr))
    bad = 41
    at = lambda i, j: int(ptr[i] + np.nonzero(idx[ptr[i]:ptr[i + 1]] == j)[0][0])  # noqa: E731
    outside = (rows < 40) | (rows >= 80)

    val = fr.dominant_values(ptr, idx, seed=3).astype(npdt)
    val[at(41, 41)] = npdt(npdt(val[at(41, 40)] / val[at(40, 40)]) * val[at(40, 41)])
    want, want_info = fr.ilu0(ptr, idx, val, dtype=npdt)
    assert want_info == bad + 1 and want[at(41, 41)] == 0
    got, info = _run("ilu0", ptr, idx, val, ITYPES[it])
    assert info == bad + 1
    assert _same_bits(got[outside], want[outside]) and _same_bits(got[rows <= bad], want[rows <= bad])
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    assert not np.isfinite(got[rows == 79]).all()                                # (the rows behind it carry inf / NaN on)

    sym = fr.dominant_values(ptr, idx, seed=4, symmetric=True).astype(npdt)
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, sym)
    lrows = np.repeat(np.arange(120), np.diff(lptr))
    clean, clean_info = _run("ic0", lptr, lidx, lval, ITYPES[it])
    assert clean_info == 0
    lval = lval.copy()
    lval[lptr[bad + 1] - 1] = -1.0
    got, info = _run("ic0", lptr, lidx, lval, ITYPES[it])
    assert info == bad + 1
    keep = (lrows < bad) | (lrows >= 80)
    assert _same_bits(got[keep], clean[keep])
    assert np.isnan(got[lptr[bad + 1] - 1]) and np.isnan(got[lrows == 79]).any()
    _, ref_info = fr.ic0(lptr, lidx, lval, dtype=npdt)
    assert ref_info == info


# ---------------------------------------------------------------------------------------------------------------------------
# public API


def _csr(ptr, idx, val, dtype, itype=torch.int32):
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(_dev(ptr, itype), _dev(idx, itype), _dev(val, dtype), (n, n))


def _comparison_solve(T, rhs):
    """M(T)⁻¹·rhs, M(T) the comparison matrix of the triangular T (Higham, Accuracy and Stability, Thm 8.5)."""
    M = -np.abs(T)
    np.fill_diagonal(M, np.abs(np.diag(T)))
    return np.linalg.solve(M, rhs)


@pytest.mark.parametrize("kind", ["ilu0", "ic0"])
@pytest.mark.parametrize("vn", DTYPES)
def test_the_factor_applies_its_inverse(vn, kind):
    """M(R), M.solve(R, transpose=True) and M.T(R) for R of both ranks against two substitutions in float64 with the COMPUTED
    factor.  Normwise 1e-5 (fp32; 1e-12 fp64) and elementwise 8·ε·Σ|terms|, the terms of x = F2⁻¹(F1⁻¹ r) being those of the
    two substitutions: M(F2)⁻¹·(|F2|·|x| + M(F1)⁻¹·|F1|·|y|), y = F1⁻¹ r (the first sweep's error reaches x through |F2⁻¹| <=
    M(F2)⁻¹)."""
    from torchsparsegradutils_amd import sparse_ic0, sparse_ilu0

    dtype, npdt, _ = DTYPES[vn]
    eps = float(np.finfo(npdt).eps)
    ptr, idx, val = _matrix("stencil27", vn, kind == "ic0")
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype)
    M = (sparse_ic0 if kind == "ic0" else sparse_ilu0)(A)
    assert int(M.info.item()) == 0 and M.values.dtype == dtype and M.values.is_cuda
    if kind == "ic0":
        lptr, lidx, _, _ = fr.lower_csr(ptr, idx)
        F1 = fr.dense(lptr, lidx, M.values.double().cpu().numpy())
        F2 = F1.T.copy()
        assert M.T is M
    else:
        F1, F2 = fr.split_lu(ptr, idx, M.values.cpu().numpy())
        assert torch.equal(M.crow_indices, A.crow_indices()) and M.col_indices.data_ptr() == A.col_indices().data_ptr()
    R = np.random.default_rng(0).standard_normal((n, 3)).astype(npdt)

    def check(got, first, second, r, what):
        r = r.astype(np.float64)
        y = np.linalg.solve(first, r)
        x = np.linalg.solve(second, y)
        mag = _comparison_solve(second, np.abs(second) @ np.abs(x) + _comparison_solve(first, np.abs(first) @ np.abs(y)))
        got = got.double().cpu().numpy()
        assert got.shape == x.shape
        norm = float(np.linalg.norm(got - x) / np.linalg.norm(x))
        worst = float((np.abs(got - x) / (8 * eps * mag + 1e-300)).max())
        print(f"{what} {vn}: normwise {norm:.2e}, elementwise {worst:.3f} of the bound")
        assert norm < (1e-5 if vn == "f32" else 1e-12) and worst <= 1.0, (what, norm, worst)

    Rd = _dev(R)
    check(M(Rd), F1, F2, R, "M(R)")
    check(M.solve(Rd[:, 0].contiguous()), F1, F2, R[:, 0], "M(r)")
    check(M.solve(Rd, transpose=True), F2.T, F1.T, R, "M.solve(R, transpose=True)")
    check(M.T(Rd), F2.T, F1.T, R, "M.T(R)")
    check(M.T.T(Rd[:, 1].contiguous()), F1, F2, R[:, 1], "M.T.T(r)")
    assert M(Rd).dtype == dtype and not M(Rd).requires_grad


def _anisotropic(nx, ny, nz, c):
    """7-point operator −∇·(diag(c)∇) with Dirichlet faces: SPD."""
    ptr, idx = fr.stencil(nx, ny, nz, 7)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    d = np.abs(idx - rows)
    return ptr, idx, np.where(d == 0, 2.0 * sum(c), np.where(d == 1, -c[2], np.where(d == nz, -c[1], -c[0])))


@pytest.mark.parametrize("vn", DTYPES)
def test_ic0_preconditioned_cg_takes_fewer_iterations(vn):
    """Coefficients 1 : 10 : 100 on 12³: on CPU operands plain CG takes 56 iterations to a mean residual of 1e-6, IC(0)-PCG 13."""
    from torchsparsegradutils_amd import sparse_ic0
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    dtype, npdt, _ = DTYPES[vn]
    tol = 1e-6 if vn == "f64" else 1e-4
    ptr, idx, val = _anisotropic(12, 12, 12, (1.0, 10.0, 100.0))
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype)
    b = np.random.default_rng(0).standard_normal((n, 2)).astype(npdt)
    x64 = np.linalg.solve(fr.dense(ptr, idx, val), b.astype(np.float64))
    M = sparse_ic0(A)
    its = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, pre in (("plain", None), ("ic0", M)):
            x = linear_cg(A, _dev(b), tolerance=tol, eps=1e-20, stop_updating_after=1e-20, max_iter=500, max_tridiag_iter=0, preconditioner=pre)
            info = last_solve_info("linear_cg")
            its[name] = info["iterations"]
            err = float(np.linalg.norm(x.double().cpu().numpy() - x64) / np.linalg.norm(x64))
            print(f"{vn} {name}: {info['iterations']} iterations, relative error {err:.2e}")
            # a residual of `tol` relative to |b| is an error of at most cond(A)·tol relative to |x|; cond(A) < 200 here
            assert info["tolerance_reached"] and err < 200 * tol, (name, info, err)
    assert its["ic0"] < its["plain"], its


@pytest.mark.parametrize("vn", DTYPES)
def test_ilu0_preconditioned_bicgstab_inside_sparse_generic_solve(vn):
    from torchsparsegradutils_amd import sparse_generic_solve, sparse_ilu0
    from torchsparsegradutils_amd.utils import BICGSTABSettings, bicgstab

    dtype, npdt, _ = DTYPES[vn]
    rtol = 1e-12 if vn == "f64" else 1e-6
    ptr, idx, val = _matrix("stencil27", vn, False)
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    A = _csr(ptr, idx, val, dtype).requires_grad_(True)
    rng = np.random.default_rng(1)
    Bn, Gn = rng.standard_normal((n, 2)).astype(npdt), rng.standard_normal((n, 2)).astype(npdt)
    B = _dev(Bn).requires_grad_(True)
    M = sparse_ilu0(A)
    assert not M.values.requires_grad

    def settings(P):
        return BICGSTABSettings(reltol=rtol, abstol=0.0, precon=P)

    def solve(a, b, **kw):
        return bicgstab(a, b, settings=settings(M))

    def transpose_solve(a, b, **kw):
        return bicgstab(a.to_dense().t().to_sparse_csr(), b, settings=settings(M.T))

    X = sparse_generic_solve(A, B, solve=solve, transpose_solve=transpose_solve)
    X.backward(_dev(Gn))
    Ad = torch.from_numpy(fr.dense(ptr, idx, val.astype(np.float64))).requires_grad_(True)
    Bd = torch.from_numpy(Bn.astype(np.float64)).requires_grad_(True)
    Xd = torch.linalg.solve(Ad, Bd)
    Xd.backward(torch.from_numpy(Gn.astype(np.float64)))
    tol = 1e-9 if vn == "f64" else 2e-4       # (the solver's relative residual times the conditioning of a dominant stencil)

    def rel(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    assert rel(X.detach().double().cpu().numpy(), Xd.detach().numpy()) < tol
    assert rel(B.grad.double().cpu().numpy(), Bd.grad.numpy()) < tol
    assert rel(A.grad.values().double().cpu().numpy(), Ad.grad.numpy()[rows, idx]) < tol


def test_ic0_factor_as_precision_tril():
    from torchsparsegradutils_amd import sparse_ic0
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormal

    ptr, idx = fr.band(33, 1)
    val = fr.dominant_values(ptr, idx, seed=5, symmetric=True)
    P = _csr(ptr, idx, val, torch.float64)
    L = sparse_ic0(P).L
    assert L.layout == torch.sparse_csr and L.is_cuda
    loc = torch.zeros(33, dtype=torch.float64, device=DEV)
    xs = _dev(np.random.default_rng(7).standard_normal((4, 33)))
    got = SparseMultivariateNormal(loc, precision_tril=L).log_prob(xs)
    want = torch.distributions.MultivariateNormal(loc.cpu(), precision_matrix=torch.from_numpy(fr.dense(ptr, idx, val))).log_prob(xs.cpu())
    assert float((got.cpu() - want).abs().max()) < 1e-10 * float(want.abs().max())


def test_coo_unsorted_and_check_false():
    from torchsparsegradutils_amd import sparse_ilu0

    ptr, idx, val = _matrix("random300", "f64", False)
    A = _csr(ptr, idx, val, torch.float64)
    want = sparse_ilu0(A).values
    assert torch.equal(sparse_ilu0(A.to_sparse_coo()).values, want)
    # the same matrix with every row's columns reversed
    n = len(ptr) - 1
    rev = np.concatenate([np.arange(ptr[i], ptr[i + 1])[::-1] for i in range(n)])
    M = sparse_ilu0(_csr(ptr, idx[rev], val[rev], torch.float64))
    assert torch.equal(M.values, want) and torch.equal(M.col_indices.cpu(), torch.from_numpy(idx).to(torch.int32))
    zero = val.copy()
    zero[fr.diag_positions(ptr, idx)[0]] = 0.0
    with pytest.raises(RuntimeError, match="zero pivot in row 0"):
        sparse_ilu0(_csr(ptr, idx, zero, torch.float64))
    M = sparse_ilu0(_csr(ptr, idx, zero, torch.float64), check=False)
    assert M.info.is_cuda and int(M.info.item()) == 1
