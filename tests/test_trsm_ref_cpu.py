"""The reference of the triangular-solve geometry tests, checked on the CPU: the substitution agrees with a dense solve, an emulated
kernel of each precision stays inside the bound on every input tests/test_gpu_sptrsm_geometry.py uses, and a wrong solve breaks the
bound by orders of magnitude — so the bound can be met and has teeth."""

import numpy as np
import pytest

import _trsm_ref as R

EMULATED_COLUMNS = 16          # columns of a solve are independent and identically drawn: the emulation walks the first few


@pytest.mark.parametrize("n", [1, 2, 17, 64, 257])
@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("side", ["lower", "upper", "lower_T", "upper_T"])
def test_solve64_agrees_with_a_dense_solve(side, unit, n):
    ptr, idx, val = R.pattern(n, seed=3)
    if side.startswith("upper"):
        ptr, idx, val = R.to_upper(ptr, idx, val)
    lower = side.startswith("lower")
    if side.endswith("_T"):
        ptr, idx, val = R.transpose_csr(ptr, idx, val)
        lower = not lower
    D = R.dense(ptr, idx, val)
    assert np.array_equal(D, np.tril(D) if lower else np.triu(D))
    if unit:
        np.fill_diagonal(D, 1.0)          # (the stored diagonal is ignored)
    B = np.random.default_rng(5).standard_normal((n, 3))
    x = R.solve64(ptr, idx, val, B, lower, unit)
    want = np.linalg.solve(D, B)
    assert np.abs(x - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # the same without the stored diagonal (unit), and with the other triangle stored as well (ignored)
    if unit:
        assert np.array_equal(R.solve64(*R.strip_diagonal(ptr, idx, val), B, lower, True), x)
    full = R.dense(ptr, idx, val)
    full = full + (np.triu(np.ones((n, n)), 1) if lower else np.tril(np.ones((n, n)), -1))
    rr, cc = np.nonzero(full)
    fptr = np.zeros(n + 1, dtype=np.int64)
    fptr[1:] = np.cumsum(np.bincount(rr, minlength=n))
    assert np.array_equal(R.solve64(fptr, cc, full[rr, cc], B, lower, unit), x)


def test_patterns_are_what_the_kernel_geometry_needs():
    ptr, idx, val = R.pattern(R.N_WIDTHS, R.SEED)
    n = R.N_WIDTHS
    rows = np.repeat(np.arange(n), np.diff(ptr))
    assert (idx <= rows).all() and (idx[ptr[1:] - 1] == np.arange(n)).all()          # lower, diagonal last
    assert all((np.diff(idx[ptr[i]:ptr[i + 1]]) > 0).all() for i in range(n))         # sorted, no duplicates
    lens = np.diff(ptr) - 1
    assert set(R.LENS) <= set(lens.tolist())                                          # both sides of every EP, and rows of several rounds
    off = rows != idx
    dom = np.abs(val[~off]) / np.maximum(np.bincount(rows[off], np.abs(val[off]), minlength=n), 1e-300)
    assert dom.min() >= 2.0 and (val != 0).all()
    for dtype in R.DTYPES:          # rounding to the value type keeps the rows dominant and the entries non-zero
        v = R.round_to(val, dtype)
        assert (v != 0).all()
        assert (np.abs(v[~off]) / np.maximum(np.bincount(rows[off], np.abs(v[off]), minlength=n), 1e-300)).min() > 1.9
    # chains: every row that is no multiple of 3 (and has off-diagonal entries at all) waits for the row right before it
    assert all(i - 1 in idx[ptr[i]:ptr[i + 1]] for i in range(1, n) if i % 3 and lens[i])
    ap, ai, _ = R.arrow(65)
    assert ap[-1] - ap[-2] == 65 and (np.diff(ap)[:-1] == 1).all()
    cp, ci, _ = R.chain(5)
    assert ci.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    up, ui, uv = R.to_upper(ptr, idx, val)
    assert np.array_equal(R.dense(up, ui, uv), R.dense(ptr, idx, val)[::-1, ::-1])
    tp, ti, tv = R.transpose_csr(ptr, idx, val)
    assert np.array_equal(R.dense(tp, ti, tv), R.dense(ptr, idx, val).T)


def test_bf16_rounding_is_round_to_nearest_even():
    import torch

    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * 37.0
    x[:4] = [1.00390625, 1.01171875, 0.0, -1.00390625]          # ties: to even
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(R.bf16_round(x), want)


def _emulated_ratio(case, backward=False):
    ptr, idx, val = R.transpose_csr(*case.eff) if backward else case.eff
    lower = (not case.lower) if backward else case.lower
    x64, bnd = case.backward() if backward else case.forward()
    q = min(case.p, EMULATED_COLUMNS)
    rhs = (case.G if backward else case.B)[:, :q]
    x = R.emulate(ptr, idx, val, rhs, case.dtype, seed=11, lower=lower, unit=case.unit)
    return R.ratio(x, x64[:, :q], bnd[:, :q])


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_emulated_kernel_stays_inside_the_bound_on_the_width_cases(dtype, mode):
    """Test (a) of the GPU file: n = 1031, every dtype and mode, forward and the backward solve."""
    case = R.Case("pattern", R.N_WIDTHS, dtype, mode, EMULATED_COLUMNS)
    fwd, bwd = _emulated_ratio(case), _emulated_ratio(case, backward=True)
    print(f"emulated {dtype} {mode}: forward {fwd:.3f}, backward {bwd:.3f} of the bound")
    assert 0.0 < fwd <= 1.0 and 0.0 < bwd <= 1.0
    if dtype == "f32":
        assert R.rel_err(R.emulate(*case.eff, case.B, dtype, 11, case.lower, case.unit), case.forward()[0]) < R.NORMWISE["f32"]


@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_emulated_kernel_stays_inside_the_bound_on_the_row_count_cases(n):
    """Tests (b), (e) and (f) of the GPU file: every pattern and row count, fp32 (and bf16 where the GPU file uses it)."""
    worst = 0.0
    for kind in R.PATTERNS:
        if kind == "arrow" and n not in R.ARROW_ROWS:
            continue
        for mode in ("lower", "upper"):
            for dtype in ("f32", "bf16") if (kind, n) == ("pattern", 257) else ("f32",):
                r = _emulated_ratio(R.Case(kind, n, dtype, mode, EMULATED_COLUMNS))
                assert r <= 1.0, (kind, n, mode, dtype, r)
                worst = max(worst, r)
    print(f"n = {n}: emulated worst {worst:.3f} of the bound")


def test_emulated_kernel_stays_inside_the_bound_on_the_tuner_case():
    """Test (g) of the GPU file: the shallow pattern of 4096 rows, fp32."""
    ptr, idx, val = R.shallow(4096)
    val = R.round_to(val, "f32")
    assert (np.diff(ptr)[1:] == 2).all() and (idx[ptr[1:] - 1] == np.arange(4096)).all()
    B = R.round_to(np.random.default_rng(3).standard_normal((4096, 8)), "f32")
    x64 = R.solve64(ptr, idx, val, B, True, False)
    r = R.ratio(R.emulate(ptr, idx, val, B, "f32", seed=11), x64, R.bound(ptr, idx, val, x64, True, False, R.U["f32"]))
    print(f"shallow 4096: emulated {r:.3f} of the bound")
    assert 0.0 < r <= 1.0


@pytest.mark.parametrize("wrong,dtype", [("dropped_entry", "f32"), ("dropped_entry", "f64"), ("swapped_columns", "f32"),
                                         ("swapped_columns", "f64"), ("swapped_columns", "bf16")])
def test_a_wrong_solve_breaks_the_bound_by_orders_of_magnitude(wrong, dtype):
    """Measured: a dropped entry 1.3e3 (fp32) and 7e11 (fp64) of the bound, swapped columns 6.5e7, 3.5e16 and 2.5e3 (bf16).  bf16 is
    not asked for the dropped entry: one entry of a 130-entry row is 0.74 of a bound whose rows carry bf16's own 2^-7 — no bound of that
    precision sees it.  The kernel is one template for the three value types; the fp32 and fp64 cases and the bit identities of the
    GPU file are what would catch it."""
    case = R.Case("pattern", 257, dtype, "lower", 8)
    x64, bnd = case.forward()
    ptr, idx, val = case.eff
    if wrong == "dropped_entry":          # one off-diagonal entry of a long row is not accumulated
        i = int(np.argmax(np.diff(ptr)))
        k = ptr[i] + int(np.argmax(np.abs(val[ptr[i]:ptr[i + 1] - 1])))
        v = val.copy()
        v[k] = 0.0
        x = R.solve64(ptr, idx, v, case.B, True, False)
    else:          # two columns of X change places
        x = np.array(x64, dtype=np.float64)
        x[:, [2, 3]] = x[:, [3, 2]]
    r = R.ratio(x, x64, bnd)
    print(f"{wrong} {dtype}: {r:.3g} of the bound")
    assert r > 100.0


def test_bound_rows_scale_with_their_own_length():
    """γ is row-wise: a diagonal matrix is held to 5 u per element, not to the longest row of some other matrix."""
    case = R.Case("diag_only", 65, "f32", "lower", 4)
    x64, bnd = case.forward()
    assert np.allclose(bnd, 5 * R.U["f32"] * np.abs(x64), rtol=1e-12)
