"""Plain numpy reference for the sync-free triangular solve (csrc/sptrsm.hip): patterns, a float64 substitution, the
componentwise bound every correct solve of a given precision stays within, and an emulation of "any correct kernel of that precision"
that shows the bound is reachable on exactly the inputs the GPU tests use.  No GPU, no oracle binary.

The constants are derived here, not read off the kernel:

* fp32 / fp64: unit roundoff u = 2^-24 / 2^-53.  A row of `len` stored entries is `len - 1` products and additions in some order,
  one subtraction from the right-hand side and one division: (len + 4)·u per row covers it (Higham, Accuracy and Stability,
  Thm 8.5, with the comparison matrix M(T) in place of T so that the bound holds for ANY order of the row's sum).
* bf16: bf16 elements, fp32 arithmetic (u = 2^-24), and x rounded to bf16 ONCE per row, when it is handed to the rows that depend on
  it.  That rounding is a relative 2^-8 of x_i; it enters the row-wise bound as `extra`.  The bound is first order (it drops the
  (M − γ|T|)^-1 term), which is negligible at 2^-24 and not at 2^-8: `extra` is doubled to 2^-7.
"""

from __future__ import annotations

import numpy as np

LENS = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]   # row lengths on both sides of every EP = 64 / CL

U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "bf16": 2.0 ** -24}
EXTRA = {"f32": 0.0, "f64": 0.0, "bf16": 2.0 ** -7}
NORMWISE = {"f32": 1e-5, "f64": 1e-10}          # the project's existing normwise bars

# ---- what the GPU tests run (shared with tests/test_trsm_ref_cpu.py, which shows the emulation inside the bound on each) ----------
MODES = ("lower", "upper", "lower_T", "lower_unit")
DTYPES = ("f32", "f64", "bf16")
WIDTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 200]
N_WIDTHS = 1031
BACKWARD_WIDTHS = (1, 17, 65)
ROW_COUNTS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1031]
ROW_WIDTHS = (1, 8, 65)
ARROW_ROWS = (65, 257, 1031)
SEED = 7


# ---- patterns ------------------------------------------------------------------------------------------------------------------
def _csr(rows_idx, rows_val):
    ptr = np.zeros(len(rows_idx) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows_idx])
    idx = np.concatenate(rows_idx).astype(np.int64) if len(rows_idx) else np.zeros(0, np.int64)
    val = np.concatenate(rows_val).astype(np.float64) if len(rows_val) else np.zeros(0)
    return ptr, idx, val


def _diag(rng):
    return rng.uniform(1.0, 2.0) * (1.0 if rng.random() < 0.5 else -1.0)


def _offdiag(rng, k):
    """k values in (−1, 1) rescaled to an absolute sum in [0.25, 0.5]: with a diagonal in [1, 2] the row is dominant by >= 2."""
    v = rng.uniform(-1.0, 1.0, k)
    return v * (rng.uniform(0.25, 0.5) / np.abs(v).sum())


def pattern(n, seed, band=200):
    """Lower-triangular CSR (ptr, idx, val), float64, sorted columns, diagonal last.  Row i has min(LENS[i % 17], i, band) off-diagonal
    entries among the previous `band` rows; column i − 1 is forced in whenever i % 3 != 0 (deep chains)."""
    rng = np.random.default_rng(seed)
    ri, rv = [], []
    for i in range(n):
        k = min(LENS[i % len(LENS)], i, band)
        lo = max(0, i - band)
        if k == 0:
            cols = np.zeros(0, np.int64)
        elif i % 3 != 0:
            cols = np.append(rng.choice(np.arange(lo, i - 1), k - 1, replace=False), i - 1)
        else:
            cols = rng.choice(np.arange(lo, i), k, replace=False)
        cols = np.sort(cols)
        ri.append(np.append(cols, i))
        rv.append(np.append(_offdiag(rng, k) if k else np.zeros(0), _diag(rng)))
    return _csr(ri, rv)


def chain(n, seed=0):
    """Bidiagonal: every row waits for the one before it (depth n)."""
    rng = np.random.default_rng(seed)
    ri = [np.array([i - 1, i] if i else [0]) for i in range(n)]
    rv = [np.append(_offdiag(rng, 1) if i else np.zeros(0), _diag(rng)) for i in range(n)]
    return _csr(ri, rv)


def diag_only(n, seed=0):
    rng = np.random.default_rng(seed)
    return _csr([np.array([i]) for i in range(n)], [np.array([_diag(rng)]) for i in range(n)])


def arrow(n, seed=0):
    """Diagonal, except that the last row holds all n entries: one very long row."""
    rng = np.random.default_rng(seed)
    ri = [np.array([i]) for i in range(n - 1)] + [np.arange(n)]
    rv = [np.array([_diag(rng)]) for i in range(n - 1)] + [np.append(_offdiag(rng, n - 1) if n > 1 else np.zeros(0), _diag(rng))]
    return _csr(ri, rv)


def shallow(n, seed=0):
    """Diagonal plus one random off-diagonal entry per row (a few dozen dependency levels of many rows each)."""
    rng = np.random.default_rng(seed)
    ri = [np.array([0])] + [np.array([rng.integers(0, i), i]) for i in range(1, n)]
    rv = [np.array([_diag(rng)])] + [np.append(_offdiag(rng, 1), _diag(rng)) for i in range(1, n)]
    return _csr(ri, rv)


PATTERNS = {"pattern": lambda n: pattern(n, SEED), "chain": chain, "diag_only": diag_only, "arrow": arrow}


def to_upper(ptr, idx, val):
    """Index reversal i → n−1−i of rows and columns: the mirrored upper-triangular matrix (sorted columns, diagonal first)."""
    n = len(ptr) - 1
    ri = [(n - 1 - idx[ptr[i]:ptr[i + 1]])[::-1] for i in range(n - 1, -1, -1)]
    rv = [val[ptr[i]:ptr[i + 1]][::-1] for i in range(n - 1, -1, -1)]
    return _csr(ri, rv)


def transpose_csr(ptr, idx, val):
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    tptr = np.zeros(n + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(idx, minlength=n))
    return tptr, rows[order].astype(np.int64), val[order]


def strip_diagonal(ptr, idx, val, rows=None):
    """The same matrix without the stored diagonal of `rows` (default: every row)."""
    n = len(ptr) - 1
    r = np.repeat(np.arange(n), np.diff(ptr))
    keep = r != idx if rows is None else ~((r == idx) & np.isin(r, rows))
    tptr = np.zeros(n + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(r[keep], minlength=n))
    return tptr, idx[keep], val[keep]


def dense(ptr, idx, val):
    n = len(ptr) - 1
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(ptr)), idx), val)
    return D


# ---- number formats --------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """Round to the nearest bf16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def round_to(x, dtype):
    """float64 array holding `x` rounded to the value type under test."""
    if dtype == "f64":
        return np.asarray(x, dtype=np.float64)
    if dtype == "f32":
        return np.asarray(x, dtype=np.float32).astype(np.float64)
    return bf16_round(x).astype(np.float64)


# ---- substitution, bound, emulation ----------------------------------------------------------------------------------------------
def _rows(n, lower):
    return range(n) if lower else range(n - 1, -1, -1)


def _split(ptr, idx, val, i, lower, unit):
    """(columns, values) of row i on the solved side of the diagonal, and the row's diagonal (unit: 1; none stored: 0)."""
    j, a = idx[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]
    side = j < i if lower else j > i
    d = a.dtype.type(1) if unit else a[j == i].sum()
    return j[side], a[side], d


def solve64(ptr, idx, val, B, lower, unit, real=np.float64):
    """op^-1 B by row-by-row substitution in float64 (`real`: a wider type for the reference of a float64 kernel).  Entries on the other
    side of the diagonal are ignored; with `unit`, a stored diagonal is ignored."""
    n = len(ptr) - 1
    val = np.asarray(val, dtype=real)
    X = np.array(B, dtype=real).reshape(n, -1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in _rows(n, lower):
            j, a, d = _split(ptr, idx, val, i, lower, unit)
            if len(j):
                X[i] -= a @ X[j]
            X[i] /= d
    return X


def bound(ptr, idx, val, x64, lower, unit, u, extra=0.0):
    """M(T)^-1 (γ ∘ |T||x|), γ_i = (len_i + 4)·u + extra: what |x − x64| of a correct solve of unit roundoff u stays within, element
    by element (len_i: stored entries of row i; M(T): |diagonal|, −|off-diagonal|)."""
    n = len(ptr) - 1
    absx = np.abs(np.asarray(x64, dtype=np.float64)).reshape(n, -1)
    absv = np.abs(np.asarray(val, dtype=np.float64))
    Y = np.zeros_like(absx)
    for i in _rows(n, lower):
        j, a, d = _split(ptr, idx, absv, i, lower, unit)
        gamma = (ptr[i + 1] - ptr[i] + 4) * u + extra
        r = gamma * (d * absx[i] + (a @ absx[j] if len(j) else 0.0))
        Y[i] = (r + (a @ Y[j] if len(j) else 0.0)) / d
    return Y


def emulate(ptr, idx, val, B, dtype, seed, lower=True, unit=False):
    """The same substitution as a kernel of `dtype` may carry it: float32 (float64 for "f64") products and additions with each row's
    terms summed in a random order, and for bf16 x rounded to bf16 once per row."""
    real = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(seed)
    n = len(ptr) - 1
    val = np.asarray(val, dtype=real)
    X = np.array(B, dtype=real).reshape(n, -1)
    for i in _rows(n, lower):
        j, a, d = _split(ptr, idx, val, i, lower, unit)
        acc = np.zeros(X.shape[1], dtype=real)
        for k in rng.permutation(len(j)):
            acc = acc + a[k] * X[j[k]]
        x = (X[i] - acc) / real(d)
        X[i] = bf16_round(x) if dtype == "bf16" else x
    return X.astype(np.float64)


def ratio(x, x64, bnd):
    """Worst |x − x64| / bound over the elements."""
    err = np.abs(np.asarray(x, dtype=np.longdouble) - np.asarray(x64, dtype=np.longdouble)).astype(np.float64)
    return float((err / (bnd + 1e-300)).max()) if err.size else 0.0


def rel_err(x, x64):
    x64 = np.asarray(x64, dtype=np.float64)
    return float(np.linalg.norm(np.asarray(x, dtype=np.float64) - x64) / max(np.linalg.norm(x64), 1e-300))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One operand as the solve's entry points take it (`api`: CSR arrays of A, with the upper / unit / transpose flags of
    sparse_triangular_solve) and as the matrix that is actually inverted (`eff`: CSR arrays of op(A), `lower`, `unit`), a right-hand
    side, its reference solution and the bound — all on inputs rounded to `dtype` first."""

    def __init__(self, kind, n, dtype, mode, p, seed=SEED):
        base = PATTERNS[kind](n)
        base = (base[0], base[1], round_to(base[2], dtype))
        self.dtype, self.mode, self.n, self.p = dtype, mode, n, p
        self.unit = mode == "lower_unit"
        self.transpose = mode == "lower_T"
        self.upper = mode == "upper"
        if mode == "upper":
            self.api = to_upper(*base)
        elif mode == "lower_unit":
            self.api = strip_diagonal(*base)          # (the unit diagonal is not stored)
        else:
            self.api = base
        self.eff = transpose_csr(*self.api) if self.transpose else self.api
        self.lower = mode in ("lower", "lower_unit")          # side of op(A)
        rng = np.random.default_rng(seed + 1000)
        self.B = round_to(rng.standard_normal((n, p)), dtype)
        self.G = round_to(rng.standard_normal((n, p)), dtype)          # the incoming gradient of the backward solve
        self._fwd = self._bwd = None

    def _ref(self, ptr, idx, val, rhs, lower):
        real = np.longdouble if self.dtype == "f64" else np.float64          # (a float64 kernel is held against a wider substitution)
        x = solve64(ptr, idx, val, rhs, lower, self.unit, real=real)
        return x, bound(ptr, idx, val, x, lower, self.unit, U[self.dtype], EXTRA[self.dtype])

    def forward(self):
        """(x64, bound) of op(A)^-1 B, computed once at the widest p: columns are independent, narrower solves are prefixes."""
        if self._fwd is None:
            self._fwd = self._ref(*self.eff, self.B, self.lower)
        return self._fwd

    def backward(self):
        """(g64, bound) of op(A)^-T G: the solve with the other transpose flag."""
        if self._bwd is None:
            self._bwd = self._ref(*transpose_csr(*self.eff), self.G, not self.lower)
        return self._bwd
