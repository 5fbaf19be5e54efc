"""Float64 mirror of the Lanczos quadrature (csrc/tsgu_hip_quadrature.h) and the test matrices of sparse_logdet, in numpy.

Nothing here imports the package: the mirror is written from the header's text — the entries of T from (alpha, beta), the
per-column length rule, `numpy.linalg.eigh` for the nodes and weights, the probe hash — so that it can disagree with the code.
"""

import numpy as np

U = 2.0 ** -53
FN_LOG, FN_RECIPROCAL, FN_IDENTITY, FN_ONE = 0, 1, 2, 3
KIND_CG, KIND_ENTRIES = 0, 1


# ---- the probe function -------------------------------------------------------------------------------------------------------------

def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def rademacher(seed: int, n: int, p: int) -> np.ndarray:
    """out[i][c] = -1 if lowbias32(c + lowbias32(i + s)) >> 31 else +1, s = lowbias32(lo32(seed) ^ lowbias32(hi32(seed)))."""
    m = np.uint64(0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = lowbias32(np.uint64(seed & 0xFFFFFFFF) ^ lowbias32(np.uint64(seed >> 32)))
    rows = lowbias32((np.arange(n, dtype=np.uint64) + s) & m)
    h = lowbias32((np.arange(p, dtype=np.uint64)[None, :] + rows[:, None]) & m)
    return np.where((h >> np.uint64(31)) != 0, -1.0, 1.0)


# ---- T, the length rule, the quadrature -----------------------------------------------------------------------------------------------

def _positive_finite(v):
    return np.isfinite(v) & (v > 0)


def tridiagonal(col: np.ndarray, kind: int):
    """(d, e) of one column's matrix, `col` = [r][2] in float64: len(d) = r_c, len(e) = r_c - 1."""
    a, b = col[:, 0].astype(np.float64), col[:, 1].astype(np.float64)
    r = len(a)
    if kind == KIND_CG:
        bad_a = np.flatnonzero(~_positive_finite(a))
        n = int(bad_a[0]) if bad_a.size else r            # ends BEFORE the first alpha that is not positive and finite
        bad_b = np.flatnonzero(~_positive_finite(b[:n]))
        if bad_b.size:
            n = int(bad_b[0]) + 1                          # ends AFTER the first beta that is not positive and finite
        if n == 0:
            return np.zeros(0), np.zeros(0)
        ia = 1.0 / a[:n]
        d = ia.copy()
        d[1:] += b[: n - 1] * ia[: n - 1]
        e = np.sqrt(b[: max(n - 1, 0)]) * ia[: max(n - 1, 0)]
        return d, e
    bad = np.flatnonzero((b == 0) | ~np.isfinite(b))
    n = int(bad[0]) + 1 if bad.size else r
    return a[:n].copy(), b[: n - 1].copy()


def dense_t(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def apply_fn(fn: int, lam):
    with np.errstate(all="ignore"):
        return (np.log(lam), 1.0 / lam, lam, np.ones_like(lam))[fn]


def quadrature(coef: np.ndarray, kind: int, fn: int, scale=None):
    """(out, info, bound) per column of `coef` [r][2][p]: the header's contract in float64 through eigh, and the kernel-test bound
    64·r·2⁻⁵³·(‖T‖_∞ / λ_min + max_j |f(λ_j)|) (times |scale|); NaN out and bound for a column with info < 0."""
    r, _, p = coef.shape
    out, info, bound = np.zeros(p), np.zeros(p, dtype=np.int32), np.zeros(p)
    for c in range(p):
        d, e = tridiagonal(np.asarray(coef[:, :, c], dtype=np.float64), kind)
        n = len(d)
        info[c] = n
        if n == 0:
            continue
        T = dense_t(d, e)
        lam, vec = np.linalg.eigh(T)
        if fn <= FN_RECIPROCAL and lam.min() <= 0:
            out[c], info[c], bound[c] = np.nan, -n, np.nan
            continue
        f = apply_fn(fn, lam)
        sc = 1.0 if scale is None else float(scale[c])
        out[c] = sc * float((vec[0] ** 2 * f).sum())
        bound[c] = abs(sc) * 64 * r * U * (np.abs(T).sum(axis=1).max() / np.abs(lam).min() + np.abs(f).max())
    return out, info, bound


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------

def laplacian5(nx: int, ny: int, shift: float) -> np.ndarray:
    n = nx * ny
    A = np.zeros((n, n))
    for i in range(nx):
        for j in range(ny):
            k = i * ny + j
            A[k, k] = 4.0 + shift
            if i > 0:
                A[k, k - ny] = -1.0
            if i < nx - 1:
                A[k, k + ny] = -1.0
            if j > 0:
                A[k, k - 1] = -1.0
            if j < ny - 1:
                A[k, k + 1] = -1.0
    return A


def random_dominant(n: int, per_row: int = 4, margin: float = 0.3, seed: int = 0) -> np.ndarray:
    """Random symmetric, `per_row` draws per row before symmetrising, strictly diagonally dominant by `margin`."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    for i in range(n):
        c = rng.choice(n, per_row, replace=False)
        M[i, c] = rng.standard_normal(per_row)
    S = (M + M.T) / 2
    np.fill_diagonal(S, 0.0)
    S += np.diag(np.abs(S).sum(axis=1) + margin)
    return S


MATRICES = {
    "lap8x8": lambda: laplacian5(8, 8, 0.5),          # n = 64: one full wave of columns
    "lap7x9": lambda: laplacian5(7, 9, 0.05),         # n = 63: a partial wave
    "rand96": lambda: random_dominant(96, 4, 0.3),    # n = 96: one and a half
}


def csr_arrays(A: np.ndarray):
    """(crow, col, val) of the non-zero entries of a dense matrix, rows in column order."""
    mask = A != 0
    crow = np.concatenate(([0], np.cumsum(mask.sum(axis=1))))
    rows, cols = np.nonzero(mask)
    return crow.astype(np.int64), cols.astype(np.int64), A[rows, cols]


# ---- CG coefficient histories ---------------------------------------------------------------------------------------------------------

def cg_history(A: np.ndarray, Z: np.ndarray, steps: int, dtype=np.float32) -> np.ndarray:
    """hist [steps][2][p] of (alpha, beta): conjugate gradients from x = 0 on A x = z_c / |z_c| with every operation rounded to
    `dtype`.  A column is frozen (alpha = beta = 0 from there on) once |r| < 1e-10 or p'Ap is not positive: what the kernel's length
    rule is for."""
    A = A.astype(dtype)
    p = Z.shape[1]
    hist = np.zeros((steps, 2, p), dtype=dtype)
    for c in range(p):
        r = (Z[:, c] / np.linalg.norm(Z[:, c])).astype(dtype)
        pv = r.copy()
        rr = dtype(r @ r)
        for k in range(steps):
            Ap = (A @ pv).astype(dtype)
            pap = dtype(pv @ Ap)
            if not pap > 0 or np.sqrt(rr) < 1e-10:
                break
            alpha = dtype(rr / pap)
            r = (r - alpha * Ap).astype(dtype)
            rn = dtype(r @ r)
            beta = dtype(rn / rr)
            hist[k, 0, c], hist[k, 1, c] = alpha, beta
            pv = (r + beta * pv).astype(dtype)
            rr = rn
    return hist


def jacobi(spectrum: np.ndarray, rng) -> tuple:
    """(d, e) of a Jacobi matrix with the prescribed spectrum: a random orthogonal similarity of diag(spectrum), brought to
    tridiagonal form by Lanczos with full reorthogonalisation from a random start (off-diagonals positive)."""
    n = len(spectrum)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    M = (Q * spectrum) @ Q.T
    M = (M + M.T) / 2
    V = np.zeros((n, n))
    d, e = np.zeros(n), np.zeros(max(n - 1, 0))
    v = rng.standard_normal(n)
    V[:, 0] = v / np.linalg.norm(v)
    for k in range(n):
        w = M @ V[:, k]
        d[k] = V[:, k] @ w
        if k == n - 1:
            break
        for _ in range(2):
            w -= V[:, : k + 1] @ (V[:, : k + 1].T @ w)
        e[k] = np.linalg.norm(w)
        V[:, k + 1] = w / e[k]
    return d, e
