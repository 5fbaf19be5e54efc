"""numpy oracle of the factorised sparse approximate inverse (include/tsgu_hip_fsai.h), and what its tests share.

`fsai` is the definition written out row by row: gather A[J,J] from tril(A), solve A[J,J]·y = e_m with numpy's dense solver in
the chosen dtype, scale by 1 / sqrt(y_m).  The patterns and `dominant_values` are those of tests/_factor_ref.py.  Nothing here
imports the package."""

import numpy as np

from _factor_ref import (band, block_diagonal, dense, dominant_values, from_dense_mask, lower_csr,  # noqa: F401  (shared with the tests)
                         random_pattern, stencil)


def local_matrix(ptr, idx, val, J):
    """A[J,J] (symmetric, dense, dtype of `val`) from the CSR (ptr, idx, val) of tril(A): A[j_a, j_b] with j_b <= j_a is taken from
    row j_a, a position that is not stored is zero."""
    m = len(J)
    M = np.zeros((m, m), dtype=np.asarray(val).dtype)
    where = {int(j): b for b, j in enumerate(J)}
    for a, j in enumerate(J):
        for p in range(int(ptr[j]), int(ptr[j + 1])):
            b = where.get(int(idx[p]))
            if b is not None and b <= a:
                M[a, b] = M[b, a] = val[p]
    return M


def fsai(ptr, idx, val, sptr, sidx, dtype=np.float64):
    """(values of G on the lower pattern (sptr, sidx), info) for the CSR (ptr, idx, val) of tril(A); columns ascending, the diagonal
    last in every row of both.  info: 0, or 1 + the lowest row with y_m <= 0 or NaN."""
    n = len(sptr) - 1
    a = np.asarray(val).astype(dtype)
    out = np.zeros(len(sidx), dtype=dtype)
    info = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e = int(sptr[i]), int(sptr[i + 1])
            J = sidx[s:e]
            assert J[-1] == i and np.all(np.diff(J) > 0)
            M = local_matrix(ptr, idx, a, J)
            rhs = np.zeros(e - s, dtype=dtype)
            rhs[-1] = 1
            y = np.linalg.solve(M, rhs).astype(dtype)
            if not y[-1] > 0 and not info:
                info = i + 1
            out[s:e] = y / np.sqrt(y[-1])
    return out, info


def power_lower_pattern(ptr, idx, k):
    """(lptr, lidx): the lower triangle of the pattern of the k-th power of the pattern (ptr, idx) (k >= 1; structural: no
    cancellation)."""
    n = len(ptr) - 1
    P = dense(ptr, idx, np.ones(len(idx))) != 0
    Q = P.copy()
    for _ in range(k - 1):
        Q = (Q.astype(np.int64) @ P.astype(np.int64)) != 0
    lptr, lidx = from_dense_mask(np.tril(Q))
    return lptr, lidx


def row_residuals(ptr, idx, val, sptr, sidx, g, u):
    """For every row of S, in float64 from the inputs as given and the computed g:
    (‖A[J,J]·g − e_m / g_m‖₂, (3m + 5)·m·u·‖A[J,J]‖₂·‖g‖₂, m) — the normwise backward-error bound of a Cholesky solve (Higham,
    Accuracy and Stability, Thm 10.4 with ‖|Rᵀ||R|‖₂ <= m·‖A‖₂) plus the roundings of the scaling."""
    n = len(sptr) - 1
    a = np.asarray(val, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    res, bound, size = np.empty(n), np.empty(n), np.empty(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e = int(sptr[i]), int(sptr[i + 1])
            m = e - s
            M = local_matrix(ptr, idx, a, sidx[s:e])
            gi = g[s:e]
            rhs = np.zeros(m)
            rhs[-1] = 1.0 / gi[-1]
            res[i] = np.linalg.norm(M @ gi - rhs)
            bound[i] = (3 * m + 5) * m * u * np.linalg.norm(M, 2) * np.linalg.norm(gi)
            size[i] = m
    return res, bound, size


def dense_lower(sptr, sidx, g):
    return dense(sptr, sidx, np.asarray(g, dtype=np.float64))
