"""sparse_topk_mm restated in numpy: float64 (or exact integer) scores, the allowed mask, the selection by a stable sort on
(−score, column) with NaN first, and the closed-form row pointer.  Shared by tests/test_sparse_topk_cpu.py and
tests/test_gpu_sparse_topk.py; nothing here imports the package."""

import numpy as np


def scores(Q, K, scale=1.0, key_bias=None):
    """scale·Q·Kᵀ + key_bias in float64 for Q [n, d], K [m, d] (integer inputs give exact integers below 2^53)."""
    S = scale * (np.asarray(Q, dtype=np.float64) @ np.asarray(K, dtype=np.float64).T)
    if key_bias is not None:
        S = S + np.asarray(key_bias, dtype=np.float64)[None, :]
    return S


def allowed(n, m, causal=False, exclude_self=False):
    """[n, m] bool: all j < m; causal: j <= i + (m − n); exclude_self: j != i."""
    i = np.arange(n)[:, None]
    j = np.arange(m)[None, :]
    ok = np.ones((n, m), dtype=bool)
    if causal:
        ok &= j <= i + (m - n)
    if exclude_self:
        ok &= j != i
    return ok


def crow(n, m, k, causal=False, exclude_self=False):
    """The row pointer in closed form (int64 [n + 1]): row i stores min(k, allowed(i)) entries."""
    i = np.arange(n, dtype=np.int64)
    lim = np.clip(i + (m - n + 1), 0, m) if causal else np.full(n, m, dtype=np.int64)
    if exclude_self:
        lim = lim - (i < lim)
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.minimum(lim, k))
    return out


def order(S, ok):
    """Per row, the allowed columns from best to worst: NaN first, then descending score (−0 = +0), the lower column first among equal
    scores.  A list of int64 arrays."""
    out = []
    for i in range(S.shape[0]):
        cols = np.flatnonzero(ok[i])
        s = S[i, cols]
        nan = np.isnan(s)
        key = np.where(nan, -np.inf, -np.where(nan, 0.0, s))        # NaN ahead of +inf's −inf: ties among them by column
        first = np.lexsort((cols, ~nan, key))                          # last key is the primary one; NaN before a −inf key of +inf
        out.append(cols[first])
    return out


def select(S, k, ok):
    """(crow, col, val): the best min(k, allowed) columns of every row, ascending, and their scores."""
    n = S.shape[0]
    ptr = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for i, best in enumerate(order(S, ok)):
        keep = np.sort(best[:k])
        ptr[i + 1] = ptr[i] + keep.size
        cols.append(keep)
        vals.append(S[i, keep])
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    val = np.concatenate(vals) if vals else np.zeros(0)
    return ptr, col.astype(np.int64), val


def boundary_ties(S, k, ok):
    """[n] bool: the k-th and (k+1)-th best allowed scores of the row are equal — the lower-column rule decides the set."""
    out = np.zeros(S.shape[0], dtype=bool)
    for i, best in enumerate(order(S, ok)):
        if best.size > k:
            a, b = S[i, best[k - 1]], S[i, best[k]]
            out[i] = a == b or (np.isnan(a) and np.isnan(b))
    return out
