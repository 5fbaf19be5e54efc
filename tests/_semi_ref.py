"""2:4 semi-structured operands restated in numpy float64 (the checker of tests/test_sparse_semi_structured_cpu.py and
tests/test_gpu_sparse_semi_structured.py): prune, indices, to_dense and the three products.  Every product returns
(value, sum of |terms|, number of terms added per element): stored zeros are terms, dropped positions are not."""

import numpy as np


def prune(W):
    """(values (m, k / 2), cols (m, k / 2) int64 ascending) of W (m, k): per aligned group of four the two entries that rank first
    by (|w| descending, column ascending); NaN ranks above inf, -0 equals +0."""
    W = np.asarray(W, dtype=np.float64)
    m, k = W.shape
    assert k % 4 == 0
    g = W.reshape(m, k // 4, 4)
    nan = np.isnan(g)
    mag = np.where(nan, 0.0, np.abs(g))
    col = np.broadcast_to(np.arange(4), g.shape)
    order = np.lexsort((col, -mag, ~nan), axis=-1)                # last key first: NaN, then the magnitude, then the column
    pos = np.sort(order[..., :2], axis=-1)
    values = np.take_along_axis(g, pos, axis=-1).reshape(m, k // 2)
    cols = (pos + 4 * np.arange(k // 4)[None, :, None]).reshape(m, k // 2)
    return values, cols.astype(np.int64)


def indices(W):
    return prune(W)[1]


def to_dense(values, cols, k):
    values = np.asarray(values, dtype=np.float64)
    out = np.zeros((values.shape[0], k))
    np.put_along_axis(out, cols, values, axis=1)
    return out


def mm(values, cols, k, B):
    """A·B for B (k, p): k / 2 terms per element."""
    A, B = to_dense(values, cols, k), np.asarray(B, dtype=np.float64)
    return A @ B, np.abs(A) @ np.abs(B), k // 2


def mm_t(values, cols, k, G):
    """Aᵀ·G for G (m, p): m terms per element (a dropped position's column of A holds zeros that are never added, but the
    kernel's chain is the m rows)."""
    A, G = to_dense(values, cols, k), np.asarray(G, dtype=np.float64)
    return A.T @ G, np.abs(A).T @ np.abs(G), A.shape[0]


def sddmm(cols, G, Y):
    """(G·Yᵀ)[i, cols[i, s]] for G (m, p), Y (k, p): p terms per element."""
    G, Y = np.asarray(G, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    full, mag = G @ Y.T, np.abs(G) @ np.abs(Y).T
    return np.take_along_axis(full, cols, axis=1), np.take_along_axis(mag, cols, axis=1), G.shape[1]
