"""The oracle of the block-sparse products (sparse_bsr_mm) in numpy float64, and the patterns its tests share.

A is (crow[nrb + 1], col[nnzb], val[nnzb, bh, bw]): every stored block is a term, in stored order; columns need not be sorted and a
repeated (I, J) is two terms.  Every result comes with the sum of the absolute values of its terms (what a rounding bound scales
with) and with the number of its terms.
"""

import numpy as np


def block_rows(crow):
    """Block row of every stored block."""
    crow = np.asarray(crow, dtype=np.int64)
    return np.repeat(np.arange(len(crow) - 1, dtype=np.int64), np.diff(crow))


def forward(crow, col, val, B, bh, bw):
    """(C, sum |terms| of every element of C, terms of every row of C) for C = A·B; C is (nrb·bh, p)."""
    val, B = np.asarray(val, dtype=np.float64).reshape(-1, bh, bw), np.asarray(B, dtype=np.float64)
    nrb, p = len(crow) - 1, B.shape[1]
    rows, col = block_rows(crow), np.asarray(col, dtype=np.int64)
    C, mag = np.zeros((nrb, bh, p)), np.zeros((nrb, bh, p))
    if len(col):
        slabs = B.reshape(-1, bw, p)[col]
        np.add.at(C, rows, np.einsum("erk,ekp->erp", val, slabs))
        np.add.at(mag, rows, np.einsum("erk,ekp->erp", np.abs(val), np.abs(slabs)))
    terms = np.repeat(np.diff(np.asarray(crow, dtype=np.int64)) * bw, bh)
    return C.reshape(nrb * bh, p), mag.reshape(nrb * bh, p), terms


def gradients(crow, col, val, B, G, bh, bw):
    """(dV, sum |terms| of dV, dB, sum |terms| of dB, terms of every row of dB): dV[e] = G[I_e] · B[J_e]ᵀ (p terms each),
    dB = Aᵀ·G ((blocks of the block column)·bh terms)."""
    val, B, G = (np.asarray(x, dtype=np.float64) for x in (val, B, G))
    val = val.reshape(-1, bh, bw)
    p = B.shape[1]
    ncb = B.shape[0] // bw
    rows, col = block_rows(crow), np.asarray(col, dtype=np.int64)
    dB, mag_b = np.zeros((ncb, bw, p)), np.zeros((ncb, bw, p))
    if len(col):
        g, b = G.reshape(-1, bh, p)[rows], B.reshape(-1, bw, p)[col]
        dV = np.einsum("erp,ecp->erc", g, b)
        mag_v = np.einsum("erp,ecp->erc", np.abs(g), np.abs(b))
        np.add.at(dB, col, np.einsum("erc,erp->ecp", val, g))
        np.add.at(mag_b, col, np.einsum("erc,erp->ecp", np.abs(val), np.abs(g)))
    else:
        dV, mag_v = np.zeros((0, bh, bw)), np.zeros((0, bh, bw))
    terms_b = np.repeat(np.bincount(col, minlength=ncb) * bh, bw)
    return dV, mag_v, dB.reshape(ncb * bw, p), mag_b.reshape(ncb * bw, p), terms_b


def random_bsr(nrb, ncb, lens, seed, duplicates=False, index_dtype=np.int64, canonical=False):
    """(crow, col) of a block pattern with `lens[i]` blocks in block row i: columns in random (unsorted) order, drawn with
    replacement when a row is longer than the matrix is wide; with `duplicates` every row of two or more blocks repeats its first
    column as its last.  `canonical`: columns sorted and distinct instead, the form torch's own sparse ops assume."""
    rng = np.random.default_rng(seed)
    assert len(lens) == nrb
    crow = np.concatenate(([0], np.cumsum(lens))).astype(index_dtype)
    cols = []
    for L in lens:
        L = int(L)
        c = rng.choice(ncb, size=L, replace=L > ncb) if L else np.zeros(0, dtype=np.int64)
        if canonical:
            c = np.sort(rng.choice(ncb, size=L, replace=False))
        elif duplicates and L >= 2:
            c[-1] = c[0]
        cols.append(c)
    col = (np.concatenate(cols) if cols and crow[-1] else np.zeros(0)).astype(index_dtype)
    return crow, col


def small_ints(shape, seed, lo=-1, hi=2):
    """Small integers (exact in every value type, bfloat16 included)."""
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.float64)
