"""The oracle of the max / min products (sparse_mm_reduce), restated in numpy, and the matrices its tests share.

Forward: a loop over the stored entries of every row, in stored order; the product val[e]·B[col[e],:] is ONE IEEE multiplication
in the accumulator type (float32 for float32 and bfloat16 operands, float64 for float64); a candidate replaces the running one on
a strict > / < (so the first of equal candidates stays, +0.0 == -0.0 included), a NaN replaces any number and then stays.  A row
without entries gives 0 and arg = -1.  bfloat16 results are the float32 result rounded once.  tests/test_sparse_mm_reduce_cpu.py pins this
against torch.sparse.mm(A, B, reduce) on the CPU, bit for bit; the GPU tests compare the kernels with it.

Gradients (float64): through the winner only, with the sum of the absolute terms each bound is made of.
"""

import numpy as np
import torch

TORCH_DTYPE = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}


def to_acc(t: torch.Tensor) -> np.ndarray:
    """A tensor of the value type as a numpy array of its accumulator type (exact)."""
    return t.detach().cpu().to(torch.float64 if t.dtype == torch.float64 else torch.float32).numpy()


def forward(crow, col, val, B, reduce):
    """(C, arg) in the accumulator type of val / B (numpy arrays of that type)."""
    assert val.dtype == B.dtype and val.dtype in (np.float32, np.float64)
    n, p = len(crow) - 1, B.shape[1]
    crow, col = np.asarray(crow, dtype=np.int64), np.asarray(col, dtype=np.int64)
    C = np.zeros((n, p), dtype=val.dtype)
    arg = np.full((n, p), -1, dtype=np.int32)
    lens = np.diff(crow)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(lens.max()) if n else 0):          # the r-th entry of every row that has one: rows are independent
            rows = np.nonzero(lens > r)[0]
            e = crow[rows] + r
            x = val[e][:, None] * B[col[e]]
            best, who = C[rows], arg[rows]
            better = (x < best) if reduce == "amin" else (x > best)
            take = (who < 0) | better | (np.isnan(x) & ~np.isnan(best))
            C[rows] = np.where(take, x, best)
            arg[rows] = np.where(take, e[:, None].astype(np.int32), who)
    return C, arg


def gradients(crow, col, val, B, G, arg):
    """(dval, sum |G·B| per entry, dB, sum |val·G| per element of dB) in float64 from the winners `arg`."""
    val, B, G = (np.asarray(x, dtype=np.float64) for x in (val, B, G))
    nnz, (m, p) = len(col), B.shape
    dval, abs_a = np.zeros(nnz), np.zeros(nnz)
    dB, abs_b = np.zeros((m, p)), np.zeros((m, p))
    i, k = np.nonzero(arg >= 0)
    e = arg[i, k].astype(np.int64)
    j = np.asarray(col, dtype=np.int64)[e]
    with np.errstate(invalid="ignore", over="ignore"):
        ta = G[i, k] * B[j, k]
        tb = val[e] * G[i, k]
    np.add.at(dval, e, ta)
    np.add.at(abs_a, e, np.abs(ta))
    np.add.at(dB, (j, k), tb)
    np.add.at(abs_b, (j, k), np.abs(tb))
    return dval, abs_a, dB, abs_b


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal bit patterns, except that any NaN equals any NaN (the payload of a NaN is not part of the semantics)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu(), b.detach().cpu()
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    word = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.masked_fill(nan, 0).view(word), b.masked_fill(nan, 0).view(word))


def random_csr(n, m, lens, seed, index_dtype=np.int64):
    """(crow, col) with `lens[i]` distinct sorted columns in row i."""
    rng = np.random.default_rng(seed)
    crow = np.concatenate(([0], np.cumsum(lens))).astype(index_dtype)
    cols = [np.sort(rng.choice(m, size=int(L), replace=False)) if L <= m else None for L in lens]
    assert all(c is not None for c in cols), "a row cannot be longer than the matrix is wide"
    col = (np.concatenate(cols) if len(cols) and crow[-1] else np.zeros(0)).astype(index_dtype)
    return crow, col


def small_ints(shape, seed, lo=-3, hi=4):
    """Small integers (exact in every value type, bfloat16 included): their products tie by the dozen."""
    return np.random.default_rng(seed).integers(lo, hi, size=shape).astype(np.float64)
