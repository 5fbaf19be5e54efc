"""The oracle of the semiring products (sparse_semiring_mm), restated in numpy float64.

Forward: a loop over the r-th stored entry of every row.  The candidate t = val[e] + B[col[e], :] is ONE addition in the accumulator
type `acc` (float32 for float32 and bfloat16 operands, float64 for float64) and everything after it is float64.  log: the
log-sum-exp of the row's candidates, -inf candidates absent, with wt = Σ_j w_j·|t_j| (w the weights) for the bounds.  Tropical: the
winner rule of _mm_reduce_ref.forward — strict compare, the first of equal candidates stays, a NaN replaces a number and then
stays — with the identity (-inf / +inf) and arg = -1 for a row without entries.

Gradients (float64) with the sums of absolute terms the bounds of tests/test_gpu_sparse_semiring.py are made of.
"""

import numpy as np

from _mm_reduce_ref import TORCH_DTYPE, random_csr, same_bits, small_ints  # noqa: F401  (shared with the tests)

SEMIRINGS = ("log", "max_plus", "min_plus")
ACC = {"float32": np.float32, "float64": np.float64, "bfloat16": np.float32}


def entries(crow, col, val, B, acc=np.float64):
    """(rows, e, t) for r = 0, 1, ...: the rows with more than r entries, their r-th entry and its candidates (float64)."""
    crow, col = np.asarray(crow, dtype=np.int64), np.asarray(col, dtype=np.int64)
    lens = np.diff(crow)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(int(lens.max()) if len(lens) else 0):
            rows = np.nonzero(lens > r)[0]
            e = crow[rows] + r
            yield rows, e, (val[e][:, None].astype(acc) + B[col[e]].astype(acc)).astype(np.float64)


def forward(crow, col, val, B, semiring, acc=np.float64):
    """log: (C, None, wt); tropical: (C, arg, None).  float64."""
    n, p = len(crow) - 1, B.shape[1]
    val, B = np.asarray(val, dtype=np.float64), np.asarray(B, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if semiring == "log":
            M = np.full((n, p), -np.inf)
            for rows, _, t in entries(crow, col, val, B, acc):
                M[rows] = np.maximum(M[rows], t)                     # (NaN propagates)
            shift = np.where(np.isfinite(M), M, 0.0)
            S = np.zeros((n, p))
            for rows, _, t in entries(crow, col, val, B, acc):
                S[rows] += np.exp(t - shift[rows])
            C = shift + np.log(S)
            wt = np.zeros((n, p))
            for rows, _, t in entries(crow, col, val, B, acc):
                wt[rows] += np.where(np.isfinite(t), np.exp(t - C[rows]) * np.abs(t), 0.0)
            return C, None, wt
        C = np.full((n, p), np.inf if semiring == "min_plus" else -np.inf)
        arg = np.full((n, p), -1, dtype=np.int32)
        for rows, e, t in entries(crow, col, val, B, acc):
            best, who = C[rows], arg[rows]
            better = (t < best) if semiring == "min_plus" else (t > best)
            take = (who < 0) | better | (np.isnan(t) & ~np.isnan(best))
            C[rows] = np.where(take, t, best)
            arg[rows] = np.where(take, e[:, None].astype(np.int32), who)
        return C, arg, None


def forward_bound(crow, C, wt, u):
    """The log forward's bound per element: (3L + 32 + 8 ln(1 + L)) u + u (Σ w|t| + 2 |C|), L the row's length."""
    L = np.diff(np.asarray(crow, dtype=np.int64)).astype(np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        return (3 * L + 32 + 8 * np.log1p(L)) * u + u * (wt + 2 * np.abs(C))


def gradients(crow, col, val, B, G, semiring, C, arg, fb, u, acc=np.float64):
    """(dval, bound of dval, dB, bound of dB) in float64.  log: W = exp(t - C) with `fb` the forward bound of the stored C;
    tropical: W = [arg == e] and the bounds are (p + 2) u Σ|G| and (L_j + 2) u Σ|G| over the winners."""
    val, B, G = (np.asarray(x, dtype=np.float64) for x in (val, B, G))
    col = np.asarray(col, dtype=np.int64)
    nnz, (m, p) = len(col), B.shape
    Lj = np.bincount(col, minlength=m).astype(np.float64)
    dval, bnd_a, dB, bnd_b = np.zeros(nnz), np.zeros(nnz), np.zeros((m, p)), np.zeros((m, p))
    with np.errstate(invalid="ignore", over="ignore"):
        for rows, e, t in entries(crow, col, val, B, acc):
            j = col[e]
            if semiring == "log":
                live = t != -np.inf
                W = np.where(live, np.exp(t - C[rows]), 0.0)
                rho = np.where(live, fb[rows] + u * (2 * np.abs(t) + np.abs(C[rows])), 0.0)
                term, mag = G[rows] * W, np.abs(G[rows]) * W
                ea, eb = mag * (rho + (p + 4) * u), mag * (rho + (Lj[j][:, None] + 4) * u)
            else:
                won = arg[rows] == e[:, None]
                term = np.where(won, G[rows], 0.0)
                ea, eb = np.abs(term) * (p + 2) * u, np.abs(term) * (Lj[j][:, None] + 2) * u
            dval[e], bnd_a[e] = term.sum(1), ea.sum(1)
            np.add.at(dB, j, term)
            np.add.at(bnd_b, j, eb)
    return dval, bnd_a, dB, bnd_b
