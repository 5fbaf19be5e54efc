"""numpy oracles of the zero-fill incomplete factorisations, and the patterns their tests share.

`ilu0` / `ic0` are the two loops of include/tsgu_hip_factor.h written out entry by entry: sequential, one rounding per operation in
the chosen dtype (ILU(0) on the GPU is compared with it bit for bit in the SAME dtype; everything else takes float64 as the
oracle).  Nothing here imports the package."""

import numpy as np


# ---------------------------------------------------------------------------------------------------------------------------
# oracles


def diag_positions(ptr, idx):
    n = len(ptr) - 1
    pos = np.empty(n, dtype=np.int64)
    for i in range(n):
        hit = np.nonzero(idx[ptr[i]:ptr[i + 1]] == i)[0]
        assert hit.size == 1, f"row {i} stores {hit.size} diagonal entries"
        pos[i] = ptr[i] + hit[0]
    return pos


def ilu0(ptr, idx, val, dtype=np.float64, shift=0.0):
    """(out, info): the IKJ loop, every operation rounded to `dtype`, updates of an entry in ascending k."""
    dt = np.dtype(dtype).type
    n = len(ptr) - 1
    a = np.asarray(val).astype(dtype)
    out = np.zeros_like(a)
    dpos = diag_positions(ptr, idx)
    scale = dt(1.0 + shift)
    info = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e = int(ptr[i]), int(ptr[i + 1])
            where = {int(idx[p]): p - s for p in range(s, e)}
            w = [dt(a[p]) for p in range(s, e)]
            w[where[i]] = dt(w[where[i]] * scale)
            for q in range(e - s):
                k = int(idx[s + q])
                if k >= i:
                    break
                w[q] = dt(w[q] / out[dpos[k]])
                for p in range(int(dpos[k]) + 1, int(ptr[k + 1])):
                    m = where.get(int(idx[p]))
                    if m is not None:
                        prod = dt(w[q] * out[p])
                        w[m] = dt(w[m] - prod)
            out[s:e] = w
            if out[dpos[i]] == 0 and not info:
                info = i + 1
    return out, info


def ic0(ptr, idx, val, dtype=np.float64, shift=0.0):
    """(out, info) on the CSR of tril(A) (ascending columns, the diagonal last): plain left-to-right sums in `dtype`."""
    dt = np.dtype(dtype).type
    n = len(ptr) - 1
    a = np.asarray(val).astype(dtype)
    out = np.zeros_like(a)
    scale = dt(1.0 + shift)
    info = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e = int(ptr[i]), int(ptr[i + 1])
            assert idx[e - 1] == i
            where = {int(idx[p]): p for p in range(s, e - 1)}
            for p in range(s, e - 1):
                k = int(idx[p])
                sk, ek = int(ptr[k]), int(ptr[k + 1])
                acc = dt(0)
                for pk in range(sk, ek - 1):
                    m = where.get(int(idx[pk]))
                    if m is not None and m < p:
                        acc = dt(acc + dt(out[m] * out[pk]))
                out[p] = dt(dt(a[p] - acc) / out[ek - 1])
            acc = dt(0)
            for p in range(s, e - 1):
                acc = dt(acc + dt(out[p] * out[p]))
            rad = dt(dt(a[e - 1] * scale) - acc)
            if not rad > 0 and not info:
                info = i + 1
            out[e - 1] = np.sqrt(rad)
    return out, info


def lower_csr(ptr, idx, val=None):
    """The CSR of tril(A) and the positions of its entries in A's arrays."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    pos = np.nonzero(idx <= rows)[0]
    lptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[pos], minlength=n), out=lptr[1:])
    return lptr, idx[pos], (None if val is None else np.asarray(val)[pos]), pos


def dense(ptr, idx, val, dtype=np.float64):
    n = len(ptr) - 1
    D = np.zeros((n, n), dtype=dtype)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    D[rows, idx] = val
    return D


def split_lu(ptr, idx, out):
    """Dense float64 (L with a unit diagonal, U) of a combined ILU array."""
    D = dense(ptr, idx, np.asarray(out, dtype=np.float64))
    return np.tril(D, -1) + np.eye(D.shape[0]), np.triu(D)


def pattern_residual_bound(ptr, idx, F, G, A, u):
    """For every stored (i, k) of the pattern: (|Σ_j F_ij·G_jk − A_ik|, (m_ik + 2)·u·Σ_j |F_ij·G_jk|) in float64, m_ik the number
    of non-zero terms — the componentwise backward-error bound of LU / Cholesky restricted to the pattern, valid for any order of
    the sums.  F, G, A dense float64; the products and sums of this check itself are formed in extended precision (np.longdouble),
    so that its own rounding does not count against a float64 factor whose bound is a few units of 2^-53."""
    n = len(ptr) - 1
    F, G, A = (np.asarray(x, dtype=np.longdouble) for x in (F, G, A))
    rows = np.repeat(np.arange(n), np.diff(ptr))
    err, bound = np.empty(idx.size, dtype=np.longdouble), np.empty(idx.size, dtype=np.longdouble)
    for a in range(0, idx.size, 1024):
        r, c = rows[a:a + 1024], idx[a:a + 1024]
        terms = F[r, :] * G[:, c].T                       # (entries, n)
        m = np.count_nonzero(terms, axis=1)
        err[a:a + 1024] = np.abs(terms.sum(axis=1) - A[r, c])
        bound[a:a + 1024] = (m + 2) * u * np.abs(terms).sum(axis=1)
    return err, bound


def lu_nopivot(D):
    """Dense LU without pivoting in float64: (unit lower L, upper U)."""
    U = np.array(D, dtype=np.float64)
    n = U.shape[0]
    L = np.eye(n)
    for k in range(n):
        for i in range(k + 1, n):
            if U[i, k] != 0:
                L[i, k] = U[i, k] / U[k, k]
                U[i, k:] -= L[i, k] * U[k, k:]
                U[i, k] = 0
    return L, U


# ---------------------------------------------------------------------------------------------------------------------------
# patterns: each returns (ptr, idx) int64 with ascending, unique columns and a stored diagonal


def from_dense_mask(mask):
    mask = np.array(mask, dtype=bool)
    n = mask.shape[0]
    mask[np.arange(n), np.arange(n)] = True
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(mask.sum(axis=1), out=ptr[1:])
    return ptr, np.nonzero(mask)[1].astype(np.int64)


def from_offsets(n, offsets):
    rows = np.arange(n)
    cols = [rows + d for d in sorted(set(offsets) | {0})]
    C = np.stack(cols, axis=1)
    ok = (C >= 0) & (C < n)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ok.sum(axis=1), out=ptr[1:])
    return ptr, C[ok].astype(np.int64)


def band(n, half):
    return from_offsets(n, range(-half, half + 1))


def stencil(nx, ny, nz, points):
    """7- or 27-point stencil on an nx × ny × nz lattice, truncated at the faces, rows in row-major order."""
    n = nx * ny * nz
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    x, y, z = x.ravel(), y.ravel(), z.ravel()
    cols, keep = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if points == 7 and abs(dx) + abs(dy) + abs(dz) > 1:
                    continue
                X, Y, Z = x + dx, y + dy, z + dz
                keep.append((X >= 0) & (X < nx) & (Y >= 0) & (Y < ny) & (Z >= 0) & (Z < nz))
                cols.append((X * ny + Y) * nz + Z)
    C, K = np.stack(cols, axis=1), np.stack(keep, axis=1)      # (offsets are generated in ascending column order)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(K.sum(axis=1), out=ptr[1:])
    return ptr, C[K].astype(np.int64)


def random_pattern(n, per_row, seed):
    """A symmetric random pattern with about `per_row` entries per row."""
    rng = np.random.default_rng(seed)
    mask = np.zeros((n, n), dtype=bool)
    r = np.repeat(np.arange(n), (per_row - 1) // 2)
    c = rng.integers(0, n, r.size)
    mask[r, c] = mask[c, r] = True
    return from_dense_mask(mask)


def arrow(n, tail, early, early_len):
    """Diagonal + the last `tail` rows and columns full up to `width` + row and column `early` holding `early_len` entries behind
    the diagonal: long rows at the end (each waits on hundreds of rows), one early row with a long upper part."""
    mask = np.zeros((n, n), dtype=bool)
    mask[n - tail:, :] = mask[:, n - tail:] = True
    mask[early, early:early + early_len + 1] = mask[early:early + early_len + 1, early] = True
    return from_dense_mask(mask)


def block_diagonal(sizes):
    n = sum(sizes)
    mask = np.zeros((n, n), dtype=bool)
    o = 0
    for b in sizes:
        mask[o:o + b, o:o + b] = True
        o += b
    return from_dense_mask(mask)


def downward_arrow(n):
    """Diagonal + last row + last column: no fill."""
    mask = np.zeros((n, n), dtype=bool)
    mask[n - 1, :] = mask[:, n - 1] = True
    return from_dense_mask(mask)


def dominant_values(ptr, idx, seed, symmetric=False, margin=1.0):
    """float64 values on the pattern: off-diagonal in [-1, 1], the diagonal = margin + the row's absolute sum (diagonally dominant;
    `symmetric`: the pattern must be, and the matrix is then SPD)."""
    rng = np.random.default_rng(seed)
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    val = rng.uniform(-1.0, 1.0, idx.size)
    if symmetric:
        D = np.zeros((n, n))
        D[rows, idx] = val
        D = np.tril(D, -1)
        D = D + D.T
        val = D[rows, idx]
    off = np.where(idx == rows, 0.0, np.abs(val))
    rowsum = np.bincount(rows, weights=off, minlength=n)
    val = np.where(idx == rows, margin + rowsum[rows], val)
    return val


def integer_cholesky_case(ptr, idx, seed):
    """(values of A = L0·L0ᵀ on the LOWER pattern (lptr, lidx), L0's values): L0 has small integers off the diagonal and powers of
    two on it, on a lower pattern WITHOUT fill (the caller chooses one), so every partial sum is an integer far below 2^24: exact in
    any order, and IC(0) must return L0 itself."""
    rng = np.random.default_rng(seed)
    lptr, lidx, _, _ = lower_csr(ptr, idx)
    n = len(lptr) - 1
    rows = np.repeat(np.arange(n), np.diff(lptr))
    l0 = rng.integers(-3, 4, lidx.size).astype(np.float64)
    l0 = np.where(lidx == rows, 2.0 ** rng.integers(0, 4, lidx.size), l0)
    L0 = dense(lptr, lidx, l0)
    A = L0 @ L0.T
    assert np.count_nonzero(np.tril(A)[dense(lptr, lidx, np.ones(lidx.size)) == 0]) == 0, "the pattern fills in"
    return lptr, lidx, A[rows, lidx], l0
