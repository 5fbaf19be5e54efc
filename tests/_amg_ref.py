"""The aggregation multigrid of sparse_amg, written out in numpy: the oracle of test_sparse_amg_cpu.py and test_gpu_sparse_amg.py.
Imports nothing from the package.

Matrices of the hierarchy are held DENSE with a boolean mask of their stored positions (the structural pattern: an entry that
cancels stays stored), so the oracle is for a few thousand rows at the most.  Sums run in numpy's order, not the kernels': the tests
compare within a tolerance, the aggregates exactly.
"""

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
DENSE_COARSE_MAX = 4096


# ---- problems -------------------------------------------------------------------------------------------------------------------------

def stencil(dims, weights=(1.0, 1.0, 1.0), full=False):
    """CSR (ptr, idx, val) in float64 of a Dirichlet stencil on an nx × ny × nz lattice, columns ascending.  7-point: −w_d towards
    the two neighbours along axis d and 2·Σw on the diagonal.  `full`: the 27-point stencil with −1 towards all 26 neighbours and
    26 on the diagonal."""
    nx, ny, nz = dims
    rows, cols, vals = [], [], []
    if full:
        offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    else:
        offs = [(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    X, Y, Z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    me = (X * ny + Y) * nz + Z
    for a, b, c in offs:
        ok = (X + a >= 0) & (X + a < nx) & (Y + b >= 0) & (Y + b < ny) & (Z + c >= 0) & (Z + c < nz)
        other = ((X + a) * ny + (Y + b)) * nz + (Z + c)
        if (a, b, c) == (0, 0, 0):
            v = 26.0 if full else 2.0 * sum(weights)
        else:
            v = -1.0 if full else -float(weights[0] * abs(a) + weights[1] * abs(b) + weights[2] * abs(c))
        rows.append(me[ok])
        cols.append(other[ok])
        vals.append(np.full(int(ok.sum()), v))
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    n = nx * ny * nz
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return ptr, cols[order].astype(np.int64), vals[order]


def to_dense(ptr, idx, val):
    """(dense matrix, boolean mask of the stored positions) of a square CSR matrix."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    D = np.zeros((n, n), dtype=val.dtype)
    D[rows, idx] = val
    mask = np.zeros(D.shape, dtype=bool)
    mask[rows, idx] = True
    return D, mask


def to_csr(D, mask):
    rows, idx = np.nonzero(mask)
    ptr = np.zeros(D.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=D.shape[0]), out=ptr[1:])
    return ptr, idx.astype(np.int64), D[rows, idx]


# ---- MIS-2 aggregation ------------------------------------------------------------------------------------------------------------------

def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def hop(ptr, idx, keys):
    """out[i] = max(keys[i], max_{j in row i} keys[j]) over unsigned 64-bit keys."""
    out = keys.copy()
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    np.maximum.at(out, rows, keys[idx])
    return out


def mis2_keys(ptr, idx):
    """(final keys, rounds) of the MIS-2 rounds — key = state << 62 | prio << 32 | index, state 2 = root, 1 = undecided, 0 = removed."""
    n = len(ptr) - 1
    i = np.arange(n, dtype=np.uint64)
    low = np.uint64((1 << 62) - 1)
    key = (np.uint64(1) << np.uint64(62)) | ((lowbias32(i) >> np.uint64(2)) << np.uint64(32)) | i
    rounds = 0
    while np.any((key >> np.uint64(62)) == 1):
        t = hop(ptr, idx, hop(ptr, idx, key))
        und = (key >> np.uint64(62)) == 1
        root = und & ((t & M32) == i)
        gone = und & ~root & ((t >> np.uint64(62)) == 2)
        key = np.where(root, (np.uint64(2) << np.uint64(62)) | (key & low), np.where(gone, key & low, key))
        rounds += 1
        assert rounds <= n + 1
    return key, rounds


def mis2_aggregate(ptr, idx):
    """(aggregate of every node, number of aggregates, rounds): every node joins the root with the largest key within distance 1,
    else within distance 2; aggregates are numbered by their roots' ascending index."""
    key, rounds = mis2_keys(ptr, idx)
    is_root = (key >> np.uint64(62)) == 2
    k = np.where(is_root, key, np.uint64(0))
    a1 = hop(ptr, idx, k)
    a2 = hop(ptr, idx, a1)
    a = np.where(a1 != 0, a1, a2)
    rank = np.cumsum(is_root) - 1
    return rank[(a & M32).astype(np.int64)].astype(np.int64), int(is_root.sum()), rounds


def mis2_properties(ptr, idx, agg):
    """(no two roots within distance 2 of each other, every node within distance 2 of its root), by dense reachability."""
    n = len(ptr) - 1
    _, mask = to_dense(ptr, idx, np.ones(len(idx)))
    reach1 = (mask | np.eye(n, dtype=bool)).astype(np.float32)
    reach2 = (reach1 @ reach1) > 0
    roots = np.nonzero((mis2_keys(ptr, idx)[0] >> np.uint64(62)) == 2)[0]          # ascending index = aggregate number
    apart = not np.any(reach2[np.ix_(roots, roots)] & ~np.eye(len(roots), dtype=bool))
    near = bool(np.all(reach2[np.arange(n), roots[agg]]))
    return apart, near


# ---- the hierarchy ----------------------------------------------------------------------------------------------------------------------

def filtered(ptr, idx, val, theta):
    """CSR of A_F: the diagonal and every off-diagonal with |a_ij| >= theta·sqrt(|a_ii·a_jj|); dropped values go to the diagonal."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    if theta <= 0:
        return ptr, idx, val
    d = np.zeros(n, dtype=val.dtype)
    d[rows[rows == idx]] = val[rows == idx]
    keep = (rows == idx) | (np.abs(val) >= val.dtype.type(theta) * np.sqrt(np.abs(d[rows] * d[idx])))
    lump = np.zeros(n, dtype=val.dtype)
    np.add.at(lump, rows[~keep], val[~keep])
    fval = val.copy()
    fval[rows == idx] += lump
    fptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=fptr[1:])
    return fptr, idx[keep], fval[keep]


def rho_hat(D, mask):
    return np.max((np.abs(D) * mask).sum(axis=1) / np.diag(D))


def hierarchy(ptr, idx, val, theta, sweeps, coarse_size, max_levels, dtype):
    """The levels as dicts: n, nnz, A / mask (dense), ptr / idx / val (CSR), w, theta, agg, n_c, P / Pmask, and on the last one
    solver ("dense" with inv, or "smoother")."""
    dtype = np.dtype(dtype).type
    val = val.astype(dtype)
    levels = []
    four, three = dtype(4), dtype(3)
    while True:
        n = len(ptr) - 1
        A, mask = to_dense(ptr, idx, val)
        lv = dict(n=n, nnz=len(idx), ptr=ptr, idx=idx, val=val, A=A, mask=mask, sweeps=sweeps, theta=None, agg=None, n_c=0)
        lv["w"] = (four / (three * rho_hat(A, mask))) / np.diag(A)
        levels.append(lv)
        if n <= coarse_size or len(levels) == max_levels:
            break
        used = theta
        fptr, fidx, fval = filtered(ptr, idx, val, used)
        agg, n_c, _ = mis2_aggregate(fptr, fidx)
        if 2 * n_c > n and theta > 0:
            used = 0.0
            fptr, fidx, fval = filtered(ptr, idx, val, used)
            agg, n_c, _ = mis2_aggregate(fptr, fidx)
        if 2 * n_c > n:
            break
        F, Fmask = to_dense(fptr, fidx, fval)
        count = np.bincount(agg, minlength=n_c)
        T = np.zeros((n, n_c), dtype=dtype)
        T[np.arange(n), agg] = dtype(1) / np.sqrt(count[agg].astype(dtype))
        Tmask = T != 0
        omega = four / (three * rho_hat(F, Fmask))
        S = -(omega / np.diag(F))[:, None] * F
        S[np.arange(n), np.arange(n)] += dtype(1)
        P = (S @ T).astype(dtype)
        Pmask = (Fmask.astype(np.float32) @ Tmask.astype(np.float32)) > 0
        Ac = (P.T @ (A @ P)).astype(dtype)
        Acmask = (Pmask.T.astype(np.float32) @ ((mask.astype(np.float32) @ Pmask.astype(np.float32)) > 0).astype(np.float32)) > 0
        lv.update(theta=used, agg=agg, n_c=n_c, P=P, Pmask=Pmask)
        ptr, idx, val = to_csr(Ac, Acmask)
    last = levels[-1]
    if last["n"] <= DENSE_COARSE_MAX:
        last["solver"] = "dense"
        last["inv"] = np.linalg.pinv(last["A"].astype(np.float64), hermitian=True).astype(dtype)
    else:
        last["solver"] = "smoother"
    return levels


def cycle(levels, b, dtype, l=0):
    """One V(sweeps, sweeps) cycle from a zero guess for b of shape (n, p)."""
    dtype = np.dtype(dtype).type
    lv = levels[l]
    A, w, s = lv["A"].astype(dtype), lv["w"].astype(dtype)[:, None], lv["sweeps"]
    b = b.astype(dtype)
    if l == len(levels) - 1:
        if lv["solver"] == "dense":
            return lv["inv"].astype(dtype) @ b
        x = w * b
        for _ in range(2 * s - 1):
            x = x + w * (b - A @ x)
        return x
    P = lv["P"].astype(dtype)
    x = w * b
    for _ in range(s - 1):
        x = x + w * (b - A @ x)
    r = b - A @ x
    x = x + P @ cycle(levels, P.T @ r, dtype, l + 1)
    for _ in range(s):
        x = x + w * (b - A @ x)
    return x


def pcg(matvec, b, precon=None, tol=1e-8, maxiter=1000):
    """Plain preconditioned CG to a relative residual `tol`: (x, iterations)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = r if precon is None else precon(r)
    p = z.copy()
    rz = float(r @ z)
    stop = tol * np.linalg.norm(b)
    for it in range(1, maxiter + 1):
        Ap = matvec(p)
        alpha = rz / float(p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        if np.linalg.norm(r) <= stop:
            return x, it
        z = r if precon is None else precon(r)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, maxiter
