"""Plain numpy reference for the multicolour ordering (csrc/tsgu_hip_color.h, sparse_coloring.py): the sequential greedy colouring,
the permutation, the per-colour sweeps in float64, and the error bounds of a sweep and of a whole application.  No GPU, no oracle
binary.  The triangular-solve pieces come from tests/_trsm_ref.py (`solve64`, `bound`, `ratio`, `emulate`), imported as they are.

The bounds
----------
One sweep over all colours IS a triangular solve with the permuted factor T (the classes only say which rows may be computed
together), so its bound is `_trsm_ref.bound` as it stands: |x − x64| <= M(T)^-1 (γ ∘ |T||x64|), γ_i = (len_i + 4)·u, M(T) the
comparison matrix.  The "scaled" sweep x_i = y_i − (Σ_j u_ij x_j) / d_i is the solve (D + U) x = D y carried out without forming D y:
multiplied by d_i, the computed row reads d_i (1 + δ'')^-1 x_i + Σ_j u_ij (1 + θ_j) x_j = d_i y_i with len_i − 1 products and
additions, one division and one subtraction — the same componentwise backward error on T with an exact right-hand side, hence the
same bound with the reference solve64(T, D y).

A whole application is x = T2^-1 (S · T1^-1 r), S = I, or S = D for Gauss-Seidel.  The first sweep returns y = y64 + e1 with
|e1| <= b1(y64) := bound(T1, y64).  The second sweep is a correct solve with the right-hand side S y it was given, so

    |x − x64| <= |x − T2^-1 S y| + |T2^-1 S e1| <= b2(|T2^-1 S y|) + M(T2)^-1 |S| b1(y64).

To first order b2(|T2^-1 S y|) = b2(x64) (the difference is a product of two error terms).  The bound used is therefore
2 · (b2(x64) + M(T2)^-1 |S| b1(y64)): first order, and doubled for the dropped second-order terms exactly as `_trsm_ref` doubles its
bf16 term.  `comparison_solve` applies M(T)^-1 by the substitution `_trsm_ref.bound` uses.
"""

from __future__ import annotations

import numpy as np

import _factor_ref as FR
import _trsm_ref as TR


# ---- the colouring ---------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def neighbours(ptr, idx):
    """adj[i]: the j != i with (i, j) or (j, i) stored."""
    n = len(ptr) - 1
    adj = [set() for _ in range(n)]
    for i in range(n):
        for j in idx[ptr[i]:ptr[i + 1]]:
            if j != i:
                adj[i].add(int(j))
                adj[int(j)].add(i)
    return adj


def greedy(ptr, idx):
    """The colouring: the nodes in descending key (lowbias32(i), i), each takes the smallest colour no coloured neighbour holds."""
    n = len(ptr) - 1
    adj = neighbours(ptr, idx)
    h = lowbias32(np.arange(n))
    colors = np.full(n, -1, dtype=np.int32)
    for i in sorted(range(n), key=lambda i: (int(h[i]), i), reverse=True):
        taken = {colors[j] for j in adj[i]}
        colors[i] = next(c for c in range(n + 1) if c not in taken)
    return colors


def is_valid(ptr, idx, colors):
    return all(colors[i] >= 0 and all(colors[j] != colors[i] for j in a) for i, a in enumerate(neighbours(ptr, idx)))


def first_clash(ptr, idx, colors, n_colors):
    """0, or 1 + the lowest row whose colour is outside [0, n_colors) or held by a neighbour."""
    for i, a in enumerate(neighbours(ptr, idx)):
        if not 0 <= colors[i] < n_colors or any(colors[j] == colors[i] for j in a):
            return i + 1
    return 0


def max_degree(ptr, idx):
    return max((len(a) for a in neighbours(ptr, idx)), default=0)


# ---- the permutation -------------------------------------------------------------------------------------------------------------
def permutation(colors):
    """(perm new → old ordered by (colour, old index), inverse, offsets of the classes)."""
    colors = np.asarray(colors, dtype=np.int64)
    perm = np.argsort(colors, kind="stable")
    inverse = np.empty_like(perm)
    inverse[perm] = np.arange(len(perm))
    k = int(colors.max()) + 1 if len(colors) else 0
    offsets = np.zeros(k + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(colors, minlength=k))
    return perm, inverse, offsets


def permute_csr(ptr, idx, val, inverse):
    """P·A·Pᵀ as CSR with ascending columns, and the position of each of its entries in A's arrays."""
    n = len(ptr) - 1
    rows = inverse[np.repeat(np.arange(n), np.diff(ptr))]
    cols = inverse[idx]
    order = np.lexsort((cols, rows))
    pptr = np.zeros(n + 1, dtype=np.int64)
    pptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return pptr, cols[order].astype(np.int64), (None if val is None else np.asarray(val)[order]), order


# ---- sweeps ----------------------------------------------------------------------------------------------------------------------
def sweep64(ptr, idx, val, B, offsets, lower, unit=False, scaled=False):
    """One triangular sweep by colour classes in float64: every row of a class is computed from rows of OTHER classes only (asserted),
    all at once.  `scaled`: x_i = b_i − Σ / d_i."""
    n = len(ptr) - 1
    val = np.asarray(val, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64).reshape(n, -1)
    X = np.full_like(B, np.nan)
    k = len(offsets) - 1
    for c in (range(k) if lower else range(k - 1, -1, -1)):
        new = {}
        for i in range(offsets[c], offsets[c + 1]):
            j, a, d = TR._split(ptr, idx, val, i, lower, unit)
            assert not np.any((j >= offsets[c]) & (j < offsets[c + 1])), "two rows of one colour are coupled"
            s = a @ X[j] if len(j) else 0.0
            new[i] = B[i] - s / d if scaled else (B[i] - s) / d
        for i, x in new.items():
            X[i] = x
    return X


def comparison_solve(ptr, idx, val, V, lower, unit):
    """M(T)^-1 V for V >= 0: the substitution with |diagonal| and −|off-diagonal|."""
    n = len(ptr) - 1
    absv = np.abs(np.asarray(val, dtype=np.float64))
    Y = np.zeros_like(np.asarray(V, dtype=np.float64).reshape(n, -1))
    V = np.asarray(V, dtype=np.float64).reshape(n, -1)
    for i in TR._rows(n, lower):
        j, a, d = TR._split(ptr, idx, absv, i, lower, unit)
        Y[i] = (V[i] + (a @ Y[j] if len(j) else 0.0)) / d
    return Y


def diagonal(ptr, idx, val):
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    d = np.zeros(n)
    d[rows[idx == rows]] = np.asarray(val, dtype=np.float64)[idx == rows]
    return d


class Stage:
    """One sweep of an application: the CSR arrays of the matrix whose `lower` (or upper) triangle is solved with, `unit`, and whether
    the right-hand side is scaled by the diagonal first (`scale`: Gauss-Seidel's second sweep)."""

    def __init__(self, ptr, idx, val, lower, unit=False, scale=False):
        self.csr, self.lower, self.unit, self.scale = (ptr, idx, np.asarray(val, dtype=np.float64)), lower, unit, scale

    def rhs(self, Y):
        return diagonal(*self.csr).astype(Y.dtype)[:, None] * Y if self.scale else Y

    def solve(self, B, real=np.float64):
        return TR.solve64(*self.csr, self.rhs(np.asarray(B, dtype=real)), self.lower, self.unit, real=real)

    def bound(self, x64, u):
        return TR.bound(*self.csr, x64, self.lower, self.unit, u)

    def emulate(self, B, dtype, seed):
        real = np.float64 if dtype == "f64" else np.float32
        rhs = (diagonal(*self.csr).astype(real)[:, None] * np.asarray(B, dtype=real)) if self.scale else B
        return TR.emulate(*self.csr, rhs, dtype, seed, lower=self.lower, unit=self.unit)


def application(first: Stage, second: Stage, R, u, real=np.float64):
    """(x64, bound) of x = T2^-1 S T1^-1 R in the numbering of the stages (see the module's docstring).  `real`: the type of the
    reference substitution (np.longdouble for the reference of a float64 kernel, as in `_trsm_ref.Case`)."""
    n = len(first.csr[0]) - 1
    R = np.asarray(R, dtype=np.float64).reshape(n, -1)
    y64 = first.solve(R, real)
    x64 = second.solve(y64, real)
    e1 = first.bound(y64, u)
    s = np.abs(diagonal(*second.csr))[:, None] if second.scale else 1.0
    bnd = second.bound(x64, u) + comparison_solve(*second.csr, s * e1, second.lower, second.unit)
    return x64, 2.0 * bnd


def emulate_application(first: Stage, second: Stage, R, dtype, seed):
    return second.emulate(first.emulate(R, dtype, seed), dtype, seed + 1)


def stages(kind, pptr, pidx, pval, transpose=False):
    """The two stages of an application object in the permuted numbering.  `pval`: for "ilu0" the combined L \\ U array, for "ic0" the
    values of L on tril of the pattern (see `FR.lower_csr`), for "sgs" the permuted matrix itself."""
    if kind == "ic0":
        lp, li, _, _ = FR.lower_csr(pptr, pidx)
        L = (lp, li, np.asarray(pval, dtype=np.float64))
        return Stage(*L, lower=True), Stage(*TR.transpose_csr(*L), lower=False)
    M = (pptr, pidx, np.asarray(pval, dtype=np.float64))
    if transpose:
        M = TR.transpose_csr(*M)
    if kind == "sgs":
        return Stage(*M, lower=True), Stage(*M, lower=False, scale=True)
    if transpose:          # (L·U)ᵀ = Uᵀ·Lᵀ: Uᵀ is the lower triangle of the transposed array, Lᵀ its unit upper triangle
        return Stage(*M, lower=True), Stage(*M, lower=False, unit=True)
    return Stage(*M, lower=True, unit=True), Stage(*M, lower=False)


# ---- the patterns of the colouring tests --------------------------------------------------------------------------------------------
def _from_rows(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, (np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if ptr[-1] else np.zeros(0, np.int64))


def stencil27_periodic(m):
    g = np.arange(m)
    x, y, z = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    rows = []
    for i in range(m ** 3):
        cols = {(((x[i] + dx) % m) * m + (y[i] + dy) % m) * m + (z[i] + dz) % m for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)}
        rows.append(sorted(cols))
    return _from_rows(rows)


def one_sided(n, seed):
    """Upper bidiagonal plus random entries stored on one side only: colouring by A's rows alone would be wrong on it."""
    rng = np.random.default_rng(seed)
    rows = [{i, i + 1} if i + 1 < n else {i} for i in range(n)]
    for _ in range(2 * n):
        i, j = rng.integers(0, n, 2)
        if i != j and int(i) not in rows[int(j)]:
            rows[int(i)].add(int(j))
    return _from_rows([sorted(r) for r in rows])


def star(n):
    """A hub row of n − 1 entries (no diagonal), and leaves that store their edge to the hub and their diagonal."""
    return _from_rows([list(range(1, n))] + [[0, i] for i in range(1, n)])


def random_rows(n, per_row, seed):
    rng = np.random.default_rng(seed)
    return _from_rows([sorted(set(rng.integers(0, n, per_row).tolist()) | {i}) for i in range(n)])


PATTERNS = {
    "n1": lambda: _from_rows([[0]]),
    "n2_coupled": lambda: _from_rows([[0, 1], [0, 1]]),
    "diag65": lambda: _from_rows([[i] for i in range(65)]),
    "path257": lambda: FR.band(257, 1),
    "stencil7_5x4x3": lambda: FR.stencil(5, 4, 3, 7),
    "stencil27_4_periodic": lambda: stencil27_periodic(4),
    "one_sided300": lambda: one_sided(300, 3),
    "star300": lambda: star(300),
    "complete70": lambda: FR.from_dense_mask(np.ones((70, 70), dtype=bool)),
    "random1031": lambda: random_rows(1031, 8, 5),
}

_CACHE = {}


def case(name):
    """(ptr, idx, colours of the reference) of a named pattern, computed once."""
    if name not in _CACHE:
        ptr, idx = PATTERNS[name]()
        colors = greedy(ptr, idx)
        colors.setflags(write=False)
        _CACHE[name] = (ptr, idx, colors)
    return _CACHE[name]


# ---- the matrices of the application tests --------------------------------------------------------------------------------------------
def lattice7(nx, ny, nz, coef=(1.0, 1.0, 1.0)):
    """The 7-point operator −∇·(c ∇) on an nx × ny × nz lattice (Dirichlet): (ptr, idx, val), coefficient coef[k] along axis k."""
    ptr, idx = FR.stencil(nx, ny, nz, 7)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    d = np.abs(idx - rows)
    val = np.where(d == 0, 2.0 * sum(coef), np.where(d == 1, -coef[2], np.where(d == nz, -coef[1], -coef[0])))
    return ptr, idx, val.astype(np.float64)


PROBLEMS = {
    "lap7_6x5x4": lambda: (*FR.stencil(6, 5, 4, 7), True),
    "lap27_4x4x4": lambda: (*FR.stencil(4, 4, 4, 27), True),
    "convdiff7_5x4x3": lambda: (*FR.stencil(5, 4, 3, 7), False),
}

# (object, problem) of the application tests: IC(0) on the symmetric problems only
APPLICATIONS = [(kind, name) for kind in ("ilu0", "ic0", "sgs") for name in PROBLEMS if kind != "ic0" or name != "convdiff7_5x4x3"]


def problem(name, seed=11):
    """(ptr, idx, val float64, symmetric) of a named diagonally dominant test matrix."""
    ptr, idx, sym = PROBLEMS[name]()
    return ptr, idx, FR.dominant_values(ptr, idx, seed, symmetric=sym), sym


def trsm_matrix(n, seed):
    """A matrix with a symmetric pattern whose lower triangle is `_trsm_ref.pattern(n, seed)` (row lengths from `_trsm_ref.LENS`,
    deep chains) and whose strict upper triangle mirrors it with values damped by the column's count, so that both triangles stay
    well conditioned: (ptr, idx, val) with ascending columns."""
    ptr, idx, val = TR.pattern(n, seed)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    off = idx != rows
    count = np.bincount(idx[off], minlength=n)
    r = np.concatenate((rows, idx[off]))
    c = np.concatenate((idx, rows[off]))
    v = np.concatenate((val, val[off] / (1.0 + count[idx[off]])))
    order = np.lexsort((c, r))
    out = np.zeros(n + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.bincount(r, minlength=n))
    return out, c[order].astype(np.int64), v[order]


def sweep_arrays(pptr, pidx):
    """(begin, end) of the lower and of the upper sweep and the diagonal positions of a CSR pattern with ascending columns."""
    diag = FR.diag_positions(pptr, pidx)
    return (pptr[:-1].copy(), diag.copy()), (diag + 1, pptr[1:].copy()), diag


def cg_iterations(Mat, b, precon, tol=1e-4, cap=500):
    """Iterations of textbook preconditioned CG to a relative residual `tol` in the operands' dtype."""
    import torch

    x = torch.zeros_like(b)
    r = b.clone()
    z = precon(r) if precon is not None else r
    p = z.clone()
    rz = torch.dot(r, z)
    target = tol * float(torch.linalg.norm(b))
    for it in range(1, cap + 1):
        Ap = Mat @ p
        alpha = rz / torch.dot(p, Ap)
        x += alpha * p
        r -= alpha * Ap
        if float(torch.linalg.norm(r)) <= target:
            return it
        z = precon(r) if precon is not None else r
        rz, old = torch.dot(r, z), rz
        p = z + (rz / old) * p
    return cap
