"""High-precision mirror of the GMRES entry points of csrc/tsgu_hip_gmres.h, the whole solve chained from them, and the two small
nonsymmetric test matrices.

One function per entry point, written from the contracts in the header — not from the kernels — on `Tr` of _krylov_ref.py: a value
in a working type wider than the kernel's next to a running bound of |kernel - mirror| for a kernel that performs the contract's
operations with unit roundoff u (one rounding per + - * / sqrt and per fma, gamma_m for a sum of m terms in any order).  A function
takes the state of a step (scal, flags, partial rows, blocks) and returns the state after it; decisions (stop rules, d = 0, hn = 0)
are taken on the mirror's values, so a caller keeps its data away from the thresholds.  `abstol` and `reltol` are taken as the
kernel's type holds them: a caller that checks bounds passes values that are exact in fp32.

With u = 0 the values are plain float64 arithmetic: `solve_column` chains the step functions into a solve, so the step tests and
the public tests share one reference.  It also returns every number a stopping decision compared with the threshold, and
`pick_reltol` chooses a tolerance at which all of them are at least 1 % away from it: there a kernel in fp32 or fp64 decides alike.
"""

import numpy as np

import _krylov_ref as K
from _krylov_ref import Tr, block_sums, colsum, fma, gamma, mirror_slack, where, work_dtype      # noqa: F401

FLAG_WORDS = 4      # flags: [0] stop | [1] every cycle ended | [2] cycles started | [3] inner steps run | finished | ended | steps | iters


def layout(m):
    """First row of every field of `scal` for restart length m, and the row count."""
    return {"threshold": 0, "estimate": 1, "hnorm": 2, "g": 3, "cs": m + 4, "sn": 2 * m + 4, "y": 3 * m + 4, "h": 4 * m + 4,
            "coef": 5 * m + 4, "R": 6 * m + 4, "rows": m * m + 6 * m + 4}


def new_state(m, p, dtype=np.float32, u=0.0):
    return Tr(np.zeros((layout(m)["rows"], p), dtype=work_dtype(dtype)), None, u), np.zeros(FLAG_WORDS + 4 * p, dtype=np.int64)


def _columns(flags, p):
    """Views of the four per-column arrays: finished, cycle ended, steps_c, iters_c."""
    return tuple(flags[FLAG_WORDS + i * p:FLAG_WORDS + (i + 1) * p] for i in range(4))


def _idle(flags, inner):
    f = K._ints(flags)
    return f[0] != 0 or (inner and f[1] != 0)


def _sq(t):
    return Tr(*t._mul_exact(t), t.u)


def _stack(ts, axis, u):
    return Tr(np.stack([t.v for t in ts], axis=axis), np.stack([t.e for t in ts], axis=axis), u)


# ---- the streaming entries (V: a list of k blocks [n][p]; R: rows per workgroup) ------------------------------------------------------

def project(w, V, k, R, flags, inner=1):
    """partial [blocks][k + 1][p]; None once idle."""
    if _idle(flags, inner):
        return None
    rows = [block_sums(Tr(*V[i]._mul_exact(w), w.u), R) for i in range(k)] + [block_sums(_sq(w), R)]
    return _stack(rows, 1, w.u)


def subtract(w, V, coef, k, R, flags, inner=1):
    """(out, partial [blocks][p]): one fma per basis vector in the order i = 0 ... k - 1; None once idle."""
    if _idle(flags, inner):
        return None
    t = w
    for i in range(k):
        t = fma(-coef[i], V[i], t)
    return t, block_sums(_sq(t), R)


def scale(w, hnorm, flags, inner=1):
    """w (1 / hnorm), 0 for a column whose cycle has ended; None once idle."""
    if _idle(flags, inner):
        return None
    p = w.shape[1]
    ended = _columns(K._ints(flags), p)[1] != 0
    inv = 1.0 / where(ended, 1.0, hnorm)
    return where(ended[None, :], 0.0, w * inv)


def update(x, V, y, k, flags):
    """x + sum_{i < min(k, steps_c)} y_i V_i, one fma per basis vector; None once flags[0] is set."""
    f = K._ints(flags)
    if f[0] != 0:
        return None
    steps = np.minimum(_columns(f, x.shape[1])[2], k)
    for i in range(int(steps.max())):
        x = where((i < steps)[None, :], fma(y[i], V[i], x), x)
    return x


# ---- the per-column state ------------------------------------------------------------------------------------------------------------

def scalar(phase, j, m, partial, scal, flags, abstol, reltol, maxiter):
    """One phase of tsgu_gmres_scalar.  Returns (scal, flags); unchanged once flags[0] is set."""
    with np.errstate(all="ignore"):
        return _scalar(phase, j, m, partial, scal, flags, abstol, reltol, maxiter)


def _scalar(phase, j, m, partial, scal, flags, abstol, reltol, maxiter):
    flags = K._ints(flags)
    if flags[0] != 0:
        return scal, flags
    p = scal.v.shape[1]
    L = layout(m)
    fin, ended, steps, iters = _columns(flags, p)
    new = {}
    if phase in (1, 2):
        live = ended == 0
        for i in range(j + 1):
            s = colsum(partial[:, i])
            new[L["coef"] + i] = where(live, s, scal[L["coef"] + i])
            new[L["h"] + i] = where(live, s if phase == 1 else scal[L["h"] + i] + s, scal[L["h"] + i])
    elif phase == 4:
        st = np.where(fin != 0, 0, steps)
        y = {}
        for i in range(m - 1, -1, -1):
            s = scal[L["g"] + i]
            for l in range(i + 1, m):
                s = where(l < st, s - scal[L["R"] + i * m + l] * y[l], s)
            d = scal[L["R"] + i * m + i]
            nz = d.v != 0
            y[i] = where((i < st) & nz, s / where(nz, d, 1.0), 0.0)
            new[L["y"] + i] = y[i]
    elif phase == 0:
        beta = colsum(partial).sqrt()
        if flags[2] == 0:
            rel = scal._co(reltol) * beta
            new[0] = where(rel.v > abstol, rel, abstol)
            fin[:] = 0
            iters[:] = 0
        thr = new.get(0, scal[0])
        live = fin == 0
        for row in (1, 2, L["g"]):
            new[row] = where(live, beta, scal[row])
        fin[live & ((beta.v <= thr.v) | (iters >= maxiter))] = 1
        ended[:] = fin
        steps[:] = 0
        flags[2] += 1
        flags[0] = flags[1] = int(np.all(fin != 0))
    else:
        hn = colsum(partial).sqrt()
        live = ended == 0
        h = [scal[L["h"] + i] for i in range(j + 1)]
        for i in range(j):
            a, b, ci, si = h[i], h[i + 1], scal[L["cs"] + i], scal[L["sn"] + i]
            h[i], h[i + 1] = ci * a + si * b, ci * b - si * a
        hj = h[j]
        den = (hj * hj + hn * hn).sqrt()
        nz = den.v != 0
        safe = where(nz, den, 1.0)
        cj, sj = where(nz, hj / safe, 1.0), where(nz, hn / safe, 0.0)
        h[j] = cj * hj + sj * hn
        gj = scal[L["g"] + j]
        gn = -(sj * gj)
        est = Tr(np.abs(gn.v), gn.e, gn.u)
        rows = {L["h"] + i: h[i] for i in range(j + 1)}
        rows.update({L["R"] + i * m + j: h[i] for i in range(j + 1)})
        rows.update({L["cs"] + j: cj, L["sn"] + j: sj, L["g"] + j + 1: gn, L["g"] + j: cj * gj, 1: est, 2: hn})
        new = {row: where(live, t, scal[row]) for row, t in rows.items()}
        steps[live] = j + 1
        iters[live] += 1
        ended[live & ((est.v <= scal.v[0]) | (hn.v == 0) | (iters >= maxiter))] = 1
        flags[3] += 1
        flags[1] = int(np.all(ended != 0))
    return K._set_rows(scal, new), flags


# ---- the two test matrices -----------------------------------------------------------------------------------------------------------

def convdiff(nx=6, ny=5, nz=4, convection=2.0):
    """7-point diffusion with first-order upwind convection along z on an nx × ny × nz lattice, Dirichlet faces (dense float64)."""
    n = nx * ny * nz
    A = np.zeros((n, n))
    idx = lambda i, j, k: (i * ny + j) * nz + k      # noqa: E731
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                r = idx(i, j, k)
                A[r, r] = 6.0 + convection
                for di, dj, dk, v in ((1, 0, 0, -1.0), (-1, 0, 0, -1.0), (0, 1, 0, -1.0), (0, -1, 0, -1.0), (0, 0, 1, -1.0),
                                      (0, 0, -1, -1.0 - convection)):
                    a, b, c = i + di, j + dj, k + dk
                    if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz:
                        A[r, idx(a, b, c)] = v
    return A


def random_shifted(n=97, density=0.06, shift=2.5, seed=5):
    """A random sparse nonsymmetric matrix plus a diagonal shift (dense float64)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) * (rng.random((n, n)) < density)
    return A + shift * np.eye(n)


# ---- the whole solve: the step functions chained with u = 0 ------------------------------------------------------------------------------

def solve_column(A, b, x0, m, maxiter, abstol, reltol, M=None):
    """GMRES(m) on one column.  Returns (x, inner steps, cycles, decisions): decisions = [(number compared, threshold), ...]."""
    n = b.size
    m = min(m, n)
    L = layout(m)
    T = lambda a: Tr(np.asarray(a, dtype=np.float64).reshape(n, 1), None, 0.0)      # noqa: E731
    scal, flags = new_state(m, 1)
    one = Tr(np.ones((1, 1)), None, 0.0)
    x = T(np.zeros(n) if x0 is None else x0)
    dec = []
    while True:
        r, part = subtract(T(b), [T(A @ x.v[:, 0])], one, 1, n, flags, 0)
        was = int(flags[FLAG_WORDS + 3])
        scal, flags = scalar(0, 0, m, part, scal, flags, abstol, reltol, maxiter)
        dec.append((float(scal.v[1, 0]), float(scal.v[0, 0])))
        if flags[0]:
            return x.v[:, 0].astype(np.float64), was, int(flags[2]) - 1, dec
        V = [scale(r, scal[2], flags, 0)]
        Z = []
        for j in range(m):
            if flags[1]:
                break
            z = V[j] if M is None else T(M @ V[j].v[:, 0])
            Z.append(z)
            w = T(A @ z.v[:, 0])
            for phase in (1, 2):
                scal, flags = scalar(phase, j, m, project(w, V, j + 1, n, flags), scal, flags, abstol, reltol, maxiter)
                w, part = subtract(w, V, [scal[L["coef"] + i] for i in range(j + 1)], j + 1, n, flags)
            scal, flags = scalar(3, j, m, part, scal, flags, abstol, reltol, maxiter)
            dec.append((float(scal.v[1, 0]), float(scal.v[0, 0])))
            V.append(scale(w, scal[2], flags))
        scal, flags = scalar(4, 0, m, None, scal, flags, abstol, reltol, maxiter)
        y = [scal[L["y"] + i] for i in range(m)]
        if M is None:
            x = update(x, V, y, m, flags)
        else:
            u = update(T(np.zeros(n)), V, y, m, flags)
            x = update(x, [T(M @ u.v[:, 0])], one, 1, flags)


def solve(A, B, m, maxiter=None, abstol=1e-8, reltol=1e-6, M=None, X0=None):
    """Column by column.  Returns (X, iterations [p], cycles [p], margin): margin = the least |number / threshold - 1| over every
    decision of every column (zero columns decide 0 <= threshold exactly and are left out)."""
    n, p = B.shape
    maxiter = 2 * n if maxiter is None else maxiter
    X, its, cyc, margin = np.zeros((n, p)), [], [], np.inf
    for c in range(p):
        x, it, cy, dec = solve_column(A, B[:, c], None if X0 is None else X0[:, c], m, maxiter, abstol, reltol, M)
        X[:, c] = x
        its.append(it)
        cyc.append(cy)
        for v, t in dec:
            if v != 0 and t > 0:
                margin = min(margin, abs(v / t - 1.0))
    return X, np.array(its), np.array(cyc), margin


def pick_reltol(A, B, m, candidates=(1e-4, 1.7e-4, 2.9e-4, 4.3e-4, 7.1e-4), abstol=0.0, M=None, maxiter=None):
    """The first tolerance at which every decision of the mirror is at least 1 % away from its threshold."""
    for tol in candidates:
        if solve(A, B, m, maxiter=maxiter, abstol=abstol, reltol=tol, M=M)[3] >= 0.01:
            return tol
    raise AssertionError("no candidate tolerance keeps the mirror's decisions 1 % away from the thresholds")
