"""High-precision mirror of the Krylov step entry points (K5 CG, K6 BiCGSTAB, K7 MINRES, column dots of include/tsgu_hip.h).

One function per entry point, written from the contracts in the header and the reference lines they cite
(torchsparsegradutils/utils/linear_cg.py:27-95, :372-382; bicgstab.py:163-241; minres.py:259-305) — not from the kernels.  A
function takes the state of a step (scal, flags, partial rows, vectors) as arrays holding the exactly rounded inputs and returns
the state after the step.

Every value is a `Tr`: the value in a working type wider than the kernel's (float64 for fp32 kernels, numpy.longdouble for
fp64 kernels, see `work_dtype`) next to a running bound of |kernel value - mirror value| for a kernel that performs the same
operations in a type with unit roundoff `u`, in any association of the sums:
    a op b      error of the operands propagated, plus one rounding  u * |result|, division and square root included: the
                library is built without any flag that relaxes them (csrc/Makefile: -O3 -ffp-contract=off only), and then the
                compiler's fp32 division and square root are correctly rounded and the fp64 ones are IEEE
    fma(a,b,c)  one rounding for the product and the sum together
    sum of m terms, any order:  gamma_m * sum |terms|,  gamma_m = m u / (1 - m u)   (Higham, Accuracy and Stability, 4.4)
The mirror's own roundings are in the bound too, with the working type's unit roundoff um (2^-53 or 2^-64): um |result| per
operation, um |a b| for a product inside an fma (the mirror does not fuse), gamma_m(um) sum|terms| per sum.  Against an fp32
kernel that is nothing; against an fp64 kernel it is a 2048th of the kernel's share, except where a result cancels to less than
a 2048th of its terms — among 10^5 random elements some do — and there the bound would otherwise ask the mirror for digits it
does not have.
With u = 0 the values are those of plain arithmetic in the working type: that is how the CPU tests chain the steps into solves.

Decisions (safe divisions, has_converged, stop rules, finished flags) are taken on the mirror's values; the caller keeps its
data away from the thresholds.  Partial rows: block b of a vector step sums the rows [b R, (b + 1) R) of the array, R = rows per
workgroup — the count the size queries tsgu_cg_num_blocks / tsgu_cg2_num_blocks answer with; the caller passes R.
"""

import numpy as np

kDivSqrt = 1.0      # roundings charged to a division or a square root
LONG_OK = np.finfo(np.longdouble).nmant >= 63      # an 80-bit long double: 2^-64 against the 2^-53 of an fp64 kernel


def work_dtype(dtype):
    """Working type of the mirror for kernels of `dtype` (a numpy dtype)."""
    return np.longdouble if np.dtype(dtype) == np.float64 and LONG_OK else np.float64


def mirror_slack(dtype):
    """Factor on every bound: 2 where the mirror is no more accurate than the kernel (fp64 kernels without a wider host type)."""
    return 2.0 if np.dtype(dtype) == np.float64 and not LONG_OK else 1.0


def gamma(m, u):
    return m * u / (1.0 - m * u) if u else 0.0


class Tr:
    """value `v` (working type) and bound `e` (float64) of the kernel's deviation from it; `u` the kernel's unit roundoff."""

    __slots__ = ("v", "e", "u")
    __array_ufunc__ = None      # numpy scalars and arrays defer to the reflected operators below

    def __init__(self, v, e=None, u=0.0):
        self.v = np.asarray(v)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)
        self.u = u

    def _co(self, o):
        return o if isinstance(o, Tr) else Tr(np.asarray(o, dtype=self.v.dtype), None, self.u)

    @property
    def um(self):
        return float(np.finfo(self.v.dtype).eps) / 2

    def _round(self, v, e, k=1.0):
        a = np.abs(v).astype(np.float64)
        with np.errstate(invalid="ignore"):        # (a discarded lane may carry inf or NaN)
            return Tr(v, e + k * self.u * (a + e) + k * self.um * a, self.u)

    def __neg__(self):
        return Tr(-self.v, self.e, self.u)

    def __add__(self, o):
        o = self._co(o)
        return self._round(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._co(o)
        return self._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return self._co(o) - self

    def _mul_exact(self, o):
        """The product as the kernel forms it inside an fma: no rounding of the kernel's, one of the mirror's."""
        a, b = np.abs(self.v).astype(np.float64), np.abs(o.v).astype(np.float64)
        return self.v * o.v, a * o.e + b * self.e + self.e * o.e + self.um * a * b

    def __mul__(self, o):
        o = self._co(o)
        return self._round(*self._mul_exact(o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._co(o)
        a, b = np.abs(self.v).astype(np.float64), np.abs(o.v).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = self.v / o.v
            lo = b - o.e
            # |a'/b' - a/b| <= (ea + |a/b| eb) / (|b| - eb), written without the difference of two nearly equal quotients
            e = np.where(lo > 0, (self.e + np.abs(v).astype(np.float64) * o.e) / np.where(lo > 0, lo, 1.0), np.inf)
        return self._round(v, np.where(np.isfinite(e), e, np.inf), kDivSqrt)

    def __rtruediv__(self, o):
        return self._co(o) / self

    def sqrt(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            v = np.sqrt(self.v)
            a = np.abs(self.v).astype(np.float64)
            # |sqrt(s + d) - sqrt(s)| = |d| / (sqrt(s + d) + sqrt(s)) <= |d| / sqrt(s);  a sum that may be 0: sqrt(|d|)
            e = np.where(a > 0, np.minimum(self.e / np.sqrt(np.where(a > 0, a, 1.0)), np.sqrt(self.e)), np.sqrt(self.e))
        return self._round(v, e, kDivSqrt)

    def __getitem__(self, k):
        return Tr(self.v[k], self.e[k], self.u)

    @property
    def shape(self):
        return self.v.shape


def fma(a, b, c):
    """a * b + c with one rounding."""
    a = a if isinstance(a, Tr) else c._co(a)
    b = a._co(b)
    c = a._co(c)
    v, e = a._mul_exact(b)
    return a._round(v + c.v, e + c.e)


def where(cond, a, b, like=None):
    like = like if like is not None else (a if isinstance(a, Tr) else b)
    a, b = like._co(a), like._co(b)
    return Tr(np.where(cond, a.v, b.v), np.where(cond, a.e, b.e), like.u)


def exact(x, dtype, u=0.0):
    """Exactly known inputs (already rounded to the kernel's type) as a Tr in the working type of `dtype`."""
    return x if isinstance(x, Tr) else Tr(np.asarray(x).astype(work_dtype(dtype)), None, u)


def colsum(t, m_extra=0):
    """Sum over axis 0 of m rows in any order (with m_extra more terms' worth of additions, for multi-stage sums)."""
    m = t.v.shape[0] + m_extra
    a = np.abs(t.v).astype(np.float64)
    return Tr(t.v.sum(axis=0), t.e.sum(axis=0) + (gamma(m, t.u) + gamma(m, t.um)) * (a + t.e).sum(axis=0), t.u)


def block_sums(t, R, blocks=None):
    """Partial rows of a vector step: row b = sum of the rows [b R, (b + 1) R) of t ([n][p]), any order within the block."""
    n, p = t.v.shape
    nb = -(-n // R) if blocks is None else blocks
    pad = nb * R - n
    v = np.concatenate([t.v, np.zeros((pad, p), dtype=t.v.dtype)]).reshape(nb, R, p)
    e = np.concatenate([t.e, np.zeros((pad, p))]).reshape(nb, R, p)
    a = np.abs(v).astype(np.float64)
    m = min(R, n)
    return Tr(v.sum(axis=1), e.sum(axis=1) + (gamma(m, t.u) + gamma(m, t.um)) * (a + e).sum(axis=1), t.u)


def _ints(flags):
    return np.array(flags, dtype=np.int64).copy()


# ---- column dots -----------------------------------------------------------------------------------------------------------

def coldot(X, Y):
    """out[c] = sum_i X[i, c] Y[i, c]; the products are formed by fma into running sums: n terms, one rounding each."""
    prod = Tr(*X._mul_exact(Y), X.u)
    return colsum(prod, m_extra=1)


# ---- K5: CG, four steps ----------------------------------------------------------------------------------------------------
# scal [4][p]: rr | alpha | beta | rnorm;  flags: [0] done, [1] iterations, [2..2+p) has_converged, [2+p..2+2p) rhs_is_zero

def _safe_div(num, den, eps):
    """The reference's safe division (linear_cg.py:35-43, :67-71): 0 where the divisor is below eps."""
    small = den.v < eps
    q = num / where(small, 1.0, den)
    return where(small, 0.0, q)


def cg_alpha(pap_partial, scal, flags, eps, p):
    """step 1: alpha = safe(rr / sum pAp partials), 0 for converged columns.  Returns scal."""
    flags = _ints(flags)
    if flags[0] != 0:
        return scal
    pap = colsum(pap_partial)
    alpha = _safe_div(scal[0], pap, eps)
    alpha = where(flags[2:2 + p] != 0, 0.0, alpha)
    return _set_rows(scal, {1: alpha})


def _set_rows(scal, rows):
    v, e = scal.v.copy(), scal.e.copy()
    for k, t in rows.items():
        v[k], e[k] = t.v, t.e
    return Tr(v, e, scal.u)


def cg_update1(r, Ap, x, pvec, scal, flags, R):
    """step 2: r -= alpha Ap; x += alpha p; |r|^2 partial rows.  Returns (r, x, rr_partial) — None once done."""
    if _ints(flags)[0] != 0:
        return None
    alpha = scal[1]
    r2 = fma(-alpha, Ap, r)
    x2 = fma(alpha, pvec, x)
    return r2, x2, block_sums(Tr(*r2._mul_exact(r2), r2.u), R)


def cg_update1_alpha(r, Ap, x, pvec, pap_partial, scal, flags, eps, R):
    """steps 1 + 2 in one launch.  Returns (r, x, scal, rr_partial) — None once done."""
    if _ints(flags)[0] != 0:
        return None
    scal = cg_alpha(pap_partial, scal, flags, eps, r.shape[1])
    r2, x2, part = cg_update1(r, Ap, x, pvec, scal, flags, R)
    return r2, x2, scal, part


def cg_beta(rr_partial, scal, flags, eps, stop_after, tolerance, iter_index, min_iter_index, p, rz_partial=None):
    """step 3 (and its preconditioned form: the recurrences on <r, z>, norms and the stop test on |r|^2).  Returns (scal, flags)."""
    flags = _ints(flags)
    if flags[0] != 0:
        return scal, flags
    rr_new = colsum(rr_partial)
    ip_new = rr_new if rz_partial is None else colsum(rz_partial)
    beta = _safe_div(ip_new, scal[0], eps)
    nrm = where(flags[2 + p:2 + 2 * p] != 0, 0.0, rr_new.sqrt())
    flags[2:2 + p] = nrm.v < stop_after
    mean = float(nrm.v.sum() / p)
    it = int(flags[1]) if iter_index < 0 else iter_index
    flags[1] = it + 1
    if it >= min_iter_index and mean < tolerance:
        flags[0] = 1
    return _set_rows(scal, {0: ip_new, 2: beta, 3: nrm}), flags


def cg_update2(r, pvec, scal, flags):
    """step 4: p = r + beta p.  Returns pvec — None once done."""
    if _ints(flags)[0] != 0:
        return None
    return fma(pvec, scal[2], r)


# ---- K5: CG, two launches, state halves by parity -----------------------------------------------------------------------------
# scal2 [5][p]: rr half 0 | rr half 1 | alpha | beta | rnorm
# flags2: [0],[1] done by half, [2] iterations, [3] unused, [4..4+p) has_converged half 0, [4+p..4+2p) half 1, [4+2p..4+3p) rhs_is_zero

def cg2_residual(r, Ap, pap_partial, scal2, flags2, parity, eps, R):
    """alpha from half `parity`; r -= alpha Ap; |r|^2 partial rows of R rows each.  Returns (r, scal2, rr_partial) — None once done."""
    flags2 = _ints(flags2)
    p = r.shape[1]
    if flags2[parity] != 0:
        return None
    pap = colsum(pap_partial)
    alpha = _safe_div(scal2[parity], pap, eps)
    alpha = where(flags2[4 + parity * p:4 + (parity + 1) * p] != 0, 0.0, alpha)
    r2 = fma(-alpha, Ap, r)
    return r2, _set_rows(scal2, {2: alpha}), block_sums(Tr(*r2._mul_exact(r2), r2.u), R)


def cg2_direction(r, pvec, x, rr_partial, scal2, flags2, parity, eps, stop_after, tolerance, min_iter_index, hist, n_hist):
    """beta; x += alpha p; p = r + beta p; rr, rnorm, has_converged, the stop word and the counter into half parity ^ 1; alpha and
    beta of iterations < n_hist into hist [n_hist][2][p].  Returns (pvec, x, scal2, flags2, hist); once done only the flag moves."""
    flags2 = _ints(flags2)
    p = r.shape[1]
    o = parity ^ 1
    if flags2[parity] != 0:
        flags2[o] = 1
        return None, None, scal2, flags2, hist
    rr_new = colsum(rr_partial)
    beta = _safe_div(rr_new, scal2[parity], eps)
    alpha = scal2[2]
    it = int(flags2[2])
    if hist is not None and it < n_hist:
        hv, he = hist.v.copy(), hist.e.copy()
        hv[it, 0], he[it, 0] = alpha.v, alpha.e
        hv[it, 1], he[it, 1] = beta.v, beta.e
        hist = Tr(hv, he, hist.u)
    nrm = where(flags2[4 + 2 * p:4 + 3 * p] != 0, 0.0, rr_new.sqrt())
    flags2[4 + o * p:4 + (o + 1) * p] = nrm.v < stop_after
    mean = float(nrm.v.sum() / p)
    flags2[2] = it + 1
    flags2[o] = 1 if (it >= min_iter_index and mean < tolerance) else 0
    x2 = fma(alpha, pvec, x)
    p2 = fma(pvec, beta, r)
    return p2, x2, _set_rows(scal2, {o: rr_new, 3: beta, 4: nrm}), flags2, hist


# ---- K7: MINRES ----------------------------------------------------------------------------------------------------------------
# scal [S][12][p]: 0 alpha | 1 beta | 2,3 c,s two steps back | 4,5 c,s one step back | 6 scale | 7 sub | 8 subsub | 9 diag |
#                  10 scale of this update | 11 beta of the previous step (rows 0, 1, 11 of block 0 serve every shift)
# flags: [0] stop, [1] iterations

def minres_scalar(phase, partial, scal, flags, eps, tol, shifts, value):
    """phase 0: alpha = value <q, A q> (partial: one set [rows][p]);  phase 1: beta_c = max(sqrt(sum), eps) and the Givens step of every
    shift (minres.py:268-289);  phase 2: stop on mean_s,c sqrt|update|^2 / sqrt|sol|^2 < tol (partial: [2 S][rows][p]; NaN never stops).
    Returns (scal, flags)."""
    flags = _ints(flags)
    if flags[0] != 0:
        return scal, flags
    S, _, p = scal.v.shape
    v, e = scal.v.copy(), scal.e.copy()

    def put(s, k, t):
        v[s, k], e[s, k] = t.v, t.e

    if phase == 0:
        put(0, 0, scal._co(value) * colsum(partial))
    elif phase == 1:
        alpha, beta_p = scal[0][0], scal[0][1]
        beta_c = colsum(partial).sqrt()
        beta_c = where(beta_c.v < eps, eps, beta_c)
        for s in range(S):
            c_pp, s_pp, c_p, s_p, scale_p = (scal[s][k] for k in (2, 3, 4, 5, 6))
            subsub = s_pp * beta_p
            sub = c_pp * beta_p
            alpha_s = alpha + shifts[s]
            diag = alpha_s * c_p - s_p * sub
            sub = sub * c_p + s_p * alpha_s
            radius = (diag * diag + beta_c * beta_c).sqrt()
            c_c = diag / radius
            s_c = beta_c / radius
            diag = diag * c_c + s_c * beta_c
            for k, t in ((2, c_p), (3, s_p), (4, c_c), (5, s_c), (6, -(scale_p * s_c)), (7, sub), (8, subsub), (9, diag),
                         (10, scale_p * c_c)):
                put(s, k, t)
        put(0, 11, beta_c)
        put(0, 1, beta_c)
        flags[1] += 1
    else:
        total = 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            for s in range(S):
                total = total + (colsum(partial[2 * s]).sqrt() / colsum(partial[2 * s + 1]).sqrt()).v.sum()
            if float(total / (p * S)) < tol:
                flags[0] = 1
    return Tr(v, e, scal.u), flags


def minres_lanczos(zpp, zp, prod, scal, flags, value, R):
    """which 0: z_c = (value (A q) - alpha z) - beta_prev z_prev2 over z_prev2; |z_c|^2 partial rows.  Returns (z_c, partial) or None."""
    if _ints(flags)[0] != 0:
        return None
    alpha, beta = scal[0][0], scal[0][11]
    zc = (zp._co(value) * prod - alpha * zp) - beta * zpp
    return zc, block_sums(Tr(*zc._mul_exact(zc), zc.u), R)


def minres_update(zc, qp, wpp, wp, sol, scal, flags, R, with_norms, qc=None):
    """which 1: z_c /= beta_c (and q_c when given); per shift w_c = ((q_p - sub w_p) - subsub w_pp) / diag over w_pp;
    sol += w_c scale; with_norms: |w_c scale|^2 (set 2 s) and |sol|^2 (set 2 s + 1) partial rows.  wpp / wp / sol: [S][n][p].
    Returns (z_c, q_c, w_c, sol, partial [2 S][blocks][p] or None) or None."""
    if _ints(flags)[0] != 0:
        return None
    S = scal.v.shape[0]
    beta = scal[0][1]
    z2 = zc / beta
    q2 = None if qc is None else qc / beta
    ws, xs, parts = [], [], []
    for s in range(S):
        sub, subsub, diag, scale = (scal[s][k] for k in (7, 8, 9, 10))
        wc = ((qp - sub * wp[s]) - subsub * wpp[s]) / diag
        up = wc * scale
        xn = sol[s] + up
        ws.append(wc)
        xs.append(xn)
        if with_norms:
            parts.append(block_sums(Tr(*up._mul_exact(up), up.u), R))
            parts.append(block_sums(Tr(*xn._mul_exact(xn), xn.u), R))
    stack = lambda ts: Tr(np.stack([t.v for t in ts]), np.stack([t.e for t in ts]), zc.u)   # noqa: E731
    return z2, q2, stack(ws), stack(xs), (stack(parts) if with_norms else None)


# ---- K6: BiCGSTAB ----------------------------------------------------------------------------------------------------------------
# scal [8][p]: rho | alpha | omega | rho_next | threshold | beta | resid | resid0
# flags: [0] all finished, [1] iterations, [2..2+p) finished, [2+p..2+2p) finishing after the half step, [2+2p..2+3p) matvecs used

def bicg_scalar(phase, partial, scal, flags, abstol, reltol, matvec_max, nmv0):
    """phase 0 init | 1 beta | 2 alpha | 3 half | 4 omega (partial: 3 sets [3][rows][p]) | 5 end.  Returns (scal, flags).
    (Finished columns may divide by zero on the way; their results are discarded.)"""
    with np.errstate(all="ignore"):
        return _bicg_scalar(phase, partial, scal, flags, abstol, reltol, matvec_max, nmv0)


def _bicg_scalar(phase, partial, scal, flags, abstol, reltol, matvec_max, nmv0):
    flags = _ints(flags)
    p = scal.v.shape[1]
    if phase != 0 and flags[0] != 0:
        return scal, flags
    fin, half, nmv = flags[2:2 + p], flags[2 + p:2 + 2 * p], flags[2 + 2 * p:2 + 3 * p]     # views: written in place
    run = fin == 0
    new = {}
    if phase == 0:
        s0 = colsum(partial)
        r0n = s0.sqrt()
        rel = scal._co(reltol) * r0n
        thr = where(rel.v > abstol, rel, abstol)
        one = Tr(np.ones(p, dtype=scal.v.dtype), None, scal.u)
        new = {0: one, 1: one, 2: one, 3: s0, 4: thr, 6: r0n, 7: r0n}
        nmv[:] = nmv0
        half[:] = 0
        fin[:] = (r0n.v <= thr.v) | (nmv0 >= matvec_max)
    elif phase == 1:
        beta = scal[3] / scal[0] * scal[1] / scal[2]
        new = {5: where(run, beta, scal[5]), 0: where(run, scal[3], scal[0])}
    elif phase == 2:
        nmv[run] += 1
        new = {1: where(run, scal[0] / colsum(partial), scal[1])}
    elif phase == 3:
        rn = colsum(partial).sqrt()
        new = {6: where(run, rn, scal[6])}
        small = run & (rn.v <= scal.v[4])
        out = run & ~small & (nmv >= matvec_max)
        half[small] = 1
        fin[out] = 1
    elif phase == 4:
        act = run & (half == 0)
        nmv[act] += 1
        om = colsum(partial[0]) / colsum(partial[1])
        new = {2: where(act, om, scal[2]), 3: where(act, -om * colsum(partial[2]), scal[3])}
    else:
        hf = run & (half != 0)
        act = run & (half == 0)
        rn = colsum(partial).sqrt()
        new = {6: where(act, rn, scal[6])}
        stop = act & ((rn.v <= scal.v[4]) | (nmv >= matvec_max))
        half[hf] = 0
        fin[hf | stop] = 1
    if phase in (0, 5):
        if phase == 5:
            flags[1] += 1
        flags[0] = int(np.all(fin != 0))
    return _set_rows(scal, new), flags


def _fin(flags, p):
    flags = _ints(flags)
    return flags[2:2 + p] != 0, flags[2 + p:2 + 2 * p] != 0


def bicg_update_p(pv, r, v, scal, flags):
    """which 0: p = (p beta - (beta omega) v) + r, finished columns untouched.  Returns p or None."""
    if _ints(flags)[0] != 0:
        return None
    fin, _ = _fin(flags, pv.shape[1])
    beta = scal[5]
    return where(fin[None, :], pv, (pv * beta - (beta * scal[2]) * v) + r)


def bicg_update_s(s, r, v, scal, flags, R):
    """which 1: s = r - alpha v (finished columns untouched); |s|^2 partial rows.  Returns (s, partial) or None."""
    if _ints(flags)[0] != 0:
        return None
    fin, _ = _fin(flags, s.shape[1])
    s2 = where(fin[None, :], s, r - scal[1] * v)
    return s2, block_sums(Tr(*s2._mul_exact(s2), s2.u), R)


def bicg_dots3(t, s, r0, flags, R):
    """which 2: partial rows of <t, s>, <t, t>, <r0, t>.  Returns [3][blocks][p] or None."""
    if _ints(flags)[0] != 0:
        return None
    ps = [block_sums(Tr(*a._mul_exact(b), a.u), R) for a, b in ((t, s), (t, t), (r0, t))]
    return Tr(np.stack([q.v for q in ps]), np.stack([q.e for q in ps]), t.u)


def bicg_update_x(x, r, s, t, q, scal, flags, R, z=None):
    """which 3 (z = None: z is s, q is p) and tsgu_bicg_update_x_precond: active columns r = s - omega t,
    x = (x + omega z) + alpha q; columns finishing after the half step x += alpha q; |r|^2 partial rows.  Returns (x, r, partial) or None."""
    if _ints(flags)[0] != 0:
        return None
    fin, half = _fin(flags, x.shape[1])
    hf = (~fin & half)[None, :]
    act = (~fin & ~half)[None, :]
    alpha, omega = scal[1], scal[2]
    aq = alpha * q
    xa = (x + omega * (s if z is None else z)) + aq
    x2 = where(hf, x + aq, where(act, xa, x))
    r2 = where(act, s - omega * t, r)
    return x2, r2, block_sums(Tr(*r2._mul_exact(r2), r2.u), R)
