"""The GMRES kernels (csrc/gmres.hip), one launch at a time, against their mirror (tests/_gmres_ref.py, the functions the float64
solve of the public tests is chained from), with every buffer between 64-element sentinel guards: an out-of-range write fails an
assertion instead of faulting.

Shapes come from tsgu_gmres_geometry (R = rows per workgroup, G = the basis group): n in {1, R - 1, R, R + 1, 3 R + 2},
p in {1, 3, 4, 5, 64, 65, 256} (scalar and wide lanes, idle threads, a 64-column window boundary, the widest scalar width),
k in {1, 2, G - 1, G, G + 1, 2 G + 1, cap + 1}; the largest n and k run only at p in {1, 5, 65, 256}.  The scalar kernel is fed
1, 3, 5, 64 and (at those four widths) 1025 partial rows: 1025 takes the fold to 256 rows first.

Bounds are carried by `Tr` (derived; u = 2^-24 or 2^-53, gamma_m = m u / (1 - m u)): a projection entry is a sum of min(R, n)
products formed inside fmas, in any order; a folded h, beta or hn a sum of n_partial terms; subtract and update one fma per basis
vector; scale one division and one multiplication; rotations, g, the estimate and y the contract's operations, one rounding each
(the build has no relaxing flags: division and square root are correctly rounded).  The mirror works in numpy.longdouble for fp64
kernels; where the host has no wider type every bound is doubled (`mirror_slack`).  Decisions are kept away from their thresholds
by the data: estimates of order one against thresholds of 2^-20 or 2^10, sums that are exactly zero or of order one.  abstol and
reltol are exact in fp32.

Exact assertions: guards, a column whose cycle has ended (zero V_{j+1}, untouched state), every entry a no-op once its stop word is
set, the counters and both sides of each stop rule (estimate <= threshold, a constructed hn = 0, iters_c reaching maxiter or one
short of it; beta <= threshold, a finished column, the threshold written on the first cycle only), zero y rows past steps_c and for
finished columns, repeatability bit for bit.
"""

import numpy as np
import pytest
import torch

import _gmres_ref as GR
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD, SENT = 64, -777.25
WIDTHS = [1, 3, 4, 5, 64, 65, 256]
EDGE_WIDTHS = (1, 5, 65, 256)
DTYPES = [torch.float32, torch.float64]
ABSTOL, RELTOL = 2.0 ** -30, 2.0 ** -12


class Buf:
    """A device array between two runs of sentinels (16-byte aligned: GUARD elements are a multiple of 16 bytes)."""

    def __init__(self, a, td):
        a = np.ascontiguousarray(a)
        self.shape, self.n = a.shape, a.size
        self.sent = SENT if td.is_floating_point else -123456
        self.flat = torch.full((self.n + 2 * GUARD,), self.sent, dtype=td, device=DEV)
        self.t = self.flat[GUARD:GUARD + self.n]
        self.t.copy_(torch.from_numpy(a.reshape(-1)).to(td))

    def get(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def ok(self):
        return bool((self.flat[:GUARD] == self.sent).all() & (self.flat[GUARD + self.n:] == self.sent).all())


class Ctx:
    def __init__(self, td):
        self.td = td
        self.nd = np.float32 if td == torch.float32 else np.float64
        self.u = 2.0 ** -24 if td == torch.float32 else 2.0 ** -53
        self.W, self.slack = GR.work_dtype(self.nd), GR.mirror_slack(self.nd)
        self.vt = _backend.vtype_of(torch.empty(0, dtype=td))

    def T(self, a):
        return GR.Tr(np.asarray(a).astype(self.W), None, self.u)

    def close(self, what, got, ref):
        assert got.shape == ref.v.shape, (what, got.shape, ref.v.shape)
        err = np.abs(got.astype(self.W) - ref.v).astype(np.float64)
        bound = ref.e * self.slack
        assert np.isfinite(bound).all(), f"{what}: an element without a finite bound"
        exact = bound == 0
        assert np.array_equal(got[exact].astype(self.W), ref.v[exact]), f"{what} differs where it is determined exactly"
        bad = err > bound
        assert not bad.any(), f"{what}: max |err| / bound = {(err[bad] / bound[bad]).max():.3f}"


def _launch(name, *args):
    _backend.launch(name, DEV, *[a.t if isinstance(a, Buf) else a for a in args])


def _flags(p, stop=0, idle=0, cycles=0, fin=None, ended=None, steps=None, iters=None):
    f = np.zeros(4 + 4 * p, dtype=np.int32)
    f[0], f[1], f[2] = stop, idle, cycles
    for i, a in enumerate((fin, ended, steps, iters)):
        if a is not None:
            f[4 + i * p:4 + (i + 1) * p] = a
    return f


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_streaming_kernels(td, p):
    ctx = Ctx(td)
    nd, vt = ctx.nd, ctx.vt
    rng = np.random.default_rng(100 + p)
    cap, G, R, _ = _backend.gmres_geometry(td, 1, p)
    assert cap >= 64 and G >= 2
    edge = p in EDGE_WIDTHS
    rows = sorted({1, max(R - 1, 1), R, R + 1} | ({3 * R + 2} if edge else set()))
    counts = sorted({1, 2, G - 1, G, G + 1} | ({2 * G + 1, cap + 1} if edge else set()))
    for n in rows:
        nb = _backend.gmres_geometry(td, n, p)[3]
        assert nb == -(-n // R)
        slab = -(-n * p // 4) * 4
        for k in counts:
            w = rng.standard_normal((n, p)).astype(nd)
            Vh = np.zeros((k, slab), dtype=nd)
            Vh[:, :n * p] = rng.standard_normal((k, n * p)).astype(nd)
            V3 = Vh[:, :n * p].reshape(k, n, p)
            coef = rng.standard_normal((k, p)).astype(nd)
            ended = (rng.random(p) < 0.3).astype(np.int32)
            steps = rng.integers(0, k + 1, size=p).astype(np.int32)
            hnorm = (0.5 + np.abs(rng.standard_normal(p))).astype(nd)
            hnorm[ended != 0] = 0.0                                     # never read for a column whose cycle has ended
            fl = _flags(p, ended=ended, steps=steps)
            dw, dV, dc, dh = Buf(w, td), Buf(Vh, td), Buf(coef, td), Buf(hnorm, td)
            flags = Buf(fl, torch.int32)
            part, part2 = Buf(np.zeros((nb, k + 1, p)), td), Buf(np.zeros((nb, p)), td)
            out, vnext = Buf(np.zeros((n, p)), td), Buf(np.zeros((n, p)), td)
            x0 = rng.standard_normal((n, p)).astype(nd)
            dx = Buf(x0, td)
            _launch("tsgu_gmres_project", vt, n, p, k, dw, dV, slab, part, flags, 1)
            _launch("tsgu_gmres_subtract", vt, n, p, k, dw, dV, slab, dc, out, part2, flags, 1)
            _launch("tsgu_gmres_scale", vt, n, p, dw, dh, vnext, flags, 1)
            _launch("tsgu_gmres_update", vt, n, p, k, dx, dV, slab, dc, flags)
            torch.cuda.synchronize()
            bufs = (dw, dV, dc, dh, flags, part, part2, out, vnext, dx)
            assert all(b.ok() for b in bufs), f"a kernel wrote outside its buffer (n={n}, p={p}, k={k})"
            assert np.array_equal(dw.get(), w) and np.array_equal(dV.get(), Vh), "inputs are not written"
            tag = f"n={n} p={p} k={k} {td}"
            Tw, TV, Tc = ctx.T(w), [ctx.T(V3[i]) for i in range(k)], [ctx.T(coef[i]) for i in range(k)]
            ctx.close("project " + tag, part.get(), GR.project(Tw, TV, k, R, fl))
            ref_out, ref_part = GR.subtract(Tw, TV, Tc, k, R, fl)
            ctx.close("subtract " + tag, out.get(), ref_out)
            ctx.close("subtract partial " + tag, part2.get(), ref_part)
            gv = vnext.get()
            assert not gv[:, ended != 0].any(), "a column whose cycle has ended gets a zero basis vector"
            ctx.close("scale " + tag, gv, GR.scale(Tw, ctx.T(hnorm), fl))
            gx = dx.get()
            ctx.close("update " + tag, gx, GR.update(ctx.T(x0), TV, Tc, k, fl))
            assert np.array_equal(gx[:, steps == 0], x0[:, steps == 0]), "a column without steps keeps its bits"
            part_b = Buf(np.zeros((nb, k + 1, p)), td)
            _launch("tsgu_gmres_project", vt, n, p, k, dw, dV, slab, part_b, flags, 1)
            assert _same_bits(part_b.get(), part.get()), "the same launch twice gives the same bits"
            for stop, idle, inner in ((1, 0, 0), (0, 1, 1)):
                f2 = _flags(p, stop=stop, idle=idle, steps=steps)
                assert GR.project(Tw, TV, k, R, f2, inner) is None and GR.scale(Tw, ctx.T(hnorm), f2, inner) is None
                d2 = Buf(f2, torch.int32)
                keep = Buf(np.full((nb, k + 1, p), 3.5), td)
                keep2, o2, x2 = Buf(np.full((nb, p), 3.5), td), Buf(np.full((n, p), 3.5), td), Buf(x0, td)
                _launch("tsgu_gmres_project", vt, n, p, k, dw, dV, slab, keep, d2, inner)
                _launch("tsgu_gmres_subtract", vt, n, p, k, dw, dV, slab, dc, o2, keep2, d2, inner)
                _launch("tsgu_gmres_scale", vt, n, p, dw, dh, o2, d2, inner)
                if stop:
                    _launch("tsgu_gmres_update", vt, n, p, k, x2, dV, slab, dc, d2)
                torch.cuda.synchronize()
                assert (keep.get() == 3.5).all() and (keep2.get() == 3.5).all() and (o2.get() == 3.5).all() and \
                    np.array_equal(x2.get(), x0), "every entry is a no-op once its stop word is set"
                assert all(b.ok() for b in (d2, keep, keep2, o2, x2))


def _partial_counts(p):
    return [1, 3, 5, 64] + ([1025] if p in EDGE_WIDTHS else [])


def _run_scalar(ctx, phase, j, m, partial, scal0, fl0, maxiter, p, n_partial):
    """Launch one phase twice on fresh copies (repeatability) and compare state and flags with the mirror; returns the mirror's."""
    fold_rows = _backend.load_library().tsgu_cg_fold_rows()
    outs = []
    for _ in range(2):
        scal, flags = Buf(scal0, ctx.td), Buf(fl0, torch.int32)
        dp = Buf(partial, ctx.td) if partial is not None else None
        fold = Buf(np.zeros((fold_rows, m + 1, p)), ctx.td)
        _launch("tsgu_gmres_scalar", ctx.vt, phase, j, m, dp, n_partial, fold, scal, flags, ABSTOL, RELTOL, maxiter, p)
        torch.cuda.synchronize()
        assert all(b.ok() for b in (scal, flags, fold) + ((dp,) if dp is not None else ())), "a kernel wrote outside its buffer"
        outs.append((scal.get(), flags.get()))
    assert _same_bits(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]), "the same launch twice gives the same bits"
    ref_s, ref_f = GR.scalar(phase, j, m, None if partial is None else ctx.T(partial), ctx.T(scal0), fl0, ABSTOL, RELTOL, maxiter)
    tag = f"phase {phase} p={p} rows={n_partial} {ctx.td}"
    assert np.array_equal(outs[0][1], ref_f), f"flags {tag}: {outs[0][1][:4]} vs {ref_f[:4]}"
    ctx.close("scal " + tag, outs[0][0], ref_s)
    return outs[0][0], ref_s, ref_f


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_scalar_h_phases(td, p):
    ctx = Ctx(td)
    rng = np.random.default_rng(7 + p)
    m, j = 6, 3
    L = GR.layout(m)
    for n_partial in _partial_counts(p):
        ended = (rng.random(p) < 0.3).astype(np.int32)
        scal0 = rng.standard_normal((L["rows"], p)).astype(ctx.nd)
        fl0 = _flags(p, cycles=1, ended=ended)
        p1 = rng.standard_normal((n_partial, j + 2, p)).astype(ctx.nd)
        got, _, _ = _run_scalar(ctx, 1, j, m, p1, scal0, fl0, 100, p, n_partial)
        p2 = (rng.standard_normal((n_partial, j + 2, p)) * 1e-3).astype(ctx.nd)
        got2, _, _ = _run_scalar(ctx, 2, j, m, p2, got, fl0, 100, p, n_partial)
        untouched = np.ones(L["rows"], dtype=bool)
        untouched[L["h"]:L["h"] + j + 1] = untouched[L["coef"]:L["coef"] + j + 1] = False
        assert _same_bits(got2[untouched], scal0[untouched]), "the h phases write h and coef only"
        assert _same_bits(got2[:, ended != 0], scal0[:, ended != 0]), "a column whose cycle has ended is untouched"


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_scalar_cycle_start(td, p):
    ctx = Ctx(td)
    rng = np.random.default_rng(21 + p)
    m, maxiter = 5, 40
    L = GR.layout(m)
    for n_partial in _partial_counts(p):
        for shift in range(4):                      # every column passes through every kind
            kind = (np.arange(p) + shift) % 4       # 0 runs on | 1 zero residual | 2 finished before | 3 iters_c = maxiter
            part = (0.5 + rng.random((n_partial, p))).astype(ctx.nd)
            part[:, kind == 1] = 0.0
            scal0 = rng.standard_normal((L["rows"], p)).astype(ctx.nd)
            # first cycle: the threshold is written, finished and iters_c are reset whatever they held
            fl0 = _flags(p, cycles=0, fin=rng.integers(0, 2, p), ended=rng.integers(0, 2, p), steps=rng.integers(0, m, p),
                         iters=rng.integers(0, 9, p))
            got, ref_s, ref_f = _run_scalar(ctx, 0, 0, m, part, scal0, fl0, maxiter, p, n_partial)
            fin = ref_f[4:4 + p]
            assert np.array_equal(fin != 0, kind == 1) and ref_f[2] == 1 and ref_f[0] == ref_f[1] == int((kind == 1).all())
            assert not ref_f[4 + 2 * p:].any() and np.array_equal(ref_f[4 + p:4 + 2 * p], fin)
            assert (got[0, kind == 1] == ctx.nd(ABSTOL)).all(), "a zero column: threshold = abstol, finished at once"
            # a later cycle: the threshold stays, finished columns are untouched, beta on both sides of the threshold, the cut-off
            scal0[0] = np.where(kind == 1, 2.0 ** 10, 2.0 ** -20).astype(ctx.nd)
            part = (0.5 + rng.random((n_partial, p))).astype(ctx.nd)
            fl1 = _flags(p, cycles=3, fin=(kind == 2), ended=rng.integers(0, 2, p), steps=rng.integers(0, m, p),
                         iters=np.where(kind == 3, maxiter, maxiter - 1))
            got, ref_s, ref_f = _run_scalar(ctx, 0, 0, m, part, scal0, fl1, maxiter, p, n_partial)
            assert _same_bits(got[0], scal0[0]), "the threshold is written on the first cycle only"
            assert _same_bits(got[:, kind == 2], scal0[:, kind == 2]), "a finished column is untouched"
            assert np.array_equal(ref_f[4:4 + p] != 0, kind != 0) and ref_f[2] == 4 and ref_f[0] == int((kind != 0).all())
            assert np.array_equal(ref_f[4 + 3 * p:], fl1[4 + 3 * p:]), "a cycle start does not count steps"
            # flags[0] set: nothing moves
            fl2 = fl1.copy()
            fl2[0] = 1
            s2, f2 = Buf(scal0, td), Buf(fl2, torch.int32)
            _launch("tsgu_gmres_scalar", ctx.vt, 0, 0, m, Buf(part, td), n_partial, None, s2, f2, ABSTOL, RELTOL, maxiter, p)
            torch.cuda.synchronize()
            assert _same_bits(s2.get(), scal0) and np.array_equal(f2.get(), fl2) and s2.ok() and f2.ok()


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_scalar_rotations_and_stop_rules(td, p):
    ctx = Ctx(td)
    rng = np.random.default_rng(33 + p)
    m, maxiter = 6, 50
    L = GR.layout(m)
    for n_partial in _partial_counts(p):
        for j in ((0, 3, m - 1) if n_partial == 3 else (3,)):
            for shift in range(6):
                # 0 runs on | 1 estimate <= threshold | 2 hn = 0 | 3 iters_c reaches maxiter | 4 cycle ended before | 5 one short of maxiter
                kind = (np.arange(p) + shift) % 6
                scal0 = rng.standard_normal((L["rows"], p)).astype(ctx.nd)
                ang = rng.uniform(0.3, 1.2, (m, p))
                scal0[L["cs"]:L["cs"] + m], scal0[L["sn"]:L["sn"] + m] = np.cos(ang).astype(ctx.nd), np.sin(ang).astype(ctx.nd)
                scal0[L["g"]:L["g"] + m + 1] = (1.0 + rng.random((m + 1, p))).astype(ctx.nd)
                scal0[L["h"]:L["h"] + m] = (1.0 + rng.random((m, p))).astype(ctx.nd)        # positive h and angles in the first
                scal0[0] = np.where(kind == 1, 2.0 ** 10, 2.0 ** -20).astype(ctx.nd)       # quadrant: h_j stays away from zero
                part = (0.5 + rng.random((n_partial, p))).astype(ctx.nd) / n_partial
                part[:, kind == 2] = 0.0
                iters = np.where(kind == 3, maxiter - 1, np.where(kind == 5, maxiter - 2, 7))
                fl0 = _flags(p, cycles=2, ended=(kind == 4), steps=np.full(p, j), iters=iters)
                got, ref_s, ref_f = _run_scalar(ctx, 3, j, m, part, scal0, fl0, maxiter, p, n_partial)
                live = kind != 4
                assert _same_bits(got[:, ~live], scal0[:, ~live]), "a column whose cycle has ended is untouched"
                assert (got[2, kind == 2] == 0).all() and (got[L["sn"] + j, kind == 2] == 0).all(), "hn = 0: sn_j = 0, hnorm = 0"
                assert (np.abs(got[1, live & (kind != 2)]) > 2.0 ** -6).all(), "estimates of order one"
                ended = ref_f[4 + p:4 + 2 * p] != 0
                assert np.array_equal(ended, np.isin(kind, (1, 2, 3, 4))), "both sides of each stop rule"
                assert np.array_equal(ref_f[4 + 2 * p:4 + 3 * p], np.where(live, j + 1, j))
                assert np.array_equal(ref_f[4 + 3 * p:], iters + live)
                assert ref_f[3] == 1 and ref_f[0] == 0 and ref_f[1] == int(ended.all()) and ref_f[2] == 2
                changed = np.zeros(L["rows"], dtype=bool)
                changed[[1, 2, L["cs"] + j, L["sn"] + j, L["g"] + j, L["g"] + j + 1]] = True
                changed[L["h"]:L["h"] + j + 1] = True
                changed[[L["R"] + i * m + j for i in range(j + 1)]] = True
                assert _same_bits(got[~changed], scal0[~changed]), "phase 3 writes column j of R, rotation j, g_j, g_{j+1} and h only"
        fl2 = _flags(p, stop=1, cycles=2, steps=np.full(p, 3))
        s2, f2 = Buf(scal0, td), Buf(fl2, torch.int32)
        _launch("tsgu_gmres_scalar", ctx.vt, 3, 3, m, Buf(part, td), n_partial, None, s2, f2, ABSTOL, RELTOL, maxiter, p)
        torch.cuda.synchronize()
        assert _same_bits(s2.get(), scal0) and np.array_equal(f2.get(), fl2), "a no-op once flags[0] is set"


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_scalar_back_substitution(td, p):
    ctx = Ctx(td)
    rng = np.random.default_rng(55 + p)
    for m in (1, 5, 9):
        L = GR.layout(m)
        scal0 = rng.standard_normal((L["rows"], p)).astype(ctx.nd)
        for i in range(m):                                                  # a well-conditioned triangle: diagonal 2 ... 3
            scal0[L["R"] + i * m + i] = (2.0 + rng.random(p)).astype(ctx.nd) * rng.choice([-1.0, 1.0], p)
        steps = rng.integers(0, m + 1, p)
        steps[rng.integers(0, p)] = m
        fin = (rng.random(p) < 0.25).astype(np.int32)
        zero_diag = (rng.random(p) < 0.2) & (steps > 0)
        scal0[L["R"], zero_diag] = 0.0                                      # R(0, 0) = 0: y_0 = 0, no division
        fl0 = _flags(p, cycles=1, fin=fin, ended=np.ones(p), steps=steps, iters=steps)
        got, ref_s, ref_f = _run_scalar(ctx, 4, 0, m, None, scal0, fl0, 100, p, 0)
        assert np.array_equal(ref_f, fl0), "the cycle end moves no flag"
        y = got[L["y"]:L["y"] + m]
        st = np.where(fin != 0, 0, steps)
        assert not y[np.arange(m)[:, None] >= st[None, :]].any(), "zero rows past steps_c and for finished columns"
        assert not y[0, zero_diag & (fin == 0)].any()
        other = np.ones(L["rows"], dtype=bool)
        other[L["y"]:L["y"] + m] = False
        assert _same_bits(got[other], scal0[other]), "phase 4 writes y only"
        fl2 = fl0.copy()
        fl2[0] = 1
        s2, f2 = Buf(scal0, td), Buf(fl2, torch.int32)
        _launch("tsgu_gmres_scalar", ctx.vt, 4, 0, m, None, 0, None, s2, f2, ABSTOL, RELTOL, 100, p)
        torch.cuda.synchronize()
        assert _same_bits(s2.get(), scal0) and np.array_equal(f2.get(), fl2), "a no-op once flags[0] is set"
