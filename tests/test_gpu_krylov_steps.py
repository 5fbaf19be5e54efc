"""The Krylov step kernels (csrc/krylov.hip, minres.hip, bicgstab.hip), one launch at a time, against their high-precision mirror
(tests/_krylov_ref.py), and the solves with 257 ... 1024 right-hand sides end to end.

Every test builds the state of one step with a seeded generator, rounds it to the kernel's type, launches ONE entry point eagerly
and compares every output array with the mirror evaluated on exactly those rounded inputs.  Buffers are sized with the library's
own size queries (tsgu_cg_num_blocks, tsgu_cg2_num_blocks, tsgu_coldot_max_blocks, tsgu_cg_fold_rows) and carry 64 sentinel
elements before and after: an out-of-range write fails an assertion instead of faulting.

Shapes come from the geometry, not from a workload.  An [n][p] array is laid out in lanes of `vec` columns (vec = the 16-byte lane
width, 4 fp32 / 2 fp64 columns, when p is a multiple of it, else 1), lpr = ceil(p / vec) lanes per row, rpp = 256 / lpr rows per
pass, R = 4 rpp rows per workgroup (`_geom`, the arithmetic of vec_geom in csrc/krylov_common.h with kPasses = 4):
  p   1, 2, 3, 4, 5 (scalar and wide lanes, idle threads), 63, 64, 65 (the 64-column windows of the column sums, a ragged last
      window), 127, 128, 129, 192, 255, 256 (lpr not dividing 256; the last width of the one-launch forms), and above 256
      260, 512, 1020, 1024 (fp32) / 258, 512 (fp64): the two-step CG path and finalisers that walk up to 16 windows
  n   1, R - 1, R, R + 1, 3 R + 2
  partial rows fed to the scalar kernels: 1, 3, 4, 5 (the 4-chain unroll), 17, 64, 1024, and 1025, 2051 where a `fold` buffer is
      taken (more than 4 x 256 rows are folded to 256 rows of ceil(rows / 256): 2051 leaves a short last chunk and empty ones).
      Counts up to 64 run at every p; 1024, 1025 and 2051 only at p = 1, 5, 63, 65, 256 and the widths above 256 (one width on
      each side of a window boundary, the narrowest and the widest), to keep the tests to a few seconds
  the two-launch form: sizes whose workgroups take 1, 2 and 3 groups of passes (the unrolled and the generic instances)
Operands offset by one element force scalar lanes in tsgu_coldot (with leading dimensions that are no multiple of the lane width;
above 256 columns that is TSGU_ERR_TOO_LARGE); the other vector entries demand 16-byte alignment and must answer
TSGU_ERR_BAD_ARG.  Widths no geometry covers (257, 1028 in fp32; 259, 514 in fp64) must answer TSGU_ERR_TOO_LARGE.

Bounds (derived, not measured; u = 2^-24 or 2^-53).  The mirror carries them along with its values (`Tr` in _krylov_ref.py):
  * a sum of m terms in whatever order: |s^ - s| <= gamma_m sum|terms|, gamma_m = m u / (1 - m u).  A kernel's partial row sums at
    most R squares or products, each formed inside an fma (no rounding of its own): m = min(R, n).  A scalar kernel sums the
    n_partial rows it is given (two or three stages, any order): m = n_partial.  tsgu_coldot: m = n + 1.
  * a scalar formed from sums: the errors of its inputs propagated through the operations the contract lists, one rounding u per
    + - * / and square root (the library is built without flags that relax division or square root, so the compiler's are
    correctly rounded).  For alpha = rr / pap of positive summands this is the (m + 2) u of the textbook, to first order.
  * a vector output: one rounding per fma of the contract (CG), one per operation where the contract writes separate operations
    (MINRES, BiCGSTAB: the library is built without contraction), plus the propagated error of the per-column scalar it uses
    where the same launch forms that scalar (cg_update1_alpha, cg2_residual, cg2_direction).
  * fp64 kernels: the mirror works in numpy.longdouble (64-bit mantissa) and its own roundings are part of every bound (a 2048th
    of the kernel's, which only shows where a result cancels almost completely); where the host has no wider type every bound
    is doubled instead.
Decisions (safe divisions, has_converged, finished, stop words) are kept away from their thresholds by the data: sums that are
either exactly zero or of order one against thresholds of 1e-3 and below.

Exact assertions (bits or integers): frozen columns, every entry a no-op once its stop word is set, counters and stop rules on
both sides of each condition, hist rows, guard elements, repeatability, and the elementwise outputs of a column not depending on
the width of the array it sits in.
"""

import warnings

import numpy as np
import pytest
import torch

import _golden as G
import _krylov_ref as K
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 64
SENT_F, SENT_I = -777.25, -123456
SMALL = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 192, 255, 256]
WIDE = {torch.float32: [260, 512, 1020, 1024], torch.float64: [258, 512]}
PARTIALS = [1, 3, 4, 5, 17, 64, 1024]
FOLDED = [1025, 2051]
DTYPES = [torch.float32, torch.float64]
EPS, STOP_AFTER = 2.0 ** -33, 2.0 ** -30
BAD_ARG, TOO_LARGE = -2, -3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _backend.load_library()
    yield


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Dev:
    """A device array between two rows of sentinels; `off` elements of misalignment."""

    def __init__(self, a, td, off=0):
        a = np.ascontiguousarray(a)
        self.shape, self.n = a.shape, a.size
        self.sent = SENT_F if td.is_floating_point else SENT_I
        self.flat = torch.full((self.n + 2 * GUARD + off,), self.sent, dtype=td, device=DEV)
        self.lo = GUARD + off
        self.t = self.flat[self.lo:self.lo + self.n]
        self.t.copy_(torch.from_numpy(a.reshape(-1)).to(td))

    def get(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def guards_ok(self):
        f = self.flat
        return bool((f[:self.lo] == self.sent).all() & (f[self.lo + self.n:] == self.sent).all())


class Ctx:
    """Everything that depends on the value type, the device buffers of the running case and the ratios seen."""

    def __init__(self, td):
        self.td = td
        self.nd = np.float32 if td == torch.float32 else np.float64
        self.u = 2.0 ** -24 if td == torch.float32 else 2.0 ** -53
        self.W = K.work_dtype(self.nd)
        self.slack = K.mirror_slack(self.nd)
        self.wide = 16 // np.dtype(self.nd).itemsize
        self.vt = _backend.vtype_of(torch.empty(0, dtype=td))
        self.lib = _backend.load_library()
        self.devs, self.ratios = [], {}

    def r(self, x):
        return float(self.nd(x))

    def T(self, a):
        return K.Tr(np.asarray(a).astype(self.W), None, self.u)

    def rnd(self, rng, shape):
        return rng.standard_normal(shape).astype(self.nd)

    def pos(self, rng, shape):
        return (0.5 + np.abs(rng.standard_normal(shape))).astype(self.nd)

    def dev(self, a, off=0):
        d = Dev(np.asarray(a, dtype=self.nd), self.td, off)
        self.devs.append(d)
        return d

    def ints(self, a):
        d = Dev(np.asarray(a, dtype=np.int32), torch.int32)
        self.devs.append(d)
        return d

    def fin(self):
        torch.cuda.synchronize()
        for d in self.devs:
            assert d.guards_ok(), "a kernel wrote outside its buffer"
        self.devs = []

    def close(self, entry, what, got, ref, before=None):
        """|got - mirror| <= bound elementwise (exactly equal where the bound is 0); `ref` None: the array must keep its bits."""
        if ref is None:
            assert same_bits(got, np.asarray(before, dtype=got.dtype)), f"{entry}: {what} changed although the step is a no-op"
            return
        assert got.shape == ref.v.shape, (entry, what, got.shape, ref.v.shape)
        err = np.abs(got.astype(self.W) - ref.v).astype(np.float64)
        bound = ref.e * self.slack
        zero = bound == 0
        assert np.array_equal(got[zero].astype(self.W), ref.v[zero]), f"{entry}: {what} differs where it is determined exactly"
        # an infinite bound (a divisor within its own error of zero) would exempt an element from the comparison: the data keep
        # every divisor away from zero, and lanes the contract discards carry the bound of the value they keep
        assert np.isfinite(bound).all(), f"{entry}: {what}: {int((~np.isfinite(bound)).sum())} elements without a finite bound"
        live = ~zero
        ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
        self.ratios[entry] = max(self.ratios.get(entry, 0.0), ratio)
        assert ratio <= 1.0, f"{entry}: {what}: max |err| / bound = {ratio:.3f}"

    def report(self):
        for entry, ratio in sorted(self.ratios.items()):
            print(f"[krylov steps] {entry:28s} {str(self.td):14s} max |err| / bound = {ratio:.3f}")
        assert self.ratios, "nothing was compared"


def launch(name, *args):
    _backend.launch(name, DEV, *[a.t if isinstance(a, Dev) else a for a in args])


def status(ctx, name, *args):
    """The status an entry point answers (for the calls that must be refused)."""
    argv = [a.t.data_ptr() if isinstance(a, Dev) else a for a in args]
    return getattr(ctx.lib, name)(*argv, DEV.index, torch.cuda.current_stream(DEV).cuda_stream)


def _geom(p, wide):
    vec = wide if p % wide == 0 else 1
    lpr = -(-p // vec)
    return None if lpr > 256 else (256 // lpr) * 4


def _rows(R):
    return sorted({1, max(R - 1, 1), R, R + 1, 3 * R + 2})


def _widths(td):
    return SMALL + WIDE[td]


def _blocks(ctx, n, p):
    nb = ctx.lib.tsgu_cg_num_blocks(ctx.vt, n, p)
    assert nb == -(-n // _geom(p, ctx.wide)), (n, p, nb)
    return nb


def _cols(p):
    return np.arange(p)


# ---- column dots -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("td", DTYPES)
def test_coldot(td):
    ctx, rng = Ctx(td), np.random.default_rng(1)
    for p in _widths(td):
        R = _geom(p, ctx.wide)
        for n in _rows(R):
            for off, pad in ((0, 0), (1, 3)):
                ld = p + pad
                X, Y = ctx.rnd(rng, (n, ld)), ctx.rnd(rng, (n, ld))
                dx, dy = ctx.dev(X, off), ctx.dev(Y, off)
                if off and p > 256:               # scalar lanes cover 256 columns: refused (wider operands go in slabs, below)
                    assert status(ctx, "tsgu_coldot", ctx.vt, n, p, dx, ld, dy, ld, ctx.dev(np.zeros((1, p))), ctx.dev(np.zeros(p))) == TOO_LARGE
                    ctx.fin()
                    continue
                nb = ctx.lib.tsgu_coldot_max_blocks(n, p) if p <= 256 else _blocks(ctx, n, p)
                part, out = ctx.dev(np.full((nb, p), 0.25)), ctx.dev(np.zeros(p))
                launch("tsgu_coldot", ctx.vt, n, p, dx, ld, dy, ld, part, out)
                ref = K.coldot(ctx.T(X[:, :p]), ctx.T(Y[:, :p]))
                got = out.get()
                ctx.close("tsgu_coldot", f"out p={p} n={n} off={off}", got, ref)
                assert same_bits(dx.get(), X) and same_bits(dy.get(), Y)
                ctx.fin()
                if off == 0:
                    # the binding: the same bits as the launcher up to 256 columns, slabs of 256 above
                    via = _backend.coldot(torch.from_numpy(X[:, :p].copy()).to(DEV), torch.from_numpy(Y[:, :p].copy()).to(DEV)).cpu().numpy()
                    if p <= 256:
                        assert same_bits(via, got), (p, n)
                    ctx.close("_backend.coldot", f"p={p} n={n}", via, ref)
    for p in (257, 261, 1030) if td == torch.float32 else (257, 515, 1030):      # widths no step kernel takes: the dot still does
        X, Y = ctx.rnd(rng, (37, p)), ctx.rnd(rng, (37, p))
        via = _backend.coldot(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV)).cpu().numpy()
        ctx.close("_backend.coldot", f"p={p}", via, K.coldot(ctx.T(X), ctx.T(Y)))
        sl = _backend.coldot(torch.from_numpy(X).to(DEV)[:, 1:p - 2], torch.from_numpy(Y).to(DEV)[:, 1:p - 2]).cpu().numpy()   # strided, unaligned
        ctx.close("_backend.coldot", f"view p={p}", sl, K.coldot(ctx.T(X[:, 1:p - 2]), ctx.T(Y[:, 1:p - 2])))
    ctx.report()


# ---- K5, four steps ----------------------------------------------------------------------------------------------------------------

def mk_cg(ctx, rng, n, p, n_partial=0, done=0, it=3):
    c = _cols(p)
    rr = ctx.pos(rng, p)
    rr[c % 5 == 4] = 0                                                 # rr_old < eps: beta = 0
    scal = np.stack([rr, ctx.rnd(rng, p), ctx.rnd(rng, p), ctx.pos(rng, p)])
    inp = dict(scal=scal, head=np.array([done, it], dtype=np.int32), fcols=np.stack([c % 7 == 3, c % 13 == 6]).astype(np.int32))
    for k in ("r", "Ap", "x", "pv"):
        inp[k] = ctx.rnd(rng, (max(n, 1), p))
    if n_partial:
        inp["pap"] = ctx.pos(rng, (n_partial, p))
        inp["pap"][:, c % 11 == 5] = 0                                 # p'Ap < eps: alpha = 0
        inp["rrp"] = ctx.pos(rng, (n_partial, p))
        inp["rrp"][:, c % 17 == 8] = 0                                 # a residual of exactly zero: has_converged
        inp["rzp"] = ctx.pos(rng, (max(n_partial // 2, 1), p))
    return inp


def flags_of(inp):
    return np.concatenate([inp["head"], inp["fcols"].reshape(-1)])


def run_cg_alpha(ctx, inp, fold=True):
    p, n_partial = inp["scal"].shape[1], inp["pap"].shape[0]
    pap, scal, fl = ctx.dev(inp["pap"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    fb = ctx.dev(np.full((ctx.lib.tsgu_cg_fold_rows(), p), 0.25)) if fold else None
    launch("tsgu_cg_alpha", ctx.vt, pap, n_partial, fb, scal, fl, EPS, p)
    ref = K.cg_alpha(ctx.T(inp["pap"]), ctx.T(inp["scal"]), flags_of(inp), ctx.r(EPS), p)
    out = scal.get()
    ctx.close("tsgu_cg_alpha", f"scal p={p} rows={n_partial}", out, ref)
    assert np.array_equal(fl.get(), flags_of(inp)) and same_bits(pap.get(), inp["pap"])
    ctx.fin()
    return out


def run_cg_update1(ctx, inp, fused=False, off=0):
    n, p = inp["r"].shape
    R = _geom(p, ctx.wide)
    nb = _blocks(ctx, n, p)
    r, Ap, x, pv = (ctx.dev(inp[k], off) for k in ("r", "Ap", "x", "pv"))
    scal, fl, part = ctx.dev(inp["scal"]), ctx.ints(flags_of(inp)), ctx.dev(np.full((nb, p), 0.25))
    if fused:
        name = "tsgu_cg_update1_alpha"
        args = (ctx.vt, n, p, r, Ap, x, pv, ctx.dev(inp["pap"]), inp["pap"].shape[0], scal, fl, EPS, part)
    else:
        name = "tsgu_cg_update1"
        args = (ctx.vt, n, p, r, Ap, x, pv, scal, fl, part)
    if off or (fused and p > 256):
        assert status(ctx, name, *args) == BAD_ARG, (name, p, off)
        ctx.fin()
        return None
    launch(name, *args)
    Tr = {k: ctx.T(inp[k]) for k in ("r", "Ap", "x", "pv", "scal")}
    if fused:
        ref = K.cg_update1_alpha(Tr["r"], Tr["Ap"], Tr["x"], Tr["pv"], ctx.T(inp["pap"]), Tr["scal"], flags_of(inp), ctx.r(EPS), R)
        rr, rx, rs, rp = ref if ref is not None else (None,) * 4
    else:
        ref = K.cg_update1(Tr["r"], Tr["Ap"], Tr["x"], Tr["pv"], Tr["scal"], flags_of(inp), R)
        rr, rx, rp = ref if ref is not None else (None,) * 3
        rs = Tr["scal"]
    out = dict(r=r.get(), x=x.get(), part=part.get(), scal=scal.get())
    tag = f"p={p} n={n}"
    ctx.close(name, "r " + tag, out["r"], rr, inp["r"])
    ctx.close(name, "x " + tag, out["x"], rx, inp["x"])
    ctx.close(name, "rr_partial " + tag, out["part"], rp, np.full((nb, p), 0.25))
    ctx.close(name, "scal " + tag, out["scal"], rs, inp["scal"])
    assert same_bits(Ap.get(), inp["Ap"]) and same_bits(pv.get(), inp["pv"]) and np.array_equal(fl.get(), flags_of(inp))
    if fused and ref is not None:
        frozen = (inp["fcols"][0] != 0) | (inp["pap"].sum(0) == 0)               # has_converged, or p'Ap < eps: alpha = 0
        assert same_bits(out["r"][:, frozen], inp["r"][:, frozen]) and same_bits(out["x"][:, frozen], inp["x"][:, frozen])
        assert np.all(out["scal"][1, frozen] == 0)
    ctx.fin()
    return out


def run_cg_beta(ctx, inp, precond=False, iter_index=-1, min_iter=2, tol=2.0 ** -40):
    p, n_partial = inp["scal"].shape[1], inp["rrp"].shape[0]
    rrp, scal, fl = ctx.dev(inp["rrp"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    if precond:
        rzp = ctx.dev(inp["rzp"])
        launch("tsgu_cg_beta_precond", ctx.vt, rrp, n_partial, rzp, inp["rzp"].shape[0], scal, fl, EPS, STOP_AFTER, tol, iter_index,
               min_iter, p)
    else:
        launch("tsgu_cg_beta", ctx.vt, rrp, n_partial, scal, fl, EPS, STOP_AFTER, tol, iter_index, min_iter, p)
    rs, rf = K.cg_beta(ctx.T(inp["rrp"]), ctx.T(inp["scal"]), flags_of(inp), ctx.r(EPS), ctx.r(STOP_AFTER), ctx.r(tol), iter_index,
                       min_iter, p, rz_partial=ctx.T(inp["rzp"]) if precond else None)
    name = "tsgu_cg_beta_precond" if precond else "tsgu_cg_beta"
    out = dict(scal=scal.get(), flags=fl.get())
    ctx.close(name, f"scal p={p} rows={n_partial}", out["scal"], rs)
    assert np.array_equal(out["flags"], rf), (name, p, n_partial, out["flags"][:2], rf[:2])
    if inp["head"][0] == 0:
        assert np.all(out["scal"][2, inp["scal"][0] == 0] == 0)                    # rr_old < eps: beta = 0
        assert np.all(out["scal"][3, inp["fcols"][1] != 0] == 0)                   # rhs_is_zero: norm 0
    ctx.fin()
    return out


def run_cg_update2(ctx, inp, off=0):
    n, p = inp["r"].shape
    r, pv, scal, fl = ctx.dev(inp["r"], off), ctx.dev(inp["pv"], off), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    args = (ctx.vt, n, p, r, pv, scal, fl)
    if off:
        assert status(ctx, "tsgu_cg_update2", *args) == BAD_ARG
        ctx.fin()
        return None
    launch("tsgu_cg_update2", *args)
    ref = K.cg_update2(ctx.T(inp["r"]), ctx.T(inp["pv"]), ctx.T(inp["scal"]), flags_of(inp))
    out = dict(pv=pv.get())
    ctx.close("tsgu_cg_update2", f"pvec p={p} n={n}", out["pv"], ref, inp["pv"])
    if ref is not None:
        z = inp["scal"][2] == 0
        assert same_bits(out["pv"][:, z], inp["r"][:, z])
    assert same_bits(r.get(), inp["r"]) and same_bits(scal.get(), inp["scal"])
    ctx.fin()
    return out


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("entry", ["update1", "update1_alpha", "update2"])
def test_cg_vector_steps(td, entry):
    ctx, rng = Ctx(td), np.random.default_rng(2)
    for p in _widths(td):
        for n in _rows(_geom(p, ctx.wide)):
            for off in (0, 1):
                inp = mk_cg(ctx, rng, n, p, n_partial=5)
                if entry == "update2":
                    inp["scal"][2, _cols(p) % 5 == 4] = 0
                    run_cg_update2(ctx, inp, off)
                else:
                    run_cg_update1(ctx, inp, fused=entry == "update1_alpha", off=off)
    if entry == "update1_alpha":                                        # its partial rows: every count, and the refusal past 1024
        for p in (5, 65, 256):
            for rows in PARTIALS:
                run_cg_update1(ctx, mk_cg(ctx, rng, 9, p, n_partial=rows), fused=True)
        inp = mk_cg(ctx, rng, 9, 8, n_partial=1025)
        d = {k: ctx.dev(inp[k]) for k in ("r", "Ap", "x", "pv", "pap", "scal")}
        assert status(ctx, "tsgu_cg_update1_alpha", ctx.vt, 9, 8, d["r"], d["Ap"], d["x"], d["pv"], d["pap"], 1025, d["scal"],
                      ctx.ints(flags_of(inp)), EPS, ctx.dev(np.zeros((1, 8)))) == TOO_LARGE
        ctx.fin()
    ctx.report()


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("entry", ["alpha", "beta", "beta_precond"])
def test_cg_scalar_steps(td, entry):
    ctx, rng = Ctx(td), np.random.default_rng(3)
    for p in _widths(td):
        long = p in (1, 5, 63, 65, 256) or p > 256
        for rows in PARTIALS + (FOLDED if entry == "alpha" else []):
            if rows >= 1024 and not long:
                continue
            inp = mk_cg(ctx, rng, 0, p, n_partial=rows)
            if entry == "alpha":
                run_cg_alpha(ctx, inp)
                if rows in (5, 1025):
                    run_cg_alpha(ctx, inp, fold=False)                 # no fold buffer: the finaliser takes every row itself
            else:
                run_cg_beta(ctx, inp, precond=entry == "beta_precond")
    ctx.report()


# ---- K5, two launches ------------------------------------------------------------------------------------------------------------

def mk_cg2(ctx, rng, n, p, n_partial, parity, done=0, it=3, n_hist=0):
    c = _cols(p)
    rr = [ctx.pos(rng, p), ctx.pos(rng, p)]
    rr[parity][c % 5 == 4] = 0
    scal = np.stack(rr + [ctx.rnd(rng, p), ctx.rnd(rng, p), ctx.pos(rng, p)])
    head = np.array([0, 0, it, 0], dtype=np.int32)
    head[parity] = done
    conv = [c % 7 == 3, c % 7 == 5]
    fcols = np.stack([conv[parity], conv[parity ^ 1], c % 13 == 6]).astype(np.int32)
    inp = dict(scal=scal, head=head, fcols=fcols, parity=parity)
    for k in ("r", "Ap", "x", "pv"):
        inp[k] = ctx.rnd(rng, (n, p))
    inp["pap"] = ctx.pos(rng, (n_partial, p))
    inp["pap"][:, c % 11 == 5] = 0
    inp["rrp"] = ctx.pos(rng, (n_partial, p))
    inp["rrp"][:, c % 17 == 8] = 0
    inp["hist"] = np.zeros((n_hist, 2, p), dtype=ctx.nd) if n_hist else None
    return inp


def _cg2_rows(ctx, n, p):
    """Rows per workgroup of tsgu_cg2_residual: as many groups of four passes as leave at most 1024 partial rows."""
    R = _geom(p, ctx.wide)
    groups = -(-(-(-n // R)) // 1024)
    nb = ctx.lib.tsgu_cg2_num_blocks(ctx.vt, n, p)
    assert nb == -(-n // (R * groups)) and nb <= 1024
    return R * groups, nb, groups


def run_cg2_residual(ctx, inp, off=0):
    n, p = inp["r"].shape
    par = inp["parity"]
    args_of = lambda r, Ap, pap, scal, fl, part: (ctx.vt, n, p, r, Ap, pap, inp["pap"].shape[0], scal, fl, par, EPS, part)   # noqa: E731
    if p > 256 or off or inp["pap"].shape[0] > 1024:
        d = [ctx.dev(inp["r"], off), ctx.dev(inp["Ap"], off), ctx.dev(inp["pap"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp)),
             ctx.dev(np.zeros((1, p)))]
        want = BAD_ARG if (p > 256 or off) else TOO_LARGE
        assert status(ctx, "tsgu_cg2_residual", *args_of(*d)) == want
        ctx.fin()
        return None
    R2, nb, _ = _cg2_rows(ctx, n, p)
    r, Ap, pap, scal, fl = ctx.dev(inp["r"]), ctx.dev(inp["Ap"]), ctx.dev(inp["pap"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    part = ctx.dev(np.full((nb, p), 0.25))
    launch("tsgu_cg2_residual", *args_of(r, Ap, pap, scal, fl, part))
    ref = K.cg2_residual(ctx.T(inp["r"]), ctx.T(inp["Ap"]), ctx.T(inp["pap"]), ctx.T(inp["scal"]), flags_of(inp), par, ctx.r(EPS), R2)
    rr, rs, rp = ref if ref is not None else (None, ctx.T(inp["scal"]), None)
    out = dict(r=r.get(), scal=scal.get(), part=part.get())
    tag = f"p={p} n={n}"
    ctx.close("tsgu_cg2_residual", "r " + tag, out["r"], rr, inp["r"])
    ctx.close("tsgu_cg2_residual", "scal2 " + tag, out["scal"], rs)
    ctx.close("tsgu_cg2_residual", "rr_partial " + tag, out["part"], rp, np.full((nb, p), 0.25))
    assert same_bits(Ap.get(), inp["Ap"]) and np.array_equal(fl.get(), flags_of(inp))
    if ref is not None:
        frozen = (inp["fcols"][par] != 0) | (inp["pap"].sum(0) == 0)
        assert same_bits(out["r"][:, frozen], inp["r"][:, frozen]) and np.all(out["scal"][2, frozen] == 0)
    ctx.fin()
    return out


def run_cg2_direction(ctx, inp, off=0, min_iter=2, tol=2.0 ** -40):
    n, p = inp["r"].shape
    par, hist = inp["parity"], inp["hist"]
    n_hist = 0 if hist is None else hist.shape[0]
    n_partial = inp["rrp"].shape[0]
    r, pv, x = ctx.dev(inp["r"], off), ctx.dev(inp["pv"], off), ctx.dev(inp["x"], off)
    rrp, scal, fl = ctx.dev(inp["rrp"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    hd = ctx.dev(hist) if n_hist else None
    args = (ctx.vt, n, p, r, pv, x, rrp, n_partial, scal, fl, par, EPS, STOP_AFTER, tol, min_iter, hd, n_hist)
    if p > 256 or off or n_partial > 1024:
        assert status(ctx, "tsgu_cg2_direction", *args) == (BAD_ARG if (p > 256 or off) else TOO_LARGE)
        ctx.fin()
        return None
    launch("tsgu_cg2_direction", *args)
    rp, rx, rs, rf, rh = K.cg2_direction(ctx.T(inp["r"]), ctx.T(inp["pv"]), ctx.T(inp["x"]), ctx.T(inp["rrp"]), ctx.T(inp["scal"]),
                                         flags_of(inp), par, ctx.r(EPS), ctx.r(STOP_AFTER), ctx.r(tol), min_iter,
                                         ctx.T(hist) if n_hist else None, n_hist)
    out = dict(pv=pv.get(), x=x.get(), scal=scal.get(), flags=fl.get(), hist=hd.get() if n_hist else None)
    tag = f"p={p} n={n} rows={n_partial}"
    ctx.close("tsgu_cg2_direction", "pvec " + tag, out["pv"], rp, inp["pv"])
    ctx.close("tsgu_cg2_direction", "x " + tag, out["x"], rx, inp["x"])
    ctx.close("tsgu_cg2_direction", "scal2 " + tag, out["scal"], rs)
    assert np.array_equal(out["flags"], rf), (tag, out["flags"][:4], rf[:4])
    if n_hist:
        ctx.close("tsgu_cg2_direction", "hist " + tag, out["hist"], rh)
        it = int(inp["head"][2])
        if rp is not None and it < n_hist:
            assert same_bits(out["hist"][it, 0], inp["scal"][2]) and same_bits(out["hist"][it, 1], out["scal"][3])
        assert not np.any(np.delete(out["hist"], it, axis=0) if (rp is not None and it < n_hist) else out["hist"])
    if rp is not None:
        z = inp["scal"][par] == 0
        assert same_bits(out["pv"][:, z], inp["r"][:, z])                              # rr_old < eps: beta = 0, p = r
        assert np.all(out["scal"][4, inp["fcols"][2] != 0] == 0)
    assert same_bits(r.get(), inp["r"])
    ctx.fin()
    return out


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("entry", ["residual", "direction"])
def test_cg2_steps(td, entry):
    ctx, rng = Ctx(td), np.random.default_rng(4)
    run = run_cg2_residual if entry == "residual" else run_cg2_direction
    k = 0
    for p in _widths(td):
        for n in _rows(_geom(p, ctx.wide)):
            for off in (0, 1):
                k += 1
                # with a hist buffer of 4 rows the counter stands at 0, 3 (the last row), 4 and 7 (past it: nothing may be written)
                n_hist = 4 if k % 3 else 0
                run(ctx, mk_cg2(ctx, rng, n, p, 5, parity=(k >> 1) & 1, n_hist=n_hist, it=(0, 3, 4, 7)[(k // 3) % 4]), off=off)
    for p in (5, 65, 256):
        for rows in PARTIALS + [1025]:
            run(ctx, mk_cg2(ctx, rng, 9, p, rows, parity=rows & 1))
    ctx.report()


@pytest.mark.parametrize("td", DTYPES)
def test_cg2_groups_of_passes(td):
    """Workgroups that take 1, 2 and 3 groups of four passes: the unrolled instances (wide lanes) and the generic one; p = 255 takes
    the scalar-lane instance with 2 groups."""
    ctx, rng = Ctx(td), np.random.default_rng(5)
    k1 = 1024 * _geom(256, ctx.wide)
    shapes = [(256, 1027, 1), (256, k1 + 1, 2), (256, 2 * k1 + 1, 3), (255, 4 * 1024 + 1, 2)]
    for p, n, groups in shapes:
        assert _cg2_rows(ctx, n, p)[2] == groups, (p, n)
        inp = mk_cg2(ctx, rng, n, p, 3, parity=groups & 1)
        run_cg2_residual(ctx, inp)
        inp["rrp"] = ctx.pos(rng, (_cg2_rows(ctx, n, p)[1], p))
        run_cg2_direction(ctx, inp)
    ctx.report()


# ---- K7 MINRES -------------------------------------------------------------------------------------------------------------------

def mk_minres(ctx, rng, n, p, S, rows=5, stop=0, it=4):
    scal = ctx.rnd(rng, (S, 12, p))
    for k in (1, 9, 11):
        scal[:, k] = ctx.pos(rng, (S, p))
    inp = dict(scal=scal, flags=np.array([stop, it], dtype=np.int32), shifts=ctx.rnd(rng, S), value=0.75)
    inp["part"] = ctx.pos(rng, (2 * S, rows, p))
    for k in ("zpp", "zp", "prod", "qc"):
        inp[k] = ctx.rnd(rng, (max(n, 1), p))
    for k in ("wpp", "wp", "sol"):
        inp[k] = ctx.rnd(rng, (S, max(n, 1), p))
    return inp


def run_minres_scalar(ctx, inp, phase, tol=2.0 ** -60, single=False, fold=True, eps=2.0 ** -40):
    S, _, p = inp["scal"].shape
    rows = inp["part"].shape[1]
    part, scal, fl, sh = ctx.dev(inp["part"]), ctx.dev(inp["scal"]), ctx.ints(inp["flags"]), ctx.dev(inp["shifts"])
    fb = ctx.dev(np.full((ctx.lib.tsgu_cg_fold_rows(), p), 0.25)) if fold else None
    value = 1.0 if single else inp["value"]
    if single:
        launch("tsgu_minres_scalar", ctx.vt, phase, part, rows, rows * p, fb, scal, fl, eps, tol, float(inp["shifts"][0]), p)
    else:
        launch("tsgu_minres_scalar_ms", ctx.vt, phase, part, rows, rows * p, fb, scal, fl, eps, tol, sh, S, value, p)
    sets = ctx.T(inp["part"])
    rs, rf = K.minres_scalar(phase, sets if phase == 2 else sets[0], ctx.T(inp["scal"]), inp["flags"], ctx.r(eps), ctx.r(tol),
                             ctx.T(inp["shifts"]).v, ctx.r(value))
    out = dict(scal=scal.get(), flags=fl.get())
    ctx.close(f"tsgu_minres_scalar{'' if single else '_ms'}({phase})", f"scal p={p} rows={rows} S={S}", out["scal"], rs)
    assert np.array_equal(out["flags"], rf), (phase, p, rows, out["flags"], rf)
    assert same_bits(part.get(), inp["part"])
    ctx.fin()
    return out


def run_minres_vector(ctx, inp, which, with_norms=True, use_qc=False, single=False, off=0):
    n, p = inp["zp"].shape
    S = inp["scal"].shape[0]
    R, nb = _geom(p, ctx.wide), _blocks(ctx, n, p)
    plane = -(-n * p // 4) * 4                                             # planes of the shifts start on 16-byte boundaries
    planes = lambda a: np.concatenate([a.reshape(S, n * p), np.zeros((S, plane - n * p), dtype=a.dtype)], axis=1)   # noqa: E731
    scal, fl = ctx.dev(inp["scal"]), ctx.ints(inp["flags"])
    part = ctx.dev(np.full((2 * S, nb, p), 0.25))
    name = "tsgu_minres_vector" if single else "tsgu_minres_vector_ms"
    Tr = {k: ctx.T(inp[k]) for k in inp if k not in ("flags", "value")}
    value = 1.0 if single else inp["value"]
    if which == 0:
        zpp, zp, prod = ctx.dev(inp["zpp"], off), ctx.dev(inp["zp"], off), ctx.dev(inp["prod"], off)
        if single:
            args = (ctx.vt, 0, n, p, zpp, zp, prod, None, None, scal, fl, part, nb * p, 0)
        else:
            args = (ctx.vt, 0, n, p, zpp, zp, prod, None, None, None, scal, fl, part, nb * p, 0, S, plane, value)
        if off:
            assert status(ctx, name, *args) == BAD_ARG
            ctx.fin()
            return None
        launch(name, *args)
        ref = K.minres_lanczos(Tr["zpp"], Tr["zp"], Tr["prod"], Tr["scal"], inp["flags"], ctx.r(value), R)
        rz, rp = ref if ref is not None else (None, None)
        out = dict(zc=zpp.get(), part=part.get()[0])
        ctx.close(f"{name}(0)", f"z_c p={p} n={n}", out["zc"], rz, inp["zpp"])
        ctx.close(f"{name}(0)", f"partial p={p} n={n}", out["part"], rp, np.full((nb, p), 0.25))
        assert same_bits(zp.get(), inp["zp"]) and same_bits(prod.get(), inp["prod"])
        assert same_bits(part.get()[1:], np.full((2 * S - 1, nb, p), 0.25, dtype=ctx.nd))
    else:
        zc, qp, qc = ctx.dev(inp["zpp"], off), ctx.dev(inp["zp"], off), (ctx.dev(inp["qc"], off) if use_qc else None)
        wpp, wp, sol = ctx.dev(planes(inp["wpp"]), off), ctx.dev(planes(inp["wp"]), off), ctx.dev(planes(inp["sol"]), off)
        if single:
            args = (ctx.vt, 1, n, p, zc, qp, wpp, wp, sol, scal, fl, part, nb * p, int(with_norms))
        else:
            args = (ctx.vt, 1, n, p, zc, qp, wpp, wp, sol, qc, scal, fl, part, nb * p, int(with_norms), S, plane, value)
        if off:
            assert status(ctx, name, *args) == BAD_ARG
            ctx.fin()
            return None
        launch(name, *args)
        ref = K.minres_update(Tr["zpp"], Tr["zp"], Tr["wpp"], Tr["wp"], Tr["sol"], Tr["scal"], inp["flags"], R, with_norms,
                              qc=Tr["qc"] if use_qc else None)
        rz, rq, rw, rx, rp = ref if ref is not None else (None,) * 5
        unplane = lambda d: d.get()[:, :n * p].reshape(S, n, p)               # noqa: E731
        out = dict(zc=zc.get(), w=unplane(wpp), sol=unplane(sol), part=part.get(), qc=qc.get() if use_qc else None)
        tag = f"p={p} n={n} S={S}"
        ctx.close(f"{name}(1)", "z_c " + tag, out["zc"], rz, inp["zpp"])
        if use_qc:
            ctx.close(f"{name}(1)", "q_c " + tag, out["qc"], rq, inp["qc"])
        ctx.close(f"{name}(1)", "w_c " + tag, out["w"], rw, inp["wpp"])
        ctx.close(f"{name}(1)", "sol " + tag, out["sol"], rx, inp["sol"])
        ctx.close(f"{name}(1)", "partial " + tag, out["part"], rp, np.full((2 * S, nb, p), 0.25))
        assert same_bits(qp.get(), inp["zp"]) and same_bits(wp.get(), planes(inp["wp"]))
        assert not np.any(wpp.get()[:, n * p:]) and not np.any(sol.get()[:, n * p:])        # the padding between the planes
    assert same_bits(scal.get(), inp["scal"]) and np.array_equal(fl.get(), inp["flags"])
    ctx.fin()
    return out


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_minres_scalar_steps(td, phase):
    ctx, rng = Ctx(td), np.random.default_rng(6 + phase)
    for p in _widths(td):
        long = p in (1, 5, 63, 65, 256) or p > 256
        for rows in PARTIALS + (FOLDED if phase < 2 else []):
            if rows >= 1024 and not long:
                continue
            S = 1 if rows >= 1024 else 3
            inp = mk_minres(ctx, rng, 0, p, S, rows=rows)
            ms = run_minres_scalar(ctx, inp, phase)
            if rows in (4, 1025):
                run_minres_scalar(ctx, inp, phase, fold=False)
            if rows == 5:                                                 # one shift, value 1: the single-shift entry gives the same bits
                one = mk_minres(ctx, rng, 0, p, 1, rows=rows)
                one["value"] = 1.0
                a, b = run_minres_scalar(ctx, one, phase), run_minres_scalar(ctx, one, phase, single=True)
                assert same_bits(a["scal"], b["scal"]) and np.array_equal(a["flags"], b["flags"])
            assert ms["flags"][1] == inp["flags"][1] + (phase == 1)
    ctx.report()


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("which", [0, 1])
def test_minres_vector_steps(td, which):
    ctx, rng = Ctx(td), np.random.default_rng(9 + which)
    k = 0
    for p in _widths(td):
        for n in _rows(_geom(p, ctx.wide)):
            k += 1
            S = 1 + (k % 3 == 0) * 2
            inp = mk_minres(ctx, rng, n, p, S)
            run_minres_vector(ctx, inp, which, with_norms=bool(k & 1), use_qc=bool(k & 2))
            run_minres_vector(ctx, inp, which, off=1)
            if k % 4 == 0:
                one = mk_minres(ctx, rng, n, p, 1)
                one["value"] = 1.0
                a, b = run_minres_vector(ctx, one, which), run_minres_vector(ctx, one, which, single=True)
                assert all(same_bits(a[key], b[key]) for key in a if a[key] is not None)
    ctx.report()


# ---- K6 BiCGSTAB -----------------------------------------------------------------------------------------------------------------

MATVEC_MAX = 6


def mk_bicg(ctx, rng, n, p, rows=5, stop=0, it=2, phase=None):
    c = _cols(p)
    scal = ctx.rnd(rng, (8, p))
    scal[4] = ctx.pos(rng, p) * ctx.nd(2.0 ** -10)                          # thresholds far below sums of order one
    for k in (0, 2):
        scal[k] = ctx.pos(rng, p) * np.where(rng.random(p) < 0.5, -1, 1).astype(ctx.nd)      # the divisors rho, omega
    fin, half = (c % 7 == 3), (c % 5 == 1) & (c % 7 != 3)
    nmv = 3 + (c % 4)                                                       # some columns at the matvec budget (6) after this step
    inp = dict(scal=scal, head=np.array([stop, it], dtype=np.int32), fcols=np.stack([fin, half, nmv]).astype(np.int32))
    sign = phase in (2, 4)
    inp["part"] = (ctx.rnd if sign else ctx.pos)(rng, (3, rows, p))
    if sign:
        inp["part"][1] = ctx.pos(rng, (rows, p))                            # <t, t>
        inp["part"][0] = ctx.pos(rng, (rows, p)) * np.where(c % 2, -1, 1).astype(ctx.nd)     # <r0, v>, <t, s>: one sign per column
    else:
        inp["part"][:, :, c % 11 == 5] = 0                                  # |s|, |r| of exactly zero: below every threshold
    for k in ("x", "r", "s", "t", "pv", "v", "r0", "z"):
        inp[k] = ctx.rnd(rng, (max(n, 1), p))
    return inp


def run_bicg_scalar(ctx, inp, phase, fold=True, matvec_max=MATVEC_MAX, nmv0=1):
    p, rows = inp["scal"].shape[1], inp["part"].shape[1]
    part, scal, fl = ctx.dev(inp["part"]), ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    fb = ctx.dev(np.full((ctx.lib.tsgu_cg_fold_rows(), p), 0.25)) if fold else None
    abstol, reltol = 2.0 ** -20, 2.0 ** -12
    launch("tsgu_bicg_scalar", ctx.vt, phase, part if phase != 1 else None, rows if phase != 1 else 0, rows * p, fb, scal, fl, abstol,
           reltol, matvec_max, nmv0, p)
    sets = ctx.T(inp["part"])
    rs, rf = K.bicg_scalar(phase, None if phase == 1 else (sets if phase == 4 else sets[0]), ctx.T(inp["scal"]), flags_of(inp),
                           ctx.r(abstol), ctx.r(reltol), matvec_max, nmv0)
    out = dict(scal=scal.get(), flags=fl.get())
    ctx.close(f"tsgu_bicg_scalar({phase})", f"scal p={p} rows={rows}", out["scal"], rs)
    assert np.array_equal(out["flags"], rf), (phase, p, rows, out["flags"][:2], rf[:2])
    if phase != 0 and inp["head"][0] == 0:
        done = inp["fcols"][0] != 0
        assert same_bits(out["scal"][:, done], inp["scal"][:, done])          # finished columns keep every scalar
    ctx.fin()
    return out


def run_bicg_vector(ctx, inp, which, off=0, precond=False):
    n, p = inp["x"].shape
    R, nb = _geom(p, ctx.wide), _blocks(ctx, n, p)
    scal, fl = ctx.dev(inp["scal"]), ctx.ints(flags_of(inp))
    part = ctx.dev(np.full((3, nb, p), 0.25))
    d = {k: ctx.dev(inp[k], off) for k in ("x", "r", "s", "t", "pv", "v", "r0", "z")}
    Tr = {k: ctx.T(inp[k]) for k in ("x", "r", "s", "t", "pv", "v", "r0", "z", "scal")}
    fl_in = flags_of(inp)
    if precond:
        name = "tsgu_bicg_update_x_precond"
        args = (ctx.vt, n, p, d["x"], d["r"], d["s"], d["t"], d["pv"], d["z"], scal, fl, part)
    else:
        name = "tsgu_bicg_vector"
        ops = [("pv", "r", "v", None, None), ("s", "r", "v", None, None), ("t", "s", "r0", None, None), ("x", "r", "s", "t", "pv")][which]
        args = (ctx.vt, which, n, p, *[d[k] if k else None for k in ops], scal, fl, part, nb * p)
    if off:
        assert status(ctx, name, *args) == BAD_ARG
        ctx.fin()
        return None
    launch(name, *args)
    tag = f"p={p} n={n}"
    label = name if precond else f"{name}({which})"
    fresh = np.full((3, nb, p), 0.25)
    out, changed = {}, set()
    if which == 0 and not precond:
        ref = K.bicg_update_p(Tr["pv"], Tr["r"], Tr["v"], Tr["scal"], fl_in)
        out["pv"] = d["pv"].get()
        ctx.close(label, "p " + tag, out["pv"], ref, inp["pv"])
        changed = {"pv"}
        assert same_bits(part.get(), fresh.astype(ctx.nd))
    elif which == 1 and not precond:
        ref = K.bicg_update_s(Tr["s"], Tr["r"], Tr["v"], Tr["scal"], fl_in, R)
        rs, rp = ref if ref is not None else (None, None)
        out["s"], out["part"] = d["s"].get(), part.get()
        ctx.close(label, "s " + tag, out["s"], rs, inp["s"])
        ctx.close(label, "partial " + tag, out["part"][0], rp, fresh[0])
        changed = {"s"}
    elif which == 2 and not precond:
        ref = K.bicg_dots3(Tr["t"], Tr["s"], Tr["r0"], fl_in, R)
        out["part"] = part.get()
        ctx.close(label, "partial " + tag, out["part"], ref, fresh)
    else:
        ref = K.bicg_update_x(Tr["x"], Tr["r"], Tr["s"], Tr["t"], Tr["pv"], Tr["scal"], fl_in, R, z=Tr["z"] if precond else None)
        rx, rr, rp = ref if ref is not None else (None, None, None)
        out["x"], out["r"], out["part"] = d["x"].get(), d["r"].get(), part.get()
        ctx.close(label, "x " + tag, out["x"], rx, inp["x"])
        ctx.close(label, "r " + tag, out["r"], rr, inp["r"])
        ctx.close(label, "partial " + tag, out["part"][0], rp, fresh[0])
        changed = {"x", "r"}
    for k in d:
        if k not in changed:
            assert same_bits(d[k].get(), inp[k]), (label, k)
    if ref is not None:
        done = inp["fcols"][0] != 0
        for k in changed:
            assert same_bits(out[k][:, done], inp[k][:, done]), (label, k)              # finished columns are frozen
    assert same_bits(scal.get(), inp["scal"]) and np.array_equal(fl.get(), fl_in)
    ctx.fin()
    return out


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("phase", [0, 1, 2, 3, 4, 5])
def test_bicg_scalar_steps(td, phase):
    ctx, rng = Ctx(td), np.random.default_rng(20 + phase)
    for p in _widths(td):
        long = p in (1, 5, 63, 65, 256) or p > 256
        for rows in ([5] if phase == 1 else PARTIALS + (FOLDED if phase in (0, 2, 3, 5) else [])):
            if rows >= 1024 and not long:
                continue
            inp = mk_bicg(ctx, rng, 0, p, rows=rows, phase=phase)
            run_bicg_scalar(ctx, inp, phase)
            if rows in (4, 1025):
                run_bicg_scalar(ctx, inp, phase, fold=False)
    ctx.report()


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("which", [0, 1, 2, 3, "precond"])
def test_bicg_vector_steps(td, which):
    ctx, rng = Ctx(td), np.random.default_rng(30)
    for p in _widths(td):
        for n in _rows(_geom(p, ctx.wide)):
            inp = mk_bicg(ctx, rng, n, p)
            for off in (0, 1):
                run_bicg_vector(ctx, inp, 3 if which == "precond" else which, off=off, precond=which == "precond")
    ctx.report()


@pytest.mark.parametrize("td", DTYPES)
def test_hist_rows_only_below_n_hist(td):
    """alpha and beta of iteration `it` go to row `it` of hist while it < n_hist; at and past n_hist nothing is written (the rows
    stay zero, the sentinels behind the buffer stay intact: run_cg2_direction asserts both)."""
    ctx, rng = Ctx(td), np.random.default_rng(43)
    for p in (3, 65, 256):
        for it in (0, 3, 4, 7):
            for par in (0, 1):
                out = run_cg2_direction(ctx, mk_cg2(ctx, rng, 9, p, 5, parity=par, it=it, n_hist=4))
                assert bool(np.any(out["hist"])) == (it < 4) and out["flags"][2] == it + 1
                if it < 4:
                    assert np.any(out["hist"][it, 0]) and not np.any(np.delete(out["hist"], it, axis=0))


@pytest.mark.parametrize("td", DTYPES)
def test_widths_no_geometry_covers_are_refused(td):
    """More than 256 columns that are no multiple of the 16-byte lane width, or more than 256 lanes: the vector entries answer
    TSGU_ERR_TOO_LARGE (the one-launch and two-launch CG forms, which stop at 256 columns, TSGU_ERR_BAD_ARG) and touch nothing."""
    ctx, rng = Ctx(td), np.random.default_rng(44)
    n = 3
    for p in ((257, 1028) if td == torch.float32 else (259, 514)):
        assert ctx.lib.tsgu_cg_num_blocks(ctx.vt, n, p) == -1 and _geom(p, ctx.wide) is None
        v = [ctx.dev(ctx.rnd(rng, (n, p))) for _ in range(6)]
        plane = -(-n * p // 4) * 4                                        # planes of the shifts on 16-byte boundaries
        w = [ctx.dev(ctx.rnd(rng, (2, plane))) for _ in range(3)]
        scal, fl, part = ctx.dev(ctx.pos(rng, (2, 12, p))), ctx.ints(np.zeros(4 + 3 * p)), ctx.dev(np.full((6, n, p), 0.25))
        sh = ctx.dev(ctx.rnd(rng, 2))
        before = [d.get() for d in v + w + [scal, part]]
        calls = [("tsgu_cg_update1", (n, p, v[0], v[1], v[2], v[3], scal, fl, part), TOO_LARGE),
                 ("tsgu_cg_update2", (n, p, v[0], v[1], scal, fl), TOO_LARGE),
                 ("tsgu_cg_update1_alpha", (n, p, v[0], v[1], v[2], v[3], part, 1, scal, fl, EPS, part), BAD_ARG),
                 ("tsgu_cg2_residual", (n, p, v[0], v[1], part, 1, scal, fl, 0, EPS, part), BAD_ARG),
                 ("tsgu_cg2_direction", (n, p, v[0], v[1], v[2], part, 1, scal, fl, 0, EPS, STOP_AFTER, 1.0, 2, None, 0), BAD_ARG),
                 ("tsgu_minres_vector", (0, n, p, v[0], v[1], v[2], None, None, scal, fl, part, n * p, 0), TOO_LARGE),
                 ("tsgu_minres_vector", (1, n, p, v[0], v[1], w[0], w[1], w[2], scal, fl, part, n * p, 1), TOO_LARGE),
                 ("tsgu_minres_vector_ms", (0, n, p, v[0], v[1], v[2], None, None, None, scal, fl, part, n * p, 0, 2, plane, 0.75), TOO_LARGE),
                 ("tsgu_minres_vector_ms", (1, n, p, v[0], v[1], w[0], w[1], w[2], v[3], scal, fl, part, n * p, 1, 2, plane, 0.75), TOO_LARGE),
                 ("tsgu_bicg_update_x_precond", (n, p, v[0], v[1], v[2], v[3], v[4], v[5], scal, fl, part), TOO_LARGE)]
        calls += [("tsgu_bicg_vector", (which, n, p, v[0], v[1], v[2], v[3], v[4], scal, fl, part, n * p), TOO_LARGE) for which in range(4)]
        calls += [("tsgu_coldot", (n, p, v[0], p, v[1], p, part, scal), TOO_LARGE)]
        for name, args, want in calls:
            assert status(ctx, name, ctx.vt, *args) == want, (name, p, args[0])
        del sh
        assert all(same_bits(d.get(), b) for d, b in zip(v + w + [scal, part], before))
        ctx.fin()


# ---- exact behaviour ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("td", DTYPES)
def test_every_entry_is_a_noop_once_its_stop_word_is_set(td):
    """The run_* helpers compare every output with its input, bit for bit, where the mirror says the step does nothing; the one
    change allowed is tsgu_cg2_direction carrying the flag to the other half."""
    ctx, rng = Ctx(td), np.random.default_rng(40)
    for p in (5, 64, 129, 256, WIDE[td][0], WIDE[td][-1]):
        n = _geom(p, ctx.wide) + 1
        inp = mk_cg(ctx, rng, n, p, n_partial=5, done=1)
        before = flags_of(inp)
        run_cg_alpha(ctx, inp)
        run_cg_update1(ctx, inp)
        assert np.array_equal(run_cg_beta(ctx, inp)["flags"], before)
        assert np.array_equal(run_cg_beta(ctx, inp, precond=True)["flags"], before)
        run_cg_update2(ctx, inp)
        big = mk_cg(ctx, rng, n, p, n_partial=1025, done=1)
        run_cg_alpha(ctx, big)                                            # the fold honours the stop word too
        if p <= 256:
            run_cg_update1(ctx, inp, fused=True)
            for par in (0, 1):
                two = mk_cg2(ctx, rng, n, p, 5, parity=par, done=1, n_hist=4)
                run_cg2_residual(ctx, two)
                out = run_cg2_direction(ctx, two)
                want = flags_of(two)
                want[par ^ 1] = 1
                assert np.array_equal(out["flags"], want)
        m = mk_minres(ctx, rng, n, p, 2, stop=1)
        for phase in (0, 1, 2):
            assert np.array_equal(run_minres_scalar(ctx, m, phase, tol=2.0 ** 60)["flags"], m["flags"])
        for which in (0, 1):
            run_minres_vector(ctx, m, which, use_qc=True)
        b = mk_bicg(ctx, rng, n, p, stop=1)
        for phase in (1, 2, 3, 4, 5):
            assert np.array_equal(run_bicg_scalar(ctx, mk_bicg(ctx, rng, n, p, stop=1, phase=phase), phase)["flags"][:2], [1, 2])
        for which in (0, 1, 2, 3):
            run_bicg_vector(ctx, b, which)
        run_bicg_vector(ctx, b, 3, precond=True)
        out = run_bicg_scalar(ctx, b, 0)                                  # INIT runs whatever the stop word says
        assert out["flags"][0] == int(np.all(out["flags"][2:2 + p] != 0))


@pytest.mark.parametrize("td", DTYPES)
def test_counters_and_stop_rules(td):
    ctx, rng = Ctx(td), np.random.default_rng(41)
    for p in (3, 65, 256, WIDE[td][-1]):
        # CG: stop needs it >= min_iter_index AND mean < tolerance; the mean of sqrt(sums of order one) is of order one
        for it, min_iter, tol, want in ((5, 5, 2.0 ** 20, 1), (4, 5, 2.0 ** 20, 0), (5, 5, 2.0 ** -20, 0), (9, 5, 2.0 ** 20, 1)):
            inp = mk_cg(ctx, rng, 0, p, n_partial=4, it=it)
            out = run_cg_beta(ctx, inp, min_iter=min_iter, tol=tol)
            assert out["flags"][0] == want and out["flags"][1] == it + 1
            if p <= 256:
                for par in (0, 1):
                    two = mk_cg2(ctx, rng, 3, p, 4, parity=par, it=it)
                    out = run_cg2_direction(ctx, two, min_iter=min_iter, tol=tol)
                    assert out["flags"][par ^ 1] == want and out["flags"][par] == 0 and out["flags"][2] == it + 1
        inp = mk_cg(ctx, rng, 0, p, n_partial=4, it=0)                      # iter_index >= 0 overrides the device counter
        assert run_cg_beta(ctx, inp, iter_index=7, min_iter=7, tol=2.0 ** 20)["flags"][:2].tolist() == [1, 8]
        assert run_cg_beta(ctx, inp, iter_index=6, min_iter=7, tol=2.0 ** 20)["flags"][:2].tolist() == [0, 7]
        # MINRES: mean(|update| / |sol|) < tol stops; a NaN ratio (0 / 0) never does
        m = mk_minres(ctx, rng, 0, p, 2, rows=4)
        assert run_minres_scalar(ctx, m, 2, tol=2.0 ** 20)["flags"].tolist() == [1, 4]
        assert run_minres_scalar(ctx, m, 2, tol=2.0 ** -20)["flags"].tolist() == [0, 4]
        assert run_minres_scalar(ctx, m, 1)["flags"].tolist() == [0, 5]
        m["part"][0:2, :, 0] = 0
        assert run_minres_scalar(ctx, m, 2, tol=2.0 ** 20)["flags"].tolist() == [0, 4]
        # BiCGSTAB: the budget reached at the half step and at the end, the early exit after the half step, the counters
        for phase in (3, 5):
            b = mk_bicg(ctx, rng, 0, p, rows=4, phase=phase)
            out = run_bicg_scalar(ctx, b, phase)
            fin, half, nmv = (out["flags"][2 + k * p:2 + (k + 1) * p] for k in range(3))
            fin0, half0, nmv0 = b["fcols"]
            run = fin0 == 0
            small = b["part"][0].sum(0) == 0
            assert np.array_equal(nmv, nmv0) and out["flags"][1] == 2 + (phase == 5)
            if phase == 3:
                assert np.array_equal(half[run], (half0[run] != 0) | small[run])
                assert np.array_equal(fin[run], ~small[run] & (nmv0[run] >= MATVEC_MAX))
            else:
                assert not half[run].any()
                assert np.array_equal(fin[run] != 0, (half0[run] != 0) | small[run] | (nmv0[run] >= MATVEC_MAX))
                assert out["flags"][0] == int(np.all(fin != 0))
            assert np.array_equal(fin[~run], fin0[~run]) and np.array_equal(half[~run], half0[~run])
        for phase in (2, 4):
            b = mk_bicg(ctx, rng, 0, p, rows=4, phase=phase)
            out = run_bicg_scalar(ctx, b, phase)
            fin0, half0, nmv0 = b["fcols"]
            counted = (fin0 == 0) & ((half0 == 0) | (phase == 2))
            assert np.array_equal(out["flags"][2 + 2 * p:], nmv0 + counted)
        b = mk_bicg(ctx, rng, 0, p, rows=4, phase=0)
        out = run_bicg_scalar(ctx, b, 0, matvec_max=1, nmv0=1)            # the budget spent before the first iteration
        assert out["flags"][0] == 1 and np.all(out["flags"][2:2 + p] == 1) and np.all(out["flags"][2 + 2 * p:] == 1)


@pytest.mark.parametrize("td", DTYPES)
def test_repeatable_and_independent_of_the_width(td):
    """Two launches on the same inputs give the same bits (sums included); the elementwise outputs of a column are the same bits
    whether it sits in a narrow or in a wide array (its sums may be associated differently: they stay under the bound)."""
    ctx, rng = Ctx(td), np.random.default_rng(42)
    wide_p = WIDE[td][1]
    for p_w, p_n in ((256, 5), (wide_p, 5), (wide_p, 64), (255, 3)):
        n = 3 * _geom(p_n, ctx.wide) + 2
        cut = lambda inp: {k: (v[..., :p_n].copy() if isinstance(v, np.ndarray) and v.ndim and v.shape[-1] == p_w else v)   # noqa: E731
                           for k, v in inp.items()}
        cg = mk_cg(ctx, rng, n, p_w, n_partial=5)
        a, b, c = run_cg_update1(ctx, cg), run_cg_update1(ctx, cg), run_cg_update1(ctx, cut(cg))
        assert all(same_bits(a[k], b[k]) for k in a)
        assert same_bits(a["r"][:, :p_n], c["r"]) and same_bits(a["x"][:, :p_n], c["x"])
        a, b, c = run_cg_update2(ctx, cg), run_cg_update2(ctx, cg), run_cg_update2(ctx, cut(cg))
        assert same_bits(a["pv"], b["pv"]) and same_bits(a["pv"][:, :p_n], c["pv"])
        a, b = run_cg_beta(ctx, cg), run_cg_beta(ctx, cg)
        assert same_bits(a["scal"], b["scal"])
        m = mk_minres(ctx, rng, n, p_w, 2)
        for which, keys in ((0, ["zc"]), (1, ["zc", "w", "sol"])):
            a, b, c = run_minres_vector(ctx, m, which), run_minres_vector(ctx, m, which), run_minres_vector(ctx, cut(m), which)
            assert all(same_bits(a[k], b[k]) for k in a if a[k] is not None)
            assert all(same_bits(a[k][..., :p_n], c[k]) for k in keys)
        bi = mk_bicg(ctx, rng, n, p_w)
        for which, keys in ((0, ["pv"]), (1, ["s"]), (3, ["x", "r"])):
            a, b, c = run_bicg_vector(ctx, bi, which), run_bicg_vector(ctx, bi, which), run_bicg_vector(ctx, cut(bi), which)
            assert all(same_bits(a[k], b[k]) for k in a)
            assert all(same_bits(a[k][:, :p_n], c[k]) for k in keys)
        if p_w <= 256:
            two = mk_cg2(ctx, rng, n, p_w, 5, parity=1)
            a, b, c = run_cg2_direction(ctx, two), run_cg2_direction(ctx, two), run_cg2_direction(ctx, cut(two))
            assert same_bits(a["pv"], b["pv"]) and same_bits(a["scal"], b["scal"])
            assert same_bits(a["x"][:, :p_n], c["x"])                     # (x uses alpha only, which is an input of this step)


# ---- solves wider than 256 columns, end to end --------------------------------------------------------------------------------------

def _tiled(base, p):
    """(n, p) right-hand sides from the stored columns: column j is stored column j mod k scaled by 1 + j / 64."""
    k = base.shape[1]
    j = np.arange(p)
    return np.ascontiguousarray(base[:, j % k] * (1.0 + j / 64.0))


def _rel(x, ref):
    return float(np.abs(x.double().cpu().numpy() - ref).max() / np.abs(ref).max())


# float64: the tolerances of test_generic_solve_all_solvers_fwd_bwd for the same systems (the reference's CG freezes near 1e-5 ... 1e-6:
# its eps guards act on squared norms).  float32: the suite's float32 tolerance for these systems (2e-5, the stored fp32 BiCGSTAB
# iterate of test_generic_solve_nonsymmetric_with_transpose_solver_and_bicgstab32): cond(A) u is 1e-6 for both matrices.
SOLVE_TOL = {torch.float64: dict(cg=2e-5, bicgstab=1e-9, minres=1e-9), torch.float32: dict(cg=2e-5, bicgstab=2e-5, minres=2e-5)}


@pytest.mark.parametrize("td,p", [(torch.float32, 260), (torch.float64, 260), (torch.float32, 1024), (torch.float64, 512)])
def test_solves_with_more_than_256_right_hand_sides(td, p):
    from torchsparsegradutils_amd.utils import (BICGSTABSettings, LinearCGSettings, MINRESSettings, bicgstab, linear_cg, minres)

    z = G.load("generic_small.npz")
    S, Tm = z["S"], z["nonsym_T"]
    tol = SOLVE_TOL[td]
    A = torch.from_numpy(S).to(td).to(DEV).to_sparse_csr()
    An = torch.from_numpy(Tm).to(td).to(DEV).to_sparse_csr()
    tight = td == torch.float64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        B = _tiled(z["csr_2d6_cg_B"], p)
        x = linear_cg(A, torch.from_numpy(B).to(td).to(DEV), settings=LinearCGSettings(cg_tolerance=1e-12))
        e = _rel(x, np.linalg.solve(S, B))
        print(f"[wide solves] linear_cg {td} p={p}: rel {e:.3e} (tolerance {tol['cg']:.0e})")
        assert x.shape == (S.shape[0], p) and e < tol["cg"]
        B = _tiled(z["csr_2d6_minres_B"], p)
        x = minres(A, torch.from_numpy(B).to(td).to(DEV), settings=MINRESSettings(minres_tolerance=1e-12))
        e = _rel(x, np.linalg.solve(S, B))
        print(f"[wide solves] minres {td} p={p}: rel {e:.3e} (tolerance {tol['minres']:.0e})")
        assert x.shape == (S.shape[0], p) and e < tol["minres"]
        B = _tiled(z["nonsym_B"], p)
        st = BICGSTABSettings(reltol=1e-12, abstol=1e-14) if tight else BICGSTABSettings()
        Bd = torch.from_numpy(B).to(td).to(DEV)
        x = bicgstab(An, Bd, settings=st)
        e = _rel(x, np.linalg.solve(Tm, B))
        print(f"[wide solves] bicgstab {td} p={p}: rel {e:.3e} (tolerance {tol['bicgstab']:.0e})")
        assert x.shape == (Tm.shape[0], p) and e < tol["bicgstab"]


@pytest.mark.parametrize("td", DTYPES)
def test_bicgstab_leading_256_columns_of_260_equal_their_own_solve_bit_for_bit(td):
    """BiCGSTAB's columns are independent problems: the leading 256 columns of the 260-column solve equal the solve of those columns
    alone, bit for bit.  The elementwise updates of a column are the same bits at every width
    (test_repeatable_and_independent_of_the_width) but its column sums are not: a workgroup of a 260-column array covers R = 12
    rows (65 lanes of 4 columns, 3 rows per pass), one of a 256-column array R = 16, so <r0, v>, |s|^2, <t, s>, <t, t>, |r|^2 would
    be associated differently and alpha, omega and the iterates would differ in their last bits (measured that way: 9.2e-6 in
    float32 at default settings, 2.3e-14 in float64).  The driver therefore solves wide right-hand sides 256 columns at a time."""
    from torchsparsegradutils_amd.utils import BICGSTABSettings, bicgstab

    z = G.load("generic_small.npz")
    Tm = z["nonsym_T"]
    An = torch.from_numpy(Tm).to(td).to(DEV).to_sparse_csr()
    Bd = torch.from_numpy(_tiled(z["nonsym_B"], 260)).to(td).to(DEV)
    st = BICGSTABSettings(reltol=1e-12, abstol=1e-14) if td == torch.float64 else BICGSTABSettings()
    x = bicgstab(An, Bd, settings=st)
    x256 = bicgstab(An, Bd[:, :256].contiguous(), settings=st)
    print(f"[wide solves] bicgstab {td}: leading 256 columns of 260 against the 256 alone: max |diff| {float((x[:, :256] - x256).abs().max()):.3e}")
    assert torch.equal(x[:, :256], x256)


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", [5, 260])
def test_linear_cg_takes_column_major_right_hand_sides(td, p):
    """The kernels work on contiguous [n][p] arrays: a right-hand side in another layout is solved as its contiguous copy, bit for bit."""
    from torchsparsegradutils_amd.utils import LinearCGSettings, linear_cg

    z = G.load("generic_small.npz")
    A = torch.from_numpy(z["S"]).to(td).to(DEV).to_sparse_csr()
    B = torch.from_numpy(_tiled(z["csr_2d6_cg_B"], p)).to(td).to(DEV)
    Bt = B.t().contiguous().t()
    assert not Bt.is_contiguous() and torch.equal(B, Bt)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        st = LinearCGSettings(cg_tolerance=1e-12)
        x, xt = linear_cg(A, B, settings=st), linear_cg(A, Bt, settings=st)
    assert torch.equal(x, xt)


@pytest.mark.parametrize("td", DTYPES)
def test_batched_right_hand_sides_fold_to_512_columns(td):
    from torchsparsegradutils_amd.utils import LinearCGSettings, linear_cg

    z = G.load("generic_small.npz")
    S = z["S"]
    A = torch.from_numpy(S).to(td).to(DEV).to_sparse_csr()
    B = np.stack([_tiled(z["csr_2d6_cg_B"], 64) * (1.0 + b) for b in range(8)])          # (8, n, 64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = linear_cg(A, torch.from_numpy(B).to(td).to(DEV), settings=LinearCGSettings(cg_tolerance=1e-12))
    e = _rel(x, np.linalg.solve(S, B))
    print(f"[wide solves] linear_cg {td} batch (8, n, 64): rel {e:.3e}")
    assert x.shape == B.shape and e < SOLVE_TOL[td]["cg"]


@pytest.mark.parametrize("td,p", [(torch.float32, 257), (torch.float32, 1028), (torch.float64, 259), (torch.float64, 514)])
def test_refused_widths_state_the_rule(td, p):
    from torchsparsegradutils_amd.utils import bicgstab, linear_cg, minres

    z = G.load("generic_small.npz")
    A = torch.from_numpy(z["S"]).to(td).to(DEV).to_sparse_csr()
    B = torch.from_numpy(_tiled(z["csr_2d6_cg_B"], p)).to(td).to(DEV)
    wide = 16 // B.element_size()
    for solver in (linear_cg, minres, bicgstab):
        if p > 1024 and solver is not linear_cg:
            continue                                                     # (those two leave the fused path above 1024 columns)
        with pytest.raises(RuntimeError, match=f"multiples of {wide} up to {256 * wide}"):
            solver(A, B)
