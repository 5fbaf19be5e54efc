"""The plan kernel families called directly (`_backend`), in every plan form, against the float64 restatement of tests/_csr_ref.py:
the row-pair union walk (csr_spmm_rowpack, csr_sddmm_rowpack, csr_mm_backward_rowpack; csrc/rowpack_impl.h) and the row-block tiles
(csr_spmm_tile, csr_sddmm_tile; csrc/tile_impl.h).  These are what a sparse_mm step runs on a pattern it has seen before.

Cases (tests/_plan_cases.py; their claims — which staging chunk, capacity, residue of the unrolled walk, pipeline depth a case reaches —
are asserted on the host by test_plan_cases_cpu.py from the plans' own arrays).  The plans are built on the CPU, exactly as that module
checks them, and copied to the device.

A. Row pairs: the 8 lane geometries (float32 p = 8, 16, 32, 64 and bfloat16 p = 16, 32, 64, 128: 2×4, 4×2, 8×1, 16×1 column × entry
lanes) × 20 patterns.  Each pattern runs in every walk that compiles for the geometry — stored order with ownership bits (SpMM, SDDMM;
8 and 16 column lanes), stored order with slot words (SpMM), the permuted walk of a transposed pattern (SpMM, fused backward), and on
the two lattices the same with brick ownership — in stream and dictionary form, with int32 and int64 row pointers.
B. Tiles (float32): a composite of blocks on the kernel's limits (224 distinct columns with 1792 entries, an empty block, one row of
224 entries, row lengths around the rounds of eight, lists of 1, 7, 8, 9 columns, a ragged partial block), an empty first / last
block, fewer than 64 rows, blocks of 511, 512, 513 and 1024 value chunks, p = 32, 64, 96 and 1024, and the persistent pipeline: 3·S + 3
blocks for the S = 2 · compute units workgroups of the launch, so that every workgroup stages block k + 1 while it walks block k.

Exact: values and operands are integers in [−3, 3]; every product and sum is exact in float32, so C, gradB, gradA and the SDDMM (alpha
−1 and 2) must EQUAL the restatement, a bfloat16 result the exact value rounded once.
Bounded: random data, exact in bfloat16, so that one reference serves both types; u = 2^-24, γ_k = k·u / (1 − k·u).
  an element of C or gradB from a row of L entries   γ_L · Σ|terms|   (any order of L fused multiply-adds: serial, dealt round-robin
                                                                       to the entry lanes and folded, plane-rotated in bricks)
  an entry of gradA or of the SDDMM                  γ_{p+1} · Σ|terms|   (p fused terms in any tree, and the product with alpha)
  a bfloat16 result                                  + 2^-8 (|exact| + bound)
These bounds are derived, not measured.  Every comparison prints max |err| / bound, the module's fixture the largest per kernel and type when the module is done.
Identical bits: stream and dictionary form of one walk; the same plan with `order` (which the kernel honours and no builder sets) a
random permutation of the workgroups; int32 and int64 row pointers; operands that are column slices of a wider buffer; with one entry
lane and consecutive pairs, the forward and csr_spmm, the permuted walk and csr_spmm(perm=...); gradB of the fused backward and the
permuted SpMM; two launches of a tile kernel; the tile SpMM and Aᵀ·G and csr_spmm.
Non-finite: a NaN row of the gathered operand reaches exactly the rows and entries that reference it, in all three modes.

TSGU_TILE_CYCLIC=0 (runs of consecutive blocks per workgroup instead of the cyclic schedule) is read once per process by the launcher;
it is out of scope here: every test of this module runs the default, cyclic schedule.

Largest |err| / bound on an MI355X, float32 / bfloat16 (bfloat16: the final rounding alone comes to 1 / (1 + 2^-8) = 0.996):
  csr_spmm_rowpack 0.47 / 0.996   csr_sddmm_rowpack 0.024 / 0.982   csr_mm_backward_rowpack gradB 0.47 / 0.996, gradA 0.13 / 0.994
  csr_spmm_tile 0.49, through value chunks 0.29   csr_sddmm_tile 0.024
The module's 195 tests take 5 s together, the two pipeline cases 0.6 s and 1.0 s of it.  No kernel or builder bug was found.
"""

import time

import numpy as np
import pytest
import torch

import _csr_ref as cr
import _plan_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24
RATIOS = {}
_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    """The module's set-up and its report: whatever subset of the tests ran, in whatever order, the largest |err| / bound per kernel
    and value type and the wall time between the first test and the last are printed when the module is done (shown with -s)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _be().load_library()
    t0 = time.perf_counter()
    yield
    for key in sorted(RATIOS):
        print(f"\nlargest |err| / bound  {key[0]:28s} {key[1]:5s} {RATIOS[key]:.4f}", end="")
    print(f"\nmodule wall time {time.perf_counter() - t0:.1f} s")
    _CASES.clear()       # (the cases' device plans)
    RATIOS.clear()


def _be():
    from torchsparsegradutils_amd import _backend

    return _backend


# ---- operands and comparisons -------------------------------------------------------------------------------------------------------

def _values(rng, shape, ints):
    """float64 values exact in bfloat16: integers in [−3, 3], or uniform in (−1, 1) rounded to bfloat16."""
    if ints:
        return rng.integers(-3, 4, shape).astype(np.float64)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, shape)).to(torch.bfloat16).double().numpy()


def _dev(x, dtype, sliced=False):
    """x on the device; sliced: as a column slice of a buffer one 16-byte lane wider, one lane from its start."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    if not sliced:
        return t.to(DEV)
    lane = 16 // t.element_size()
    buf = torch.full((t.shape[0], t.shape[1] + lane), 7.0, dtype=dtype, device=DEV)
    view = buf[:, lane:]
    view.copy_(t)
    assert not view.is_contiguous() or t.shape[0] <= 1
    return view


def _index(a, itype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(itype).to(DEV)


def _stored(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).double().numpy()


def _host(t):
    return t.double().cpu().numpy()


def _gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def _same(what, got, want):
    bad = np.flatnonzero((got != want).reshape(-1))
    assert got.shape == want.shape and not len(bad), \
        f"{what}: {len(bad)} of {got.size} elements differ, the first at {np.unravel_index(bad[0], got.shape)}: " \
        f"{got.reshape(-1)[bad[0]]} for {want.reshape(-1)[bad[0]]}"


def _hold(kernel, dtype, what, got, ref, abs_terms, count):
    """|got − ref| <= γ_count Σ|terms| elementwise (bfloat16: + 2^-8 (|ref| + that)); where the bound is zero, equality."""
    bound = _gamma(count) * abs_terms
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)
    err = np.abs(got - ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    zero = bound == 0
    assert (err[zero] == 0).all(), f"{what}: an element with no terms is not zero"
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    key = (kernel, "bf16" if dtype == torch.bfloat16 else "f32")
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"{kernel} {key[1]} {what}: max |err| / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: |err| / bound = {ratio}"


# ---- A. row pairs -------------------------------------------------------------------------------------------------------------------

def _rowpack(geo, name):
    key = (pc.rpb_of(geo), geo.ep == 1, name)
    if key not in _CASES:
        case = pc.rowpack_case(name, pc.rpb_of(geo))
        plans = {k: pc.plan_to(v, DEV) for k, v in pc.rowpack_plans(case, geo).items()}
        _CASES[key] = (case, plans, pc.gathers(case)[3])
    return _CASES[key]


def test_the_geometry_table_is_the_library_s():
    for g in pc.GEOS:
        assert _be().rowpack_geometry(g.dtype, g.p) == (pc.rpb_of(g), pc.LIMITS, g.ep)
    for p in (32, 64, 96, 1024):
        assert _be().tile_geometry(torch.float32, p) == pc.TILE_GEO


def _launch(mode, plan, crow, n, val, S, own, alpha=1.0):
    be = _be()
    if mode == pc.SPMM:
        return (be.csr_spmm_rowpack(crow, val, plan, S, n),)
    if mode == pc.BWD:
        return be.csr_mm_backward_rowpack(crow, plan, val, S, own, n)
    return (be.csr_sddmm_rowpack(crow, plan, own, S, n, alpha=alpha),)


def _identical_bits(what, rng, first, key, plan, out, crows, n, vd, dense, sliced):
    """`out` again: from the other plan form of the same walk (`first` keeps the first form's result per key), with int64 row pointers,
    with the operands as column slices of a wider buffer, and with the workgroups in a random order."""
    mode, alpha = key[0], key[2]
    if key in first:
        for a, b in zip(out, first[key]):
            assert torch.equal(a, b), what + ": the two plan forms differ"
    else:
        first[key] = out
    for a, b in zip(_launch(mode, plan, crows[torch.int64], n, vd, *dense, alpha), out):
        assert torch.equal(a, b), what + ": int64 row pointers"
    for a, b in zip(_launch(mode, plan, crows[torch.int32], n, vd, *sliced, alpha), out):
        assert torch.equal(a, b), what + ": operands as column slices"
    if plan.nblocks > 1:
        shuffled = pc.plan_to(plan, DEV)
        shuffled.order = _index(rng.permutation(plan.nblocks), torch.int32)
        for a, b in zip(_launch(mode, shuffled, crows[torch.int32], n, vd, *dense, alpha), out):
            assert torch.equal(a, b), what + ": workgroups in another order"


@pytest.mark.parametrize("name", pc.ROWPACK_NAMES)
@pytest.mark.parametrize("geo", pc.GEOS, ids=pc.GEO_IDS)
def test_rowpack_kernels(geo, name):
    case, plans, perm = _rowpack(geo, name)
    n, m, p, dtype = case.n, case.m, geo.p, geo.dtype
    rng = np.random.default_rng(17)
    crows = {it: _index(case.crow, it) for it in (torch.int32, torch.int64)}
    col32 = _index(case.col, torch.int32)
    permd = _index(perm, torch.int32)
    for ints in (True, False):
        val, S, own = _values(rng, len(case.col), ints), _values(rng, (m, p), ints), _values(rng, (n, p), ints)
        vd, Sd, od = _dev(val, dtype), _dev(S, dtype), _dev(own, dtype)
        Ss, os_ = _dev(S, dtype, sliced=True), _dev(own, dtype, sliced=True)
        kind = "exact" if ints else "random"
        ref = {False: cr.spmm(case.crow, case.col, val, S), True: cr.spmm(case.crow, case.col, val, S, perm)}
        ref_abs = {False: cr.spmm_abs(case.crow, case.col, val, S), True: cr.spmm_abs(case.crow, case.col, val, S, perm)}
        dots, dots_abs = cr.sddmm(case.crow, case.col, own, S, 1.0), cr.sddmm_abs(case.crow, case.col, own, S, 1.0)
        first = {}
        for (mode, walk, form) in pc.launches(plans):
            plan = plans[walk, form]
            permuted = walk in ("perm", "brick")
            alphas = (-1.0, 2.0) if mode == pc.SDDMM else (1.0,)
            for alpha in alphas:
                what = f"{name} {pc.GEO_IDS[pc.GEOS.index(geo)]} mode {mode} {walk} {form} alpha {alpha} {kind}"
                out = _launch(mode, plan, crows[torch.int32], n, vd, Sd, od, alpha)
                # -- against float64
                if mode == pc.SDDMM:
                    got, want, terms = _host(out[0]), alpha * dots, abs(alpha) * dots_abs
                    if ints:
                        _same(what, got, _stored(want, dtype))
                    else:
                        _hold("sddmm_rowpack", dtype, what, got, want, terms, p + 1)
                else:
                    got = _host(out[-1])
                    if ints:
                        _same(what, got, _stored(ref[permuted], dtype))
                    else:
                        _hold("spmm_rowpack" if mode == pc.SPMM else "backward_rowpack gradB", dtype, what, got, ref[permuted],
                              ref_abs[permuted], case.lens[:, None])
                    if mode == pc.BWD:
                        want, terms = np.empty(len(perm)), np.empty(len(perm))
                        want[perm], terms[perm] = dots, dots_abs
                        if ints:
                            _same(what + " gradA", _host(out[0]), _stored(want, dtype))
                        else:
                            _hold("backward_rowpack gradA", dtype, what + " gradA", _host(out[0]), want, terms, p + 1)
                _identical_bits(what, rng, first, (mode, walk, alpha), plan, out, crows, n, vd, (Sd, od), (Ss, os_))
        # -- the same sums as the plan-free kernels (one entry lane, consecutive pairs), and as each other
        be = _be()
        if geo.ep == 1:
            plain = be.csr_spmm(crows[torch.int32], col32, vd, Sd, n, m)
            assert torch.equal(first[pc.SPMM, "bits", 1.0][0], plain) and torch.equal(first[pc.SPMM, "slots", 1.0][0], plain), kind
            assert torch.equal(first[pc.SPMM, "perm", 1.0][0], be.csr_spmm(crows[torch.int32], col32, vd, Sd, n, m, perm=permd)), kind
        assert torch.equal(first[pc.BWD, "perm", 1.0][1], first[pc.SPMM, "perm", 1.0][0]), kind
        if case.brick is not None:
            assert torch.equal(first[pc.BWD, "brick", 1.0][1], first[pc.SPMM, "brick", 1.0][0]), kind
            assert torch.equal(first[pc.BWD, "brick", 1.0][0], first[pc.BWD, "perm", 1.0][0]), kind + ": the dots do not depend on the walk"


@pytest.mark.parametrize("name", ["rows-3R+1", "brick-3d"])
@pytest.mark.parametrize("geo", pc.GEOS, ids=pc.GEO_IDS)
def test_rowpack_non_finite_rows_reach_what_references_them_and_nothing_else(geo, name):
    """One NaN row of the gathered operand.  SpMM and the fused backward: exactly the output rows that reference it (the second row
    of a pair is predicated, not multiplied by zero); gradA and the SDDMM: exactly the entries of that column.  On the lattice also
    through the brick plans, whose records are listed plane by plane."""
    case, plans, perm = _rowpack(geo, name)
    n, m, p, dtype = case.n, case.m, geo.p, geo.dtype
    rng = np.random.default_rng(23)
    rows = np.repeat(np.arange(n), np.diff(case.crow))
    # a column that one row of a pair references and the other does not
    bad = next(j for j in range(m) if any((r ^ 1) < n and (r ^ 1) not in set(rows[case.col == j]) for r in rows[case.col == j]))
    hit_entries = case.col == bad
    hit_rows = np.zeros(n, dtype=bool)
    hit_rows[rows[hit_entries]] = True
    assert 0 < hit_rows.sum() < n
    val, S, own = _values(rng, len(case.col), False), _values(rng, (m, p), False), _values(rng, (n, p), False)
    S[bad] = np.nan
    vd, Sd, od = _dev(val, dtype), _dev(S, dtype), _dev(own, dtype)
    crow = _index(case.crow, torch.int32)
    for (mode, walk, form) in pc.launches(plans):
        out = _launch(mode, plans[walk, form], crow, n, vd, Sd, od, -1.0)
        what = f"mode {mode} {walk} {form}"
        if mode == pc.SDDMM:
            assert np.array_equal(np.isnan(_host(out[0])), hit_entries), what
            continue
        nan = np.isnan(_host(out[-1]))
        assert np.array_equal(nan, np.broadcast_to(hit_rows[:, None], nan.shape)), what
        if mode == pc.BWD:
            want = np.zeros(len(perm), dtype=bool)
            want[perm] = hit_entries
            assert np.array_equal(np.isnan(_host(out[0])), want), what


# ---- B. tiles -----------------------------------------------------------------------------------------------------------------------

def _tile(name, S=None):
    key = ("tile", name)
    if key not in _CASES:
        case = pc.pipeline_case(S) if name == "pipeline" else pc.tile_case(name)
        fwd, back, walk = pc.tile_plans(case)
        assert fwd is not None and back is not None, f"{name}: the builder refused the pattern"
        _CASES[key] = (case, pc.plan_to(fwd, DEV), pc.plan_to(back, DEV), walk)
    return _CASES[key]


def _tile_checks(name, case, fwd, back, walk, p, random=True):
    be = _be()
    rng = np.random.default_rng(29 + p)
    dtype = torch.float32
    n, m = case.n, case.m
    wcrow, wcol, wperm = walk
    wn = len(wcrow) - 1                      # rows of the permuted walk: m for a transpose (its operand has n rows), n for a permuted W
    wm = n if case.perm is None else m
    crow, col = _index(case.crow, torch.int32), _index(case.col, torch.int32)
    wc, wi, wp = _index(wcrow, torch.int32), _index(wcol, torch.int32), _index(wperm, torch.int32)
    wlens = np.diff(wcrow)
    for ints in ((True, False) if random else (True,)):
        val, B, G, R = (_values(rng, s, ints) for s in (len(case.col), (m, p), (wm, p), (n, p)))
        vd, Bd, Gd, Rd = (_dev(x, dtype) for x in (val, B, G, R))
        what = f"tile {name} p={p} {'exact' if ints else 'random'}"
        C = be.csr_spmm_tile(fwd, vd, Bd)
        T = be.csr_spmm_tile(back, vd, Gd)
        ref_c, ref_t = cr.spmm(case.crow, case.col, val, B), cr.spmm(wcrow, wcol, val, G, wperm)
        assert C.shape == (n, p) and T.shape == (wn, p)
        if ints:
            _same(what + " SpMM", _host(C), ref_c)
            _same(what + " permuted SpMM", _host(T), ref_t)
        else:
            _hold("spmm_tile", dtype, what + " SpMM", _host(C), ref_c, cr.spmm_abs(case.crow, case.col, val, B), case.lens[:, None])
            _hold("spmm_tile permuted", dtype, what + " permuted SpMM", _host(T), ref_t, cr.spmm_abs(wcrow, wcol, val, G, wperm), wlens[:, None])
            assert torch.equal(C, be.csr_spmm(crow, col, vd, Bd, n, m)), what + ": not the bits of csr_spmm"
            assert torch.equal(T, be.csr_spmm(wc, wi, vd, Gd, wn, wm, perm=wp)), what + ": not the bits of csr_spmm(perm)"
        assert torch.equal(C, be.csr_spmm_tile(fwd, vd, Bd)) and torch.equal(T, be.csr_spmm_tile(back, vd, Gd)), what + ": two launches differ"
        for alpha in (-1.0, 2.0):
            D = be.csr_sddmm_tile(fwd, Rd, Bd, alpha=alpha)
            want = cr.sddmm(case.crow, case.col, R, B, alpha)
            if ints:
                _same(what + f" SDDMM alpha {alpha}", _host(D), want)
            else:
                _hold("sddmm_tile", dtype, what + f" SDDMM alpha {alpha}", _host(D), want, cr.sddmm_abs(case.crow, case.col, R, B, alpha), p + 1)
            assert torch.equal(D, be.csr_sddmm_tile(fwd, Rd, Bd, alpha=alpha)), what + ": two launches differ"


@pytest.mark.parametrize("p", [32, 64, 96])
@pytest.mark.parametrize("name", [k for k in pc.TILE_NAMES if k != "p1024"])
def test_tile_kernels(name, p):
    _tile_checks(name, *_tile(name), p)


def test_tile_kernels_32_column_tiles():
    _tile_checks("p1024", *_tile("p1024"), 1024)


@pytest.mark.parametrize("p", [32, 64])
def test_tile_persistent_pipeline(p):
    """3·S + 3 blocks for S = 2 · compute units persistent workgroups: 4 blocks per workgroup by the launcher's arithmetic, so every
    workgroup stages block k + 1 (and, with two column tiles, the next tile of block k) while it walks block k; every fifth block is
    empty.  Integer data: the results must equal the restatement."""
    S = 2 * _be().device_cu_count()
    case, fwd, back, walk = _tile("pipeline", S)
    assert fwd.n_blocks == 3 * S + 3 and -(-fwd.n_blocks // S) == 4
    _tile_checks("pipeline", case, fwd, back, walk, p, random=False)
