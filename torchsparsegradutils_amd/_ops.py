"""Kernel selection for one sparse operand.  Each product of a step — the forward, the transposed forward, the SDDMM and the
fused backward — runs on the first kernel family that the pattern and the operands qualify for, in one order of preference written
once, in `_choose`: lattice sweep / plane march (stencils on a row-major lattice), row-block tiles, row pairs (neighbouring rows
share columns: meshes, banded factors), plain gather kernels otherwise.  The families compute the same products (up to the
summation order each kernel documents); the choice is speed only.

Batched CSR operands (torch layout, equal nnz per item) that qualify for a planned family are handed to it as ONE block-diagonal
2-D problem (`_pattern.flat_of`: two vectorised adds on the index arrays, values untouched): the row-pair plans are
translation-deduplicated, so items that share a pattern also share their plan records."""

from __future__ import annotations

import os

import torch

from . import _backend as _be
from . import _cpu
from . import _lattice as _lt
from . import _pattern as _pt
from ._pattern import RowGather

# Row-pair kernels (csrc/rowpack_impl.h): rows 2q, 2q+1 walk the union of their columns, a shared dense row is
# gathered once.  First choice for forward, transposed and fused-backward walks when neighbouring rows share columns
# (stencil / banded / mesh patterns); TSGU_ENABLE_PACK=0 disables.  Small patterns stay on the plan-free kernels
# (launch-bound anyway).
ENABLE_PACK = os.environ.get("TSGU_ENABLE_PACK", "1") == "1"
PACK_MIN_NNZ = 1 << 16
# A row-pair plan costs a few device sorts: it is built when a pattern is seen for the PLAN_AFTER_USES-th time (the
# first use runs on the plan-free kernels), so that one-off patterns never pay for it.  0 = build at first sight.
PLAN_AFTER_USES = int(os.environ.get("TSGU_PLAN_AFTER_USES", "1"))
# ... and it is built on a worker thread + side stream (TSGU_PLAN_ASYNC=0: inline): the steps in between keep running
# on the plan-free kernels, no step ever waits for a plan.  `torchsparsegradutils_amd.wait_for_plans()` joins.
PLAN_ASYNC = os.environ.get("TSGU_PLAN_ASYNC", "1") == "1"


# Row-block tile kernels (csrc/tile_impl.h): general patterns whose neighbouring rows share columns (mesh orderings, banded factors,
# FEM matrices): a block's distinct dense rows are staged in LDS one block ahead of the walk.  Chosen before the row pairs when the
# pattern qualifies (every block's tile fits, entries share dense rows); TSGU_ENABLE_TILE=0 disables.
ENABLE_TILE = os.environ.get("TSGU_ENABLE_TILE", "1") == "1"
# Operands wider than one column tile (32 fp32 columns) run in ONE launch (round 6: the pipeline's steps are (block, column tile) pairs,
# a block's values / entry bytes / row pointers are staged once).  Round 5 ran one launch per column tile and kept wide operands over
# fewer than 8192 blocks on the plan-free kernels; TSGU_TILE_WIDE_MIN_BLOCKS restores such a threshold for A/B measurements.
TILE_COLUMNS = 32
TILE_WIDE_MIN_BLOCKS = int(os.environ.get("TSGU_TILE_WIDE_MIN_BLOCKS", "0"))


# Lattice plane-sweep kernels (csrc/lattice_impl.h): patterns that are stencils on a row-major lattice (what the
# reference's PairwiseEncoder and its stencil benchmarks produce) are walked tile by tile with the halo of the dense
# operand in LDS.  First choice when the pattern qualifies; anything else takes the row-pair / plan-free kernels.
ENABLE_LATTICE = os.environ.get("TSGU_ENABLE_LATTICE", "1") == "1"
# value types the sweeps are compiled for (fp32 accumulation for bf16)
LATTICE_DTYPES = (torch.float32, torch.bfloat16, torch.float64)
# measured launch configurations: every trial launch follows a 256 MB device copy (the cache state of a step, not of a back-to-back loop)
TUNE_COLD = os.environ.get("TSGU_TUNE_COLD", "1") != "0"


# ---- what a step launched ----------------------------------------------------------------------------------------------------------
# The step's C++ host path (sparse_matmul._settle_step_plan) does not decide anything a second time: the entry points below NOTE what
# they launched — family and the plan objects — with the pattern, and the host path is derived from notes that have stopped changing.
# (Round 5 re-derived the decision there and a finished-but-unclaimed row-pair future kept every tile pattern off the C++ path.)


def _note(plan: RowGather, product: str, dense: torch.Tensor, family: str, payload: tuple) -> None:
    own = plan.core.own
    sig = (dense.dtype, dense.size(-1))          # a pattern may be used with operands of several types and widths: a note is about ONE
    prev = own.get("launched_" + product)
    same = (prev is not None and prev[0] == family and prev[3] == sig and len(prev[1]) == len(payload)
            and all(a is b for a, b in zip(prev[1], payload)))
    own["launched_" + product] = (family, payload, (prev[2] + 1) if same else 1, sig)


def launched(plan: RowGather, product: str, dtype=None, p: int = 0):
    """(family, payload, consecutive steps with this very choice, (dtype, p)) of the last `product` ("fwd" / "bwd") on the pattern —
    None when there is none or (dtype given) when it was made with operands of another type or width."""
    got = plan.core.own.get("launched_" + product)
    if got is not None and dtype is not None and got[3] != (dtype, p):
        return None
    return got


def _lattice_plan(plan: RowGather, transposed: bool = False):
    """LatticePlan of the stored-order walk of the 2-D `plan` (or, `transposed`, of the walk of its transposed pattern; the
    values stay in `plan`'s stored order), None when the pattern is not a lattice stencil.  Cached with the pattern.
    Built at FIRST sight: the row kernels of csrc/lattice_plan.hip make it a few milliseconds (two passes over the
    pattern + a sort of one word per row), and the transposed walk needs no transposed pattern."""
    if (not ENABLE_LATTICE or not plan.crow.is_cuda or plan.batch is not None or plan.perm is not None or plan.nnz < PACK_MIN_NNZ
            or plan.n_rows != plan.n_cols):
        return None          # (plans exist for GPU operands only: CPU operands take _cpu.py)
    own = plan.core.own
    # a plan is built with host round trips (status words, class tables): never inside a stream capture — a pattern first
    # seen there runs on the plan-free kernels and gets its plan from the first call outside the capture
    capturing = None
    if "lattice" not in own:
        # index tensors of this geometry keep arriving with new content (_pattern._core_for): no analysis until THIS pattern has
        # come back for a third step — one-off patterns run plan-free (0.7 ms at C2) instead of paying ~11 ms of plan each
        sightings = own.get("volatile")
        if sightings is not None and sightings < 6:
            own["volatile"] = sightings + 1
            return None
        capturing = plan.crow.is_cuda and torch.cuda.is_current_stream_capturing()
        if capturing:
            return None
        own["lattice"] = _lt.build_lattice_plan_hip(plan, _be)
    fwd = own["lattice"]
    if not transposed or fwd is None:
        return fwd
    if "lattice_t" not in own:
        if capturing is None:
            capturing = plan.crow.is_cuda and torch.cuda.is_current_stream_capturing()
        if capturing:
            return None
        own["lattice_t"] = _lt.build_lattice_plan_hip(plan, _be, forward=fwd)
    return own["lattice_t"]


def _lattice_cfg(plan: RowGather, mode: int, dense: torch.Tensor, *others: torch.Tensor):
    """(LatticePlan, LatticeConfig) for these operands or None; `plan` is always the pattern the values are stored in (the
    transposed product walks its transposed pattern through the plan's own arrays)."""
    if not ENABLE_LATTICE:
        return None
    # steady state: contiguous 16-byte aligned operands of a pattern whose configuration is final — one dictionary lookup
    # (the checks below cost the host more than the launch itself, and a step asks three times)
    plain = dense.dim() == 2 and dense.is_contiguous() and dense.data_ptr() % 16 == 0
    for t in others:
        plain = plain and t.dim() == 2 and t.is_contiguous() and t.data_ptr() % 16 == 0
    memo = key = None
    if plain and plan.batch is None and plan.perm is None:
        memo = plan.core.own.get("lattice_memo")
        if memo is None:
            memo = plan.core.own["lattice_memo"] = {}
        key = (mode, dense.dtype, dense.size(-1), ENABLE_LATTICE, _lt.ENABLE_MARCH)
        hit = memo.get(key)
        if hit is not None:
            return hit
    if dense.dim() != 2 or not _be._tiled_ok(*(_be.rowmajor(t) for t in (dense,) + others)):
        return None
    if dense.dtype not in LATTICE_DTYPES:
        return None
    wide = dense.dtype == torch.float32 and dense.size(-1) > 64 and dense.size(-1) % 64 == 0     # plane march only: column tiles of 64
    if not wide and not _be.lattice_rows_fit(mode, dense.dtype, dense.size(-1)):
        return None            # dense rows the sweeps are not compiled for: do not even analyse the pattern
    fwd = _lattice_plan(plan)
    if fwd is None:
        return None
    capturing = torch.cuda.is_current_stream_capturing()
    if capturing and fwd._march is False:
        return None            # (the march tables are copied to the device when they are first derived: not inside a capture)
    # box stencils (periodic or truncated; 27-point, 7-point, triangular parts …): the plane-march kernels — all three products
    # from the stored-order plan alone
    cfg = _be.march_config(fwd, mode, dense.dtype, dense.size(-1))
    if cfg is not None:
        if memo is not None:
            memo[key] = (fwd, cfg)
        return fwd, cfg
    if wide:
        return None            # (no general-sweep form of these)
    lp = _lattice_plan(plan, transposed=True) if mode == _be.LAT_SPMMT else fwd
    if lp is None:
        return None
    if capturing and (mode, _be._VTYPE[dense.dtype], dense.size(-1)) not in lp._cfg:
        return None            # (record tables and class lists of a configuration are built with host round trips)
    cfg = _be.lattice_config(lp, mode, dense.dtype, dense.size(-1))
    if cfg is None:
        return None
    # (deterministic mode: the launch configuration — and with it the grouping of the Krylov loops' per-workgroup dot partials —
    # must not depend on a wall-clock trial; the ranked configuration stays.  TSGU_LATTICE_TUNE=0 does the same for a process)
    if _lt.TUNE and not cfg.tuned and not torch.are_deterministic_algorithms_enabled():
        cfg.uses += 1
        # (never beside a plan build on the worker's side stream: its device sorts would be in the trial timings)
        if cfg.uses >= _lt.TUNE_AFTER_USES and not torch.cuda.is_current_stream_capturing() and not _pt.plans_in_flight():
            try:
                cfg = _measured_cfg(lp, mode, dense, cfg)
            except torch.cuda.OutOfMemoryError:
                cfg.tuned = True      # no room for the trial operands: the ranked configuration stays
    if memo is not None and (cfg.tuned or not _lt.TUNE) and not torch.are_deterministic_algorithms_enabled():
        memo[key] = (lp, cfg)
    return lp, cfg


def _measured_cfg(lp, mode: int, dense: torch.Tensor, cfg):
    """The pattern keeps coming back: time the best-ranked launch configurations once on operands of the caller's shape
    (`_lattice.tune_config`; every configuration gives the same bits) and keep the fastest."""
    val = torch.zeros(lp.nnz, dtype=dense.dtype, device=dense.device)

    def run(c):
        if mode == _be.LAT_SDDMM:
            _be.csr_sddmm_lattice(lp, c, dense, dense)
        else:
            _be.csr_spmm_lattice(lp, c, val, dense)

    # Between two launches of one of these kernels a step (or a solver iteration) streams several hundred MB through the chip: what
    # the kernel finds in L2 / MALL is NOT what its own previous launch left there.  Back-to-back timings hide the difference between
    # configurations (C4's K1: 512 and 1024 threads time the same back to back, 26.6 against 31.4 us inside the CG loop), so every
    # timed launch follows a 256 MB device copy, and is timed by its own event pair.
    evict = None
    if TUNE_COLD:
        try:
            evict = (torch.empty(64 << 20, dtype=torch.float32, device=dense.device), torch.empty(64 << 20, dtype=torch.float32, device=dense.device))
        except torch.cuda.OutOfMemoryError:
            evict = None

    def time_ms(c):
        run(c)
        if evict is None:
            # the best of three timings of six launches: a single timing of four picked a 30 % slower configuration now and then
            # (clock ramps, a neighbour's launch) and the choice is final for the pattern
            best = None
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(6):
                    run(c)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / 6
                best = t if best is None or t < best else best
            return best
        pairs = []
        for _ in range(9):
            evict[1].copy_(evict[0])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(c)
            e1.record()
            pairs.append((e0, e1))
        pairs[-1][1].synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in pairs)
        return sum(ts[1:5]) / 4          # (the mean of the second to fifth fastest of nine: no ramp-up launch, no neighbour's spike)

    events, _be.KERNEL_EVENTS = _be.KERNEL_EVENTS, None      # (bench.py's per-kernel hook does not see the trial launches)
    try:
        with torch.cuda.device(dense.device):
            return _be.lattice_tune(lp, mode, dense.dtype, dense.size(-1), time_ms) or cfg
    finally:
        _be.KERNEL_EVENTS = events


def _pack_for(plan: RowGather, dense: torch.Tensor, *others: torch.Tensor, need_plain_slots: bool = False):
    """RowPackPlan of the 2-D `plan` for these dense operands, or None (disabled / not supported / not profitable /
    pattern not seen often enough yet)."""
    if (not ENABLE_PACK or not plan.crow.is_cuda or not dense.is_cuda or plan.batch is not None or dense.dim() != 2
            or plan.nnz < PACK_MIN_NNZ or plan.crow.dtype not in (torch.int32, torch.int64)):
        return None
    geo = _be.rowpack_geometry(dense.dtype, dense.size(-1))
    if geo is None or not _be._tiled_ok(*(_be.rowmajor(t) for t in (dense,) + others)):
        return None
    rpb, limits, entry_lanes = geo
    if need_plain_slots and entry_lanes > 1:
        return None  # SDDMM walks ownership-bit records (one entry lane per pair)
    if not plan.seen_enough(PLAN_AFTER_USES):
        return None
    # (deterministic mode: the step at which the kernels switch must not depend on a worker thread's timing)
    if PLAN_ASYNC and PLAN_AFTER_USES > 0 and not torch.are_deterministic_algorithms_enabled():
        return plan.rowpack_plan_async(rpb, limits, explicit_slots=entry_lanes > 1)
    return plan.rowpack_plan(rpb, limits, explicit_slots=entry_lanes > 1)


def _tile_for(plan: RowGather, dense: torch.Tensor, *others: torch.Tensor):
    """TilePlan of the 2-D `plan` for these dense operands, or None (disabled / not compiled for them / the pattern does not qualify
    or has not come back yet)."""
    if (not ENABLE_TILE or not plan.crow.is_cuda or not dense.is_cuda or plan.batch is not None or dense.dim() != 2
            or plan.nnz < PACK_MIN_NNZ or plan.crow.dtype not in (torch.int32, torch.int64)):
        return None
    geo = _be.tile_geometry(dense.dtype, dense.size(-1))
    if geo is None:
        return None
    ops = tuple(_be.rowmajor(t) for t in (dense,) + others)
    if not _be._tiled_ok(*ops) or any(t.dtype != dense.dtype or t.size(0) * max(t.stride(0), 1) * t.element_size() >= 2**32 for t in ops):
        return None
    if max(plan.n_cols, plan.n_rows) >= 1 << 24 or any(t.stride(0) * t.element_size() >= 1 << 24 for t in ops):
        return None          # (the kernels' tile row offsets are 24-bit products)
    if dense.size(-1) > TILE_COLUMNS and (plan.n_rows + geo[0] - 1) // geo[0] < TILE_WIDE_MIN_BLOCKS:
        return None          # (several column tiles over few blocks: see TILE_WIDE_MIN_BLOCKS)
    if not plan.seen_enough(PLAN_AFTER_USES):
        return None
    key = ("tile",) + tuple(geo)
    if key in plan.core.packs:
        return plan.core.packs[key]
    if torch.cuda.is_current_stream_capturing():
        return None          # (a plan is built with host reads: never inside a stream capture — asked for again after it)
    if PLAN_ASYNC and PLAN_AFTER_USES > 0 and not torch.are_deterministic_algorithms_enabled():
        return plan.tile_plan(geo, asynchronous=True)
    return plan.tile_plan(geo)


# ---- which family a product runs on ------------------------------------------------------------------------------------------------
# A step is made of up to four products: the forward A·B (FWD), the transposed forward Aᵀ·G on the transposed pattern with A's own
# values (FWD_T), the SDDMM at A's stored entries (SDDMM) and the fused backward, both gradients in one walk (BWD).  _choose() walks
# the order of preference between the kernel families once for all of them — lattice sweep / plane march -> row-block tiles -> row
# pairs -> plan-free — and the entry points below only note, launch and reshape what it returns.
FWD, FWD_T, SDDMM, BWD = 0, 1, 2, 3
LATTICE, TILES, ROW_PAIRS, PLAN_FREE = "lattice", "tiles", "row pairs", "plan-free"
_SWEEP = (_be.LAT_SPMM, _be.LAT_SPMMT, _be.LAT_SDDMM)        # the lattice mode of FWD, FWD_T and SDDMM


def _flat(x: torch.Tensor, y: torch.Tensor = None):
    """[x, y] of a batched problem as the operands of its block-diagonal 2-D form (`_pattern.flat_of`), or None when they are not
    batch-contiguous (the plain kernels then take the batch as gridDim.y).  y may be None."""
    out = [None, None]
    for i, t in enumerate((x, y)):
        if t is None:
            continue
        if t.dim() != 3:
            return None
        t = _be.rowmajor(t)
        if t.size(0) > 1 and t.stride(0) != t.size(1) * t.stride(1):
            return None
        if t.size(1) > 1 and t.stride(1) != t.size(2):
            return None
        out[i] = t.reshape(-1, t.size(-1))
    return out


def _choose(product: int, plan: RowGather, dtype: torch.dtype, x: torch.Tensor, y: torch.Tensor = None, asks: int = 1):
    """(family, payload, walked plan, x, y) of one product on GPU operands.

    `plan` is the pattern the values are stored in (FWD_T walks its transposed pattern), `dtype` the values' type (SDDMM: G's), x and
    y the dense operands in the order the plans take them — FWD: B; FWD_T: G; SDDMM: the gathered operand, the row operand; BWD: B, G.
    Batched operands come back flattened, and the walked plan is then the block-diagonal one.  The payload is what the launch reads
    and what is noted: (lattice plan, configuration) per sweep, the tile plan(s), the row-pair plan; plan-free: the transposed pattern
    when the product walks it.

    Asking has side effects, so which plans are asked for, on which pattern and in which order is part of the behaviour: _tile_for and
    _pack_for count a use of the pattern and may start a plan build, _lattice_plan counts a sighting of a volatile pattern.  `asks`:
    how often FWD_T asks for its sweep (spmm_t asks twice: the step at which a volatile pattern first runs on the lattice counts on it)."""
    batched = plan.batch is not None
    ok = x.dtype == dtype and (y is None or y.dtype == dtype)
    if product == SDDMM:
        ok = ok and plan.perm is None and not batched           # (no batched SDDMM)
    elif product != BWD:
        ok = ok and not _be.is_transposed_view(x)               # (transposed views: the plan-free kernel reads them column-strided)
    xf, yf = x, y
    if ok and batched:
        flat = _flat(x, y)
        ok = flat is not None
        if ok:
            xf, yf = flat
    # lattice sweeps / plane march: the stored-order pattern (FWD_T walks it transposed, through the same plan)
    if ok and ENABLE_LATTICE and plan.perm is None and dtype in LATTICE_DTYPES:
        src = _pt.flat_of(plan) if batched else plan
        if product == BWD:
            got = _lattice_cfg(src, _be.LAT_SDDMM, xf, yf)
            if got is not None:
                t = _lattice_cfg(src, _be.LAT_SPMMT, yf)
                if t is not None:
                    return LATTICE, got + t, src, xf, yf
        else:
            mode = _SWEEP[product]
            got = _lattice_cfg(src, mode, xf) if yf is None else _lattice_cfg(src, mode, xf, yf)
            if got is None and asks > 1:
                got = _lattice_cfg(src, mode, xf)
            if got is not None:
                return LATTICE, got, src, xf, yf
    if product == FWD_T:
        plan = plan.transposed
    # row-block tiles: a batched problem (its block-diagonal form) and the fused backward need the stored order
    if ok and (plan.perm is None or not (batched or product == BWD)) and (
            not batched or (ENABLE_TILE and _be.tile_geometry(dtype, x.size(-1)) is not None)):
        src = _pt.flat_of(plan) if batched else plan
        tp = _tile_for(src, xf) if yf is None else _tile_for(src, xf, yf)
        if product == BWD:
            tt = _tile_for(src.transposed, yf)         # (both plans are asked for before either is tested)
            if tp is not None and tt is not None:
                return TILES, (tp, tt), src, xf, yf
        elif tp is not None:
            return TILES, (tp,), src, xf, yf
    # row pairs (the fused backward walks the transposed pattern; the SDDMM only ownership-bit records, one entry lane per pair)
    if ok and (not batched or ENABLE_PACK):
        src = _pt.flat_of(plan) if batched else plan
        if product == BWD:
            src = src.transposed
            rp = _pack_for(src, yf, xf)
        elif product == SDDMM:
            rp = _pack_for(src, xf, yf, need_plain_slots=True)
            rp = rp if rp is not None and rp.upos is None else None
        else:
            rp = _pack_for(src, xf)
        if rp is not None:
            return ROW_PAIRS, (rp,), src, xf, yf
    if product == BWD:
        plan = plan.transposed
    return PLAN_FREE, (plan,) if product == FWD_T or product == BWD else (), plan, x, y


def _spmm_launch(choice, values: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """Launch a chosen FWD / FWD_T product; `B` is the caller's operand (choice[3] its flattened form for a batched problem)."""
    family, payload, src, Bf, _ = choice
    if family is PLAN_FREE:
        return _be.csr_spmm(src.crow, src.col, values, B, src.n_rows, src.n_cols, perm=src.perm, max_row_nnz=src.max_row_nnz)
    vals = values if Bf is B else values.reshape(-1)
    if family is LATTICE:
        out = _be.csr_spmm_lattice(payload[0], payload[1], vals, Bf)
    elif family is TILES:
        out = _be.csr_spmm_tile(payload[0], vals, Bf)
    else:
        out = _be.csr_spmm_rowpack(src.crow, vals, payload[0], Bf, src.n_rows)
    return out if Bf is B else out.view(B.size(0), -1, B.size(-1))


def _sddmm_launch(choice, plan: RowGather, G: torch.Tensor, B: torch.Tensor, alpha: float = 1.0, swap_roles: bool = False):
    family, payload, _, gathered, rowop = choice
    if family is LATTICE:
        return _be.csr_sddmm_lattice(payload[0], payload[1], rowop, gathered, alpha=alpha)
    if family is TILES:
        return _be.csr_sddmm_tile(payload[0], rowop, gathered, alpha=alpha)
    if family is ROW_PAIRS:
        return _be.csr_sddmm_rowpack(plan.crow, payload[0], rowop, gathered, plan.n_rows, alpha=alpha)
    return _be.csr_sddmm(plan.crow, plan.col, G, B, plan.n_rows, plan.n_cols, alpha=alpha, swap_roles=swap_roles)


def spmm(plan: RowGather, values: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A·B for the operand described by (plan, values); perm-aware (transposed / un-coalesced plans)."""
    if not B.is_cuda:
        return _cpu.spmm(plan, values, B)
    choice = _choose(FWD, plan, values.dtype, B)
    _note(plan, "fwd", B, choice[0], choice[1])
    return _spmm_launch(choice, values, B)


def spmm_t(owner: RowGather, values: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """Aᵀ·G for the operand (owner, values): the lattice sweep walks the transposed pattern through the owner's own arrays;
    everything else goes through the cached transposed pattern (built on first use)."""
    if not G.is_cuda:
        return _cpu.spmm(owner.transposed, values, G)
    return _spmm_launch(_choose(FWD_T, owner, values.dtype, G, asks=2), values, G)


def sddmm(plan: RowGather, G: torch.Tensor, B: torch.Tensor, alpha: float = 1.0, swap_roles: bool = False) -> torch.Tensor:
    """alpha·<G[row k], B[col k]> (or roles swapped) at the plan's stored entries, in plan order."""
    if not G.is_cuda:
        return _cpu.sddmm(plan, G, B, alpha=alpha, swap_roles=swap_roles)
    choice = _choose(SDDMM, plan, G.dtype, G if swap_roles else B, B if swap_roles else G)
    return _sddmm_launch(choice, plan, G, B, alpha, swap_roles)


def mm_backward(plan: RowGather, values: torch.Tensor, G: torch.Tensor, B: torch.Tensor):
    """(gradA values in A's order, gradB) of C = A·B in one pass over the transposed pattern."""
    if not G.is_cuda:       # CPU operands: the torch-op path (_cpu.py), chosen by the operands' device and nothing else
        return _cpu.sddmm(plan, G, B), _cpu.spmm(plan.transposed, values, G)
    family, payload, src, Bf, Gf = _choose(BWD, plan, values.dtype, B, G)
    _note(plan, "bwd", G, family, payload)
    vals = values if Bf is B else values.reshape(-1)
    if family is LATTICE:
        # the SDDMM in A's stored order (gradA leaves fully coalesced) and Aᵀ·G on the transposed walk of the same plan
        ga, gb = _be.csr_sddmm_lattice(payload[0], payload[1], Gf, Bf), _be.csr_spmm_lattice(payload[2], payload[3], vals, Gf)
    elif family is TILES:
        # the SDDMM on the stored pattern's tiles + the transposed product on the transposed pattern's tiles (A's own values)
        ga, gb = _be.csr_sddmm_tile(payload[0], Gf, Bf), _be.csr_spmm_tile(payload[1], vals, Gf)
    elif family is ROW_PAIRS and payload[0].srcstart is not None and plan.batch is None and plan.perm is None:
        # the transposed plan reached the dictionary form through row-relative value positions (mesh orderings): the SDDMM on the
        # stored-order plan + the transposed product beat the fused walk (mesh27_blocked: 124 + 208 us against 417 us)
        return sddmm(plan, G, B), _spmm_launch(_choose(FWD_T, plan, values.dtype, G), values, G)
    elif family is ROW_PAIRS:
        ga, gb = _be.csr_mm_backward_rowpack(src.crow, payload[0], vals, Gf, Bf, src.n_rows)
    else:
        return _be.csr_mm_backward(src, values, G, B, plan.n_rows, plan.n_cols)
    return (ga, gb) if Bf is B else (ga.view(values.shape), gb.view(B.shape))


def mm_backward_separate(plan: RowGather, values: torch.Tensor, G: torch.Tensor, B: torch.Tensor):
    """(gradA values in A's order, gradB) as TWO products — the SDDMM in stored order and Aᵀ·G — for operands the fused walk is not
    compiled for (fp64, very wide rows).  Noted like mm_backward when both products ran on the same family."""
    if not G.is_cuda:
        return sddmm(plan, G, B), spmm_t(plan, values, G)
    a = _choose(SDDMM, plan, G.dtype, B, G)
    ga = _sddmm_launch(a, plan, G, B)
    b = _choose(FWD_T, plan, values.dtype, G, asks=2)
    gb = _spmm_launch(b, values, G)
    if a[0] is b[0]:
        _note(plan, "bwd", G, a[0], a[1] + b[1])
    return ga, gb
