"""Patterns, plans and a host emulation for the tests of the plan kernel families: the row-pair union walk (csrc/rowpack_impl.h, plans
from _pattern.build_rowpack_plan) and the row-block tiles (csrc/tile_impl.h, plans from _tile.build_tile_plan).  Host only: numpy,
torch on the CPU and the two plan builders, which are index arithmetic.  Nothing here loads the library or reads oracle/.

The float64 references are those of tests/_csr_ref.py (`spmm`, `sddmm`, `backward`, the `*_abs` forms, `transpose`).

A case is ONE walked pattern W (n × m) and the claim it is built for.  Every walk runs on it:
  stored order      W's values in W's order: ownership-bit records, or explicit slot words (`explicit_slots`)
  permuted          W is the transpose of A (m × n) and its values are A's, read through `perm` — what the library builds for Aᵀ·G
so that a structure (a lone last row, an empty workgroup, 2048 values in one workgroup, ...) is reached by every kernel instantiation
and not only by the one whose pattern happens to have it.  Both plan builders refuse patterns without sharing (row pairs need 1.2
stored entries per union entry, tiles 2.0 per distinct column of a block), so the rows of a pair / a block draw their columns from a
common POOL (`draw`).  A claim is computed from the built plan's own arrays (`rowpack_facts`, `tile_facts`), never from the intention.

`walk_rowpack` restates the row-pair kernel's phases in float64 on the STREAM arrays of a plan (a dictionary plan goes through
_pattern.expand_classes first): stage the workgroup's values through sperm / eptr or the row pointer, walk every slot's union records,
apply slot words or ownership bits with running counters.  On integer data it must equal the plain restatement exactly; a GPU failure
next to a passing walk is the kernel's, next to a failing walk the plan builder's.
"""

import collections
import copy

import numpy as np
import torch

import _csr_ref as cr
from torchsparsegradutils_amd import _pattern, _tile
from torchsparsegradutils_amd.utils import synthetic

# ---- the geometry table of the row-pair kernels (rp_geom in csrc/rowpack_impl.h; the GPU module asserts it against the library) ----
BLOCK = 256
LIMITS = (2048, 3072, 64 * 1024)          # staged values, union records, LDS bytes per workgroup
Geo = collections.namedtuple("Geo", "dtype p cl ep")
GEOS = [Geo(torch.float32, 8, 2, 4), Geo(torch.float32, 16, 4, 2), Geo(torch.float32, 32, 8, 1), Geo(torch.float32, 64, 16, 1),
        Geo(torch.bfloat16, 16, 2, 4), Geo(torch.bfloat16, 32, 4, 2), Geo(torch.bfloat16, 64, 8, 1), Geo(torch.bfloat16, 128, 16, 1)]
GEO_IDS = [f"{'f32' if g.dtype == torch.float32 else 'bf16'}-p{g.p}-{g.cl}x{g.ep}" for g in GEOS]
TILE_GEO = (64, 224, 1792)                # rows per block, distinct columns, entries (tsgu_tile_geometry)
TILE_CHUNKS = 1024                        # value chunks per block (kTileCP = 2 per thread)

SPMM, BWD, SDDMM = 0, 1, 2


def rpb_of(geo):
    return 2 * (BLOCK // (geo.cl * geo.ep))


def unroll_of(geo, mode):
    """Gathers in flight per lane (U of csr_rowpack_kernel): 4, and 3 in the bfloat16 backward."""
    return 3 if (mode == BWD and geo.dtype == torch.bfloat16) else 4


Case = collections.namedtuple("Case", "name crow col n m lens brick")


# ---- drawing columns from pools -----------------------------------------------------------------------------------------------------

def draw(rng, lens, pool_start, pool_size, start=None):
    """(crow, col): row i has lens[i] distinct ascending columns pool_start[i] + j, j < pool_size[i].  start[i] >= 0: the cyclic window
    of lens[i] pool positions from start[i] (rows with start = i·L cover the pool in turn); otherwise a random subset."""
    lens, pool_start, pool_size = (np.asarray(a, dtype=np.int64) for a in (lens, pool_start, pool_size))
    n = len(lens)
    assert (lens <= pool_size).all()
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if crow[-1] == 0:
        return crow, np.zeros(0, dtype=np.int64)
    width = int(pool_size.max())
    j = np.arange(width)[None, :]
    keys = rng.random((n, width))
    if start is not None:
        start = np.asarray(start, dtype=np.int64)
        cyc = ((j - start[:, None]) % np.maximum(pool_size, 1)[:, None]).astype(np.float64)
        keys = np.where(start[:, None] >= 0, cyc, keys)
    keys = np.where(j < pool_size[:, None], keys, np.inf)
    rank = np.argsort(np.argsort(keys, axis=1, kind="stable"), axis=1, kind="stable")
    rows, pos = np.nonzero(rank < lens[:, None])
    return crow, pool_start[rows] + pos


def _transposed(crow, col, m):
    """A = Wᵀ as CSR (acrow, acol) and `perm`: entry e of W is A's value perm[e]."""
    acrow, acol, aperm = cr.transpose(crow, col, m)
    perm = np.empty(len(col), dtype=np.int64)
    perm[aperm] = np.arange(len(col))
    return acrow, acol, perm


# ---- A. row-pair cases --------------------------------------------------------------------------------------------------------------

def _pairs(name, rng, lens, slack=1, cover=False, hub=False):
    """Rows 2q and 2q+1 draw from pool q: max(len) + slack columns from column 2q on (the pools of neighbouring pairs overlap).
    cover: no slack, and a row as long as its pool takes all of it, so the pair's union IS the pool.  hub: one more column that every
    row references (as a row of A: a source row of n entries)."""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    q = np.arange(n) // 2
    both = np.zeros(2 * ((n + 1) // 2), dtype=np.int64)
    both[:n] = lens
    pool = both.reshape(-1, 2).max(1) + (0 if cover else slack)
    m = n + int(pool.max()) + 5
    crow, col = draw(rng, lens, 2 * q, pool[q])
    if hub:
        rows = np.repeat(np.arange(n), lens)
        col = np.concatenate([col, np.full(n, m)])
        rows = np.concatenate([rows, np.arange(n)])
        o = np.lexsort((col, rows))
        col, lens, m = col[o], lens + 1, m + 1
        crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Case(name, crow, col, n, m, lens, None)


def _spread(total, k):
    """k non-negative lengths that sum to `total`, as even as possible."""
    out = np.full(k, total // k, dtype=np.int64)
    out[:total % k] += 1
    return out


ROWPACK_NAMES = (["rows-2", "rows-3", "rows-R-1", "rows-R+1", "rows-3R+1", "single-column", "holes", "ne-255", "ne-256", "ne-257",
                  "cap-2048", "nu-256", "nu-257", "nu-512", "nu-513", "ucap-max", "residues", "hub", "brick-3d", "brick-2d"])


def rowpack_case(name, R):
    """The walked pattern of case `name` for workgroups of R rows."""
    rng = np.random.default_rng(1000 + ROWPACK_NAMES.index(name))
    if name.startswith("rows-"):
        n = {"2": 2, "3": 3, "R-1": R - 1, "R+1": R + 1, "3R+1": 3 * R + 1}[name[5:]]
        return _pairs(name, rng, rng.integers(2, 7, n))
    if name == "single-column":
        # A is ONE row of 36 entries (n = 1: no sharing, the forward plan is refused); W = Aᵀ has one entry per row, all in column 0
        lens = np.ones(37, dtype=np.int64)
        lens[5] = 0
        crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        return Case(name, crow, np.zeros(36, dtype=np.int64), 37, 1, lens, None)
    if name == "holes":
        # pairs (empty, empty), (5, empty), (empty, 5) in the first workgroup; the whole second workgroup empty; a full third one
        lens = np.full(3 * R, 5, dtype=np.int64)
        lens[R:2 * R] = 0
        lens[[2, 3, 5, 6]] = 0
        return _pairs(name, rng, lens)
    if name.startswith("ne-"):
        return _pairs(name, rng, np.concatenate([_spread(int(name[3:]), R), [3, 3]]))
    if name == "cap-2048":
        return _pairs(name, rng, np.concatenate([np.full(R, 2048 // R), [3, 3]]), cover=True)
    if name == "ucap-max":
        # The builder asks for 1.2 stored entries per union record over the WHOLE pattern, not per workgroup: a first workgroup of
        # 2048 entries whose pairs share nothing (row 2q the first half of its pool, row 2q+1 the second) has 2048 union records, and
        # three workgroups of pairs that share everything lift the pattern's figure to 1.43.  nu <= ne <= 2048 in any workgroup.
        L = 2048 // R
        lens = np.concatenate([np.full(R, L), np.full(3 * R, L // 2)])
        n = 4 * R
        q, first = np.arange(n) // 2, np.arange(n) < R
        crow, col = draw(rng, lens, 2 * q, np.where(first, 2 * L, L // 2), np.where(first, (np.arange(n) % 2) * L, 0))
        return Case(name, crow, col, n, n + 2 * L + 5, lens, None)
    if name.startswith("nu-"):
        pool = _spread(int(name[3:]), R // 2)
        lens = np.stack([pool, pool // 2], 1).reshape(-1)
        return _pairs(name, rng, lens, cover=True)
    if name == "residues":
        pool = np.arange(36)
        return _pairs(name, rng, np.stack([pool, pool // 2], 1).reshape(-1), cover=True)
    if name == "hub":
        return _pairs(name, rng, rng.integers(2, 5, 259), hub=True)
    dims = (7, 5, 6) if name == "brick-3d" else (1, 37, 26)
    if name == "brick-3d":
        crow, col = synthetic.stencil27_periodic(*dims, torch.int32)
    else:
        crow, col, _ = synthetic.laplacian7(*dims)
    n = dims[0] * dims[1] * dims[2]
    acrow, acol = crow.numpy().astype(np.int64), col.numpy().astype(np.int64)
    wcrow, wcol, _ = cr.transpose(acrow, acol, n)
    return Case(name, wcrow, wcol, n, n, np.diff(wcrow), dims)


def gathers(case, itype=torch.int64, device="cpu"):
    """(stored-order RowGather of W, permuted RowGather of W = Aᵀ, RowGather of A, perm)."""
    acrow, acol, perm = _transposed(case.crow, case.col, case.m)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(itype).to(device)  # noqa: E731
    nat = _pattern.RowGather(t(case.crow), t(case.col), case.n, case.m)
    per = _pattern.RowGather(t(case.crow), t(case.col), case.n, case.m, perm=t(perm))
    a = _pattern.RowGather(t(acrow), t(acol), case.m, case.n)
    return nat, per, a, perm


# the plan forms of a case: (walk, form) -> keyword arguments of build_rowpack_plan
FORMS = ("stream", "dictionary")


def rowpack_plans(case, geo):
    """{(walk, form): plan} on the CPU.  "bits": stored order with ownership bits (kernels with one entry lane, CL 8 and 16);
    "slots": stored order with explicit slot words; "perm": the transposed walk; "brick": the transposed walk with brick ownership
    (lattice cases).  A refusal by the builder is an error: every case the GPU module runs has a plan."""
    R = rpb_of(geo)
    nat, per, _, _ = gathers(case)
    plans = {}
    for form in FORMS:
        dedup = "off" if form == "stream" else "force"
        if geo.ep == 1:
            plans["bits", form] = _pattern.build_rowpack_plan(nat, R, LIMITS, dedup=dedup)
        plans["slots", form] = _pattern.build_rowpack_plan(nat, R, LIMITS, explicit_slots=True, dedup=dedup)
        plans["perm", form] = _pattern.build_rowpack_plan(per, R, LIMITS, dedup=dedup)
        if case.brick is not None:
            lat = _pattern.detect_lattice(per)
            assert lat is not None, f"{case.name}: no lattice detected"
            po = _pattern.brick_pair_order(case.n, lat, R // 2, "cpu")
            assert po is not None and bool((po < 0).any()), f"{case.name}: the brick divides the lattice"
            plans["brick", form] = _pattern.build_rowpack_plan(per, R, LIMITS, pair_order=po, lattice=lat, dedup=dedup)
    for key, plan in plans.items():
        assert plan is not None, f"{case.name} {key}: the builder refused the pattern"
        assert (plan.nclasses > 0) == (key[1] == "dictionary"), f"{case.name} {key}: the wrong plan form"
    return plans


MODES_OF_WALK = {"bits": (SPMM, SDDMM), "slots": (SPMM,), "perm": (SPMM, BWD), "brick": (SPMM, BWD)}


def launches(plans):
    """(mode, walk, form) of every launch the GPU module makes for a case's plans: the kernel instantiations of csr_rowpack_kernel
    reachable through the C ABI — SpMM and SDDMM in stored order with ownership bits, SpMM in stored order with slot words, SpMM
    and the fused backward through the permutation (consecutive pairs, or bricks) — each in both plan forms."""
    return [(mode, walk, form) for (walk, form) in plans for mode in MODES_OF_WALK[walk]]


def instantiations(geo):
    """What the cases of one geometry must launch between them."""
    walks = (["bits"] if geo.ep == 1 else []) + ["slots", "perm", "brick"]
    return {(mode, walk, form) for walk in walks for form in FORMS for mode in MODES_OF_WALK[walk]}


def plan_to(plan, device):
    """A fresh copy of a plan (row-pair or tile) with its arrays on `device` and no cached struct."""
    out = copy.copy(plan)
    for k in type(plan).__slots__:
        v = getattr(plan, k)
        if torch.is_tensor(v):
            setattr(out, k, v.to(device))
    out._cstruct = None
    return out


def stream_arrays(plan):
    """(uptr, ucol, upos, sperm, vpair, eptr) as int64 numpy arrays (None where the plan has none), a dictionary plan expanded."""
    if plan.nclasses > 0:
        arrays = _pattern.expand_classes(plan)
    else:
        arrays = (plan.uptr, plan.ucol, plan.upos, plan.sperm, plan.vpair, plan.eptr)
    return tuple(None if a is None else (a.cpu().numpy().astype(np.int64) & (0xFFFFFFFF if k in (1, 2) else -1)) for k, a in enumerate(arrays))


def rowpack_facts(plan, crow, n):
    """What the plan's own arrays say a launch does: values and union records per workgroup, union length per lane-group slot."""
    uptr, ucol, upos, sperm, vpair, eptr = stream_arrays(plan)
    gpb, nb, R = plan.gpb, plan.nblocks, plan.rpb
    if eptr is None:
        edges = np.minimum(np.arange(nb + 1) * R, n)
        eptr = np.asarray(crow)[edges]
    ne = np.diff(eptr)
    nu = np.diff(uptr[::gpb])
    span = np.diff(uptr)
    pairs = vpair if vpair is not None else np.arange(nb * gpb)
    live = (pairs >= 0) & (pairs < (n + 1) // 2)
    assert (span[~live] == 0).all()
    # which rows of a pair have records at all: (first, second) per slot
    slot_of = np.repeat(np.arange(nb * gpb), span)
    if upos is not None:
        has = [np.bincount(slot_of, weights=((upos >> (16 * r)) & 0x8000) == 0, minlength=nb * gpb) > 0 for r in (0, 1)]
    else:
        has = [np.bincount(slot_of, weights=(ucol >> (30 + r)) & 1, minlength=nb * gpb) > 0 for r in (0, 1)]
    states = set(zip(has[0][live].tolist(), has[1][live].tolist()))
    return dict(ne=ne, nu=nu, span=span[live], pairs=pairs[live], states=states, ecap=plan.ecap, ucap=plan.ucap, nblocks=nb,
                value_chunks=int(-(-int(ne.max()) // BLOCK)), union_chunks=int(-(-int(nu.max()) // BLOCK)))


def residues(facts, geo, mode):
    """Residues mod U·EP of the per-slot union lengths, and whether a non-empty slot is shorter than one unrolled step."""
    step = unroll_of(geo, mode) * geo.ep
    span = facts["span"]
    return set((span % step).tolist()), bool(((span > 0) & (span < step)).any())


def walk_rowpack(plan, crow, n, val, S, mode, own=None, alpha=1.0):
    """The row-pair kernel in float64 on the stream arrays.  SPMM: out (n × p).  BWD: (gradA in the value array's order, out).
    SDDMM: the dots in stored order.  `val`: the value array the plan addresses (through sperm when it has one)."""
    uptr, ucol, upos, sperm, vpair, eptr = stream_arrays(plan)
    crow = np.asarray(crow, dtype=np.int64)
    gpb, nb, R = plan.gpb, plan.nblocks, plan.rpb
    slots, permuted = upos is not None, sperm is not None
    assert mode == SPMM or (mode == BWD and permuted) or (mode == SDDMM and not slots)
    order = np.arange(nb) if plan.order is None else plan.order.cpu().numpy().astype(np.int64)
    assert sorted(order.tolist()) == list(range(nb))
    ngroups = (n + 1) // 2
    out = np.zeros((n, S.shape[1]))
    nnz = int(crow[-1])
    grad = np.zeros(nnz)
    written = np.zeros(nnz, dtype=np.int64)
    colmask = 0xFFFFFFFF if slots else 0x3FFFFFFF
    for b in order:
        if eptr is not None:
            e0, e1 = int(eptr[b]), int(eptr[b + 1])
        else:
            r0 = min(b * R, n)
            e0, e1 = int(crow[r0]), int(crow[min(r0 + R, n)])
        assert e1 - e0 <= plan.ecap and uptr[(b + 1) * gpb] - uptr[b * gpb] <= plan.ucap
        pos = sperm[e0:e1] if permuted else np.arange(e0, e1)
        staged = val[pos] if mode != SDDMM else None
        dots = np.zeros(e1 - e0)
        used = np.zeros(e1 - e0, dtype=np.int64)
        for s in range(gpb):
            slot = b * gpb + s
            pair = int(vpair[slot]) if vpair is not None else slot
            if pair < 0 or pair >= ngroups:
                continue
            w = ucol[uptr[slot]:uptr[slot + 1]]
            c = w & colmask
            for r in (0, 1):
                row = 2 * pair + r
                if slots:
                    half = (upos[uptr[slot]:uptr[slot + 1]] >> (16 * r)) & 0xFFFF
                    mine = (half & 0x8000) == 0
                    idx = half[mine]
                else:
                    mine = ((w >> (30 + r)) & 1) == 1
                    idx = (int(crow[row]) - e0 if row < n else 0) + np.arange(int(mine.sum()))
                if not mine.any():
                    continue
                assert row < n and (idx < e1 - e0).all(), "a record of a row that does not exist, or a slot beyond the staged values"
                used[idx] += 1
                if mode != SDDMM:
                    out[row] = (staged[idx, None] * S[c[mine]]).sum(0)
                if mode != SPMM:
                    dots[idx] = (own[row][None, :] * S[c[mine]]).sum(1)
        assert (used == 1).all(), "a staged value is used by no record, or by several"
        if mode == BWD:
            grad[pos] = dots
            written[pos] += 1
        elif mode == SDDMM:
            grad[e0:e1] = alpha * dots
            written[e0:e1] += 1
    if mode == SPMM:
        return out
    assert (written == 1).all()
    return (grad, out) if mode == BWD else grad


# ---- B. tile cases ------------------------------------------------------------------------------------------------------------------

TileCase = collections.namedtuple("TileCase", "name crow col n m lens perm")

_CYCLE = (0, 1, 7, 8, 9, 15, 16, 17)


def _blocks(name, rng, blocks):
    """A pattern of 64-row blocks, block b drawing from its own pool of consecutive columns.  blocks: (lens of the block's rows,
    pool size, cover[, shift]) — cover: row i takes the cyclic window from i·len on, so that the block's distinct columns are the whole
    pool; shift: the pool starts that many columns behind a multiple of 64, so that it lies across two blocks of the transposed pattern
    and a row's values are two short runs there (rows whose columns fall into one block of the transpose form ONE run together)."""
    lens, start, size, cyc = [], [], [], []
    c0 = 0
    for ln, pool, cover, *shift in blocks:
        ln = np.asarray(ln, dtype=np.int64)
        lens.append(ln)
        c0 += shift[0] if shift else 0
        start.append(np.full(len(ln), c0))
        size.append(np.full(len(ln), pool))
        cyc.append(np.cumsum(ln) - ln if cover else np.full(len(ln), -1))
        c0 = -(-(c0 + pool) // 64) * 64      # (pools start on multiples of 64, so that a block of the TRANSPOSED pattern meets one block's rows)
    lens, start, size, cyc = (np.concatenate(a) for a in (lens, start, size, cyc))
    crow, col = draw(rng, lens, start, size, np.where(cyc >= 0, cyc % np.maximum(size, 1), -1))
    return TileCase(name, crow, col, len(lens), c0 + 3, lens, None)


def _full(rows=64):
    return (np.full(rows, 28), 224, True)


def _empty():
    return (np.zeros(64, dtype=np.int64), 1, False)


def _one_long():
    ln = np.zeros(64, dtype=np.int64)
    ln[5] = 224
    return (ln, 224, True)


def _cycle():
    return (np.tile(_CYCLE, 8), 24, True)


TILE_NAMES = ["composite", "empty-first", "empty-last", "small", "chunks", "p1024"]


def tile_case(name):
    rng = np.random.default_rng(2000 + TILE_NAMES.index(name))
    if name == "composite":
        ragged = rng.integers(0, 11, 37)
        ragged[-1] = 5                      # A's last values: a run of five, whose second chunk would reach beyond the value array
        ones = rng.integers(0, 2, 64)
        ones[0] = 1
        return _blocks(name, rng, [_full(), _empty(), _one_long(), _cycle(), (np.full(64, 9), 16, True), (np.full(64, 8), 9, True),
                                   (ones, 1, False), (np.full(64, 3), 7, True), (np.full(64, 4), 8, True), (ragged, 10, False, 59)])
    if name == "empty-first":
        return _blocks(name, rng, [_empty(), _cycle(), (np.full(64, 9), 16, True)])
    if name == "empty-last":
        return _blocks(name, rng, [_cycle(), (np.full(64, 9), 16, True), _empty()])
    if name == "small":
        return _blocks(name, rng, [(rng.integers(0, 13, 37), 20, False)])
    if name == "p1024":
        return _blocks(name, rng, [(np.tile(_CYCLE, 8), 24, True), (rng.integers(0, 13, 21), 20, False)])
    assert name == "chunks"
    return chunk_case((1024, 513, 511, 512, 512))


def chunk_case(entries):
    """Five blocks of the given entry counts whose values lie ISOLATED in the value array (an arbitrary value permutation, as a
    pattern handed over in another storage order has): every value is a run of one and a chunk of its own, so a block of E entries
    has E chunks, and each chunk's other three values belong to other blocks.  Blocks 1 and 2 alternate with block 0, block 3 with 4."""
    rng = np.random.default_rng(2100 + entries[0])
    case = _blocks("chunks", rng, [(_spread(e, 64), 24, True) for e in entries])
    e = np.concatenate([[0], np.cumsum(entries)])
    assert entries[0] - entries[1] - entries[2] in (0, 1) and entries[3] - entries[4] in (0, 1)

    def alternate(first, second):
        seq = np.empty(len(first) + len(second), dtype=np.int64)
        seq[0::2], seq[1::2] = first, second
        return seq

    blocks = [np.full(k, b) for b, k in enumerate(entries)]
    owner = np.concatenate([alternate(blocks[0], np.concatenate(blocks[1:3])), alternate(blocks[3], blocks[4])])   # block of every value position
    assert (owner[1:] != owner[:-1]).all()
    perm = np.empty(e[-1], dtype=np.int64)
    for b in range(5):
        perm[e[b]:e[b + 1]] = np.flatnonzero(owner == b)
    return case._replace(perm=perm)


def pipeline_case(S, p_seed=0):
    """3·S + 3 blocks of short ragged rows (4 … 12 entries from a pool of 32 columns per block), every fifth block empty: with S
    persistent workgroups (2 per compute unit) every workgroup walks 4 or 3 blocks, staging block k + 1 while it walks block k."""
    rng = np.random.default_rng(2200 + p_seed)
    nb = 3 * S + 3
    lens = rng.integers(4, 13, (nb, 64))
    lens[4::5] = 0
    lens = lens.reshape(-1)
    blk = np.arange(nb * 64) // 64
    crow, col = draw(rng, lens, 32 * blk, np.full(nb * 64, 32))
    return TileCase("pipeline", crow, col, nb * 64, 32 * nb + 3, lens, None)


def tile_plans(case):
    """(forward plan, transposed plan or None, (tptr, tidx, tperm) of the transposed walk) on the CPU.  A case with `perm` walks its own
    pattern through that value permutation instead of a transpose."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    fwd = _tile.build_tile_plan(t(case.crow), t(case.col), case.n, case.m, *TILE_GEO)
    if case.perm is not None:
        walk = (case.crow, case.col, case.perm)
        back = _tile.build_tile_plan(t(case.crow), t(case.col), case.n, case.m, *TILE_GEO, perm=t(case.perm))
    else:
        walk = cr.transpose(case.crow, case.col, case.m)
        back = _tile.build_tile_plan(t(walk[0]), t(walk[1]), case.m, case.n, *TILE_GEO, perm=t(walk[2]))
    return fwd, back, walk


def tile_facts(plan):
    """Per block, from the plan's descriptors and lists: distinct columns (U), the padded list (Upad), entries (E), value chunks (NC)
    and entry records (X)."""
    nb = plan.n_blocks
    d = plan.desc[:nb].numpy().astype(np.int64)
    ucol = plan.ucol.numpy()
    distinct = np.array([len(np.unique(ucol[d[b, 0]:d[b, 0] + d[b, 1]])) for b in range(nb)])
    return dict(U=distinct, Upad=d[:, 1], E=d[:, 3], NC=d[:, 5], X=d[:, 7])


def value_runs(crow, perm, rows_per_block=64):
    """Lengths of the runs of consecutive value positions the blocks of a permuted walk draw (one run per source row and block)."""
    n = len(crow) - 1
    blk = np.repeat(np.arange(n), np.diff(crow)) // rows_per_block
    o = np.lexsort((perm, blk))
    src, sb = perm[o], blk[o]
    new = np.ones(len(src), dtype=bool)
    new[1:] = (src[1:] != src[:-1] + 1) | (sb[1:] != sb[:-1])
    return np.diff(np.concatenate([np.flatnonzero(new), [len(src)]]))
