"""The cases of tests/test_gpu_plan_kernels.py, checked where they are built: on the host.  Both plan builders are index arithmetic on
CPU tensors, so what a case claims to reach — a second chunk of staged values, the capacity of 2048, a pinned residue of the unrolled
walk, a block of 224 distinct columns, 1024 value chunks, a persistent workgroup that walks four blocks — is asserted here from the
plan's own arrays, and the row-pair walk restated on those arrays (`_plan_cases.walk_rowpack`) must equal the plain sums exactly.
A pattern the builder refuses fails its test; the refusals that are meant (one row, 1025 chunks) are asserted as refusals."""

import numpy as np
import pytest
import torch

import _csr_ref as cr
import _plan_cases as pc
from torchsparsegradutils_amd import _pattern, _tile

_BUILT = {}


def _built(geo, name):
    key = (pc.rpb_of(geo), geo.ep == 1, name)
    if key not in _BUILT:
        case = pc.rowpack_case(name, pc.rpb_of(geo))
        _BUILT[key] = (case, pc.rowpack_plans(case, geo))
    return _BUILT[key]


def test_the_geometry_table():
    """16-byte column lanes, pairs of at least 8 lanes, 256 threads: 64 rows per workgroup, 32 with 16 column lanes."""
    for g in pc.GEOS:
        wide = 4 if g.dtype == torch.float32 else 8
        assert g.cl * wide == g.p and g.ep == max(1, 8 // g.cl) and pc.rpb_of(g) == (32 if g.cl == 16 else 64)
    assert sorted({(g.cl, g.ep) for g in pc.GEOS}) == [(2, 4), (4, 2), (8, 1), (16, 1)]
    assert [pc.unroll_of(g, pc.BWD) for g in pc.GEOS] == [4] * 4 + [3] * 4 and {pc.unroll_of(g, pc.SPMM) for g in pc.GEOS} == {4}
    # (what a plan depends on: test_walk_rowpack_equals_the_restatement runs geometries 0, 2 and 3)
    assert {(pc.rpb_of(g), g.ep == 1) for g in pc.GEOS} == {(pc.rpb_of(pc.GEOS[k]), pc.GEOS[k].ep == 1) for k in (0, 2, 3)}


@pytest.mark.parametrize("name", pc.ROWPACK_NAMES)
@pytest.mark.parametrize("geo", pc.GEOS, ids=pc.GEO_IDS)
def test_rowpack_case_claims(geo, name):
    case, plans = _built(geo, name)
    R, n = pc.rpb_of(geo), case.n
    lost = f"{name}: the case has lost its point: "
    rows = np.repeat(np.arange(n), np.diff(case.crow))
    assert (np.diff(case.col)[rows[1:] == rows[:-1]] > 0).all() and case.col.min() >= 0 and case.col.max() < case.m
    assert case.m != n or case.brick is not None, "rectangular"
    facts = {key: pc.rowpack_facts(plan, case.crow, n) for key, plan in plans.items()}
    for key, plan in plans.items():
        f = facts[key]
        assert plan.rpb == R and plan.gpb == R // 2 and f["ne"].sum() == len(case.col) == plan.nnz
        assert f["ecap"] == max(-(-int(f["ne"].max()) // 256) * 256, 256) <= pc.LIMITS[0]
        assert f["ucap"] == max(-(-int(f["nu"].max()) // 256) * 256, 256) <= pc.LIMITS[1]
        assert (plan.upos is not None) == (key[0] != "bits") and (plan.sperm is not None) == (key[0] in ("perm", "brick"))
        if key[1] == "dictionary":     # the two forms are one walk
            for a, b in zip(pc.stream_arrays(plan), pc.stream_arrays(plans[key[0], "stream"])):
                assert b is None or np.array_equal(a, b)
        if key[0] != "brick":
            assert plan.vpair is None and plan.eptr is None and f["nblocks"] == -(-n // R)
        if key == ("perm", "dictionary"):
            assert (plan.srcstart is None) == (name == "hub"), lost + "srcstart"
    f = facts["slots", "stream"]
    if name.startswith("rows-"):
        want = {"2": 2, "3": 3, "R-1": R - 1, "R+1": R + 1, "3R+1": 3 * R + 1}[name[5:]]
        assert n == want and f["nblocks"] == -(-n // R), lost + str(n)
        if n % 2:       # a lone last row: its pair has records of the first row only
            assert f["pairs"].max() == n // 2 and (True, False) in f["states"] and case.lens[-1] > 0, lost + "lone last row"
    elif name == "single-column":
        _, _, a, _ = pc.gathers(case)
        assert a.n_rows == 1 and a.nnz == 36 and _pattern.build_rowpack_plan(a, R, pc.LIMITS) is None, "one row shares nothing: refused"
        assert plans["perm", "stream"].reuse > 1.8
    elif name == "holes":
        assert f["states"] == {(False, False), (True, False), (False, True), (True, True)}, lost + str(f["states"])
        assert f["nblocks"] == 3 and f["ne"][1] == 0 and f["nu"][1] == 0 and f["ne"][0] > 0 and f["ne"][2] > 0, lost + str(f["ne"])
    elif name.startswith("ne-"):
        want = int(name[3:])
        assert f["ne"].max() == want and f["value_chunks"] == -(-want // 256) and f["ecap"] == -(-want // 256) * 256, lost + str(f["ne"])
    elif name == "cap-2048":
        for key in plans:
            assert facts[key]["ne"].max() == 2048 == facts[key]["ecap"] and facts[key]["value_chunks"] == 8, lost + str(key)
    elif name.startswith("nu-"):
        want = int(name[3:])
        assert f["nu"].max() == want and f["union_chunks"] == -(-want // 256), lost + str(f["nu"])
    elif name == "ucap-max":
        # a workgroup's union records are at most its stored entries, and those at most 2048: 8 chunks of 256 — the kernel's other
        # four (kRpMaxU = 12) are out of any plan's reach.  Here ucap = ecap = 2048: with slot words s_upos lies at +ucap, s_val at +2·ucap
        for key in plans:
            g = facts[key]
            assert g["ecap"] == 2048 == g["ucap"] and g["union_chunks"] == 8 == g["value_chunks"], lost + str(key)
            assert g["ne"].max() == 2048 == g["nu"].max() and 1.2 <= plans[key].reuse < 1.5, lost + str(key)
            assert plans[key].ucap * (8 if plans[key].upos is not None else 4) + plans[key].ecap * 4 <= pc.LIMITS[2]
    elif name == "residues":
        for key, plan in plans.items():
            for mode in pc.MODES_OF_WALK[key[0]]:
                step = pc.unroll_of(geo, mode) * geo.ep      # (ownership-bit walks have one entry lane)
                got, short = pc.residues(facts[key], geo, mode)
                assert got == set(range(step)) and short, lost + f"{key} mode {mode}: residues {sorted(got)} of {step}"
    elif name == "hub":
        assert np.bincount(case.col).max() == n >= 257, lost + "a source row of 257 entries"
    else:
        for form in pc.FORMS:
            plan = plans["brick", form]
            assert plan.vpair is not None and (form == "dictionary" or plan.eptr is not None)
            assert bool((plan.vpair < 0).any()) and plan.lattice is not None and len(plan.lattice) == (2 if name == "brick-3d" else 1)
            assert plan.nblocks > plans["perm", form].nblocks


@pytest.mark.parametrize("geo", pc.GEOS, ids=pc.GEO_IDS)
def test_the_cases_launch_every_instantiation_and_plan_form(geo):
    seen = set()
    for name in pc.ROWPACK_NAMES:
        seen |= set(pc.launches(_built(geo, name)[1]))
    assert seen == pc.instantiations(geo)
    assert (pc.SPMM, "bits", "stream") in seen if geo.cl >= 8 else all(walk != "bits" for _, walk, _ in seen)


@pytest.mark.parametrize("name", pc.ROWPACK_NAMES)
@pytest.mark.parametrize("geo", [pc.GEOS[0], pc.GEOS[2], pc.GEOS[3]], ids=[pc.GEO_IDS[k] for k in (0, 2, 3)])
def test_walk_rowpack_equals_the_restatement(geo, name):
    """Integer data: every sum is exact, so the walk over the plan's records — in every plan form, and with the workgroups in another
    order — must EQUAL the sums over the CSR arrays.  A plan depends on the rows per workgroup and on whether the geometry has one entry
    lane (ownership bits): the three geometries here have every plan the eight build."""
    case, plans = _built(geo, name)
    rng = np.random.default_rng(3)
    nnz, n, m, p = len(case.col), case.n, case.m, 3
    _, _, _, perm = pc.gathers(case)
    val, S, own = (rng.integers(-3, 4, s).astype(np.float64) for s in (nnz, (m, p), (n, p)))
    grad = np.empty(nnz)
    grad[perm] = cr.sddmm(case.crow, case.col, own, S, 1.0)
    for (mode, walk, form) in pc.launches(plans):
        plan = plans[walk, form]
        if form == "stream" and plan.nblocks > 1:
            plan = pc.plan_to(plan, "cpu")
            plan.order = torch.from_numpy(rng.permutation(plan.nblocks)).to(torch.int32)
        got = pc.walk_rowpack(plan, case.crow, n, val, S, mode, own=own, alpha=-2.0)
        if mode == pc.SPMM:
            assert np.array_equal(got, cr.spmm(case.crow, case.col, val, S, perm if walk in ("perm", "brick") else None)), (walk, form)
        elif mode == pc.BWD:
            assert np.array_equal(got[0], grad) and np.array_equal(got[1], cr.spmm(case.crow, case.col, val, S, perm)), (walk, form)
        else:
            assert np.array_equal(got, cr.sddmm(case.crow, case.col, own, S, -2.0)), (walk, form)


# ---- tiles --------------------------------------------------------------------------------------------------------------------------

def _check_tile_plan(case, plan, crow, col, perm):
    """Every stored entry is recoverable from the plan: its column through lidx / the entry records, its value through the chunks."""
    nb, R = plan.n_blocks, 64
    n = len(crow) - 1
    d = plan.desc.numpy().astype(np.int64)
    assert nb == -(-n // R) and not d[nb:].any() and plan.desc.shape == (nb + 4, 8)
    rows = np.repeat(np.arange(n), np.diff(crow))
    blk = rows // R
    ucol, lidx = plan.ucol.numpy().astype(np.int64), plan.lidx.numpy().astype(np.int64)
    assert np.array_equal(ucol[d[blk, 0] + lidx[:len(col)]], col)
    assert np.array_equal(d[:nb, 3], np.bincount(blk, minlength=nb)) and (d[:nb, 1] % 8 == 0).all()
    ent = plan.ent.numpy().astype(np.int64) & 0xFFFF
    xrow = plan.xrow.numpy().astype(np.int64)
    q = np.arange(len(col)) - crow[rows]
    assert np.array_equal(ent[d[blk, 6] + xrow[rows] + q // 8, q % 8], lidx[:len(col)] * _tile.TILE_ROW_BYTES)
    assert (ent == pc.TILE_GEO[1] * _tile.TILE_ROW_BYTES).sum() == ent.size - len(col), "every other record slot names the zero row"
    if perm is not None:
        cpos, cslot = plan.cpos.numpy().astype(np.int64), plan.cslot.numpy().astype(np.int64) & 0xFFFF
        cblk = np.repeat(np.arange(nb), d[:nb, 5])
        assert len(cpos) == d[:nb, 5].sum() and cpos.min() >= 0 and cpos.max() <= len(col) - 4
        c, j = np.nonzero(cslot != 0xFFFF)
        entry = d[cblk[c], 2] + cslot[c, j]          # the walked entry every fetched value belongs to
        assert sorted(entry.tolist()) == list(range(len(col))) and np.array_equal(cpos[c] + j, perm[entry])


def test_tile_case_claims():
    assert pc.TILE_CHUNKS == _tile.MAX_CHUNKS
    for name in pc.TILE_NAMES:
        case = pc.tile_case(name)
        fwd, back, walk = pc.tile_plans(case)
        assert fwd is not None and back is not None, f"{name}: the builder refused the pattern"
        assert fwd.cpos is None and back.cpos is not None and fwd.reuse >= 2.0 and back.reuse >= 2.0
        _check_tile_plan(case, fwd, case.crow, case.col, None)
        _check_tile_plan(case, back, *walk)
        f, b = pc.tile_facts(fwd), pc.tile_facts(back)
        lens = np.pad(case.lens, (0, -case.n % 64)).reshape(-1, 64)
        if name == "composite":
            assert case.n % 64 == 37 and case.m != case.n
            assert (f["U"][0], f["E"][0]) == (224, 1792) and (f["U"][1], f["E"][1], f["X"][1]) == (0, 0, 0)
            assert (f["U"][2], f["E"][2], f["X"][2]) == (224, 224, 28) and (lens[2] > 0).sum() == 1
            assert sorted(set(lens[3].tolist())) == list(pc._CYCLE) and f["U"][3] == 24
            assert set(lens[4].tolist()) == {9} and set(lens[5].tolist()) == {8}, "uniform rows: the wave's min is its max"
            assert f["U"][5:9].tolist() == [9, 1, 7, 8] and f["Upad"][5:9].tolist() == [16, 8, 8, 8], "lists padded to eight with repeats"
            runs = pc.value_runs(walk[0], walk[2])
            assert set(range(1, 6)) <= set(runs.tolist()), sorted(set(runs.tolist()))
            cpos, cslot = back.cpos.numpy(), back.cslot.numpy().astype(np.int64) & 0xFFFF
            clamped = (cpos == len(case.col) - 4) & (cslot[:, 0] == 0xFFFF)
            assert clamped.any(), "a chunk clamped at nnz - 4"
            assert ((cslot == 0xFFFF).any(1) & (cslot != 0xFFFF).any(1)).any()
            assert b["E"].max() <= 1792 and b["U"].max() <= 224 and len(b["E"]) >= 8
        elif name == "empty-first":
            assert f["E"][0] == 0 and f["E"][1:].min() > 0
        elif name == "empty-last":
            assert f["E"][-1] == 0 and f["E"][:-1].min() > 0 and case.n % 64 == 0
        elif name == "small":
            assert case.n == 37 and fwd.n_blocks == 1
        elif name == "chunks":
            assert b["NC"].tolist() == [1024, 513, 511, 512, 512] == b["E"].tolist()
            cslot = back.cslot.numpy().astype(np.int64) & 0xFFFF
            assert ((cslot != 0xFFFF).sum(1) == 1).all(), "every chunk holds one value of its block and three of others"
            assert (back.cpos.numpy() == len(case.col) - 4).sum() >= 2, "the last values: chunks clamped at nnz - 4"
    # 1025 isolated values in one block: one chunk more than the kernel's threads can fetch
    over = pc.chunk_case((1025, 513, 512, 512, 512))
    fwd, back, _ = pc.tile_plans(over)
    assert fwd is not None and back is None
    # limits: one distinct column, one entry too many
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    c = pc.tile_case("composite")
    assert _tile.build_tile_plan(t(c.crow), t(c.col), c.n, c.m, 64, 223, 1792) is None
    assert _tile.build_tile_plan(t(c.crow), t(c.col), c.n, c.m, 64, 224, 1791) is None


def test_the_pipeline_case_for_a_stand_in_device():
    """S persistent workgroups (the launcher: 2 per compute unit) and 3·S + 3 blocks: ⌈blocks / S⌉ = 4 blocks per workgroup, a grid of
    ⌈blocks / 4⌉, in which (cyclic schedule: workgroup w walks blocks w, w + grid, ...) every workgroup walks 4 or 3 blocks, and in
    runs of consecutive blocks the last one walks 3."""
    S = 8
    case = pc.pipeline_case(S)
    fwd, back, walk = pc.tile_plans(case)
    assert fwd is not None and back is not None
    nb = fwd.n_blocks
    per = -(-nb // S)
    grid = -(-nb // per)
    assert nb == 3 * S + 3 and per == 4 and grid == -(-nb // 4)
    walked = [len(range(w, nb, grid)) for w in range(grid)]
    assert set(walked) == {3, 4} and nb - (grid - 1) * per == 3
    f = pc.tile_facts(fwd)
    assert (f["E"][4::5] == 0).all() and (np.delete(f["E"], np.s_[4::5]) > 256).all() and f["E"].max() <= 1792
    assert 7.5 < case.lens[case.lens > 0].mean() < 8.5 and case.lens.max() == 12
    _check_tile_plan(case, fwd, case.crow, case.col, None)
    _check_tile_plan(case, back, *walk)
