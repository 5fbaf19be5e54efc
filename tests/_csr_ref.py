"""A plain float64 restatement of the plan-free CSR kernels (csrc/spmm_impl.h, sddmm_impl.h, bwd_impl.h) and the patterns their
tests run on.  numpy only: nothing here imports the package, the library or oracle/.

References: one product per stored entry, summed per row with `reduceat` — `spmm`, `sddmm`, `coo_sddmm`, `backward`, `dot_partial`
— and for each the same sum over the absolute terms (`*_abs`), which the rounding bounds are multiples of.

Patterns: every builder takes `query(n_rows, nnz, max_row_nnz) -> Geom`, the library's own answer (`tsgu_csr_geometry`) for the
case's kernel, value type and width, and sizes itself from it: RPB = 256 / (column_lanes · entry_lanes) rows per run, W = RPB · row_runs
rows per workgroup, S = stage_entries.  The answer depends on the pattern (row_runs on the mean row length, the one-lane-per-row
geometry on the longest row), so a builder asks again with what it built until the two agree.  A builder returns a `Pattern` whose
`claim` is computed from `crow` and the final answer, never from the intention; the tests assert it (`check_claim`).
Columns are distinct and ascending inside a row; the matrix is rectangular, m = max(n, longest row) + 7.
"""

import collections

import numpy as np

BLOCK = 256

Geom = collections.namedtuple("Geom", "vec cl ep tiles runs stage")
Pattern = collections.namedtuple("Pattern", "name crow col n m lens geom claim honest")


def rpb(g):
    return BLOCK // (g.cl * g.ep)


# ---- references ---------------------------------------------------------------------------------------------------------------------

def _rows_of(crow):
    return np.repeat(np.arange(len(crow) - 1), np.diff(crow))


def _row_sums(terms, crow):
    """out[i] = Σ terms[crow[i]:crow[i+1]] (zeros for empty rows): reduceat over the starts of the rows that have entries."""
    n = len(crow) - 1
    out = np.zeros((n,) + terms.shape[1:])
    full = np.flatnonzero(np.diff(crow) > 0)
    if len(full):
        out[full] = np.add.reduceat(terms, crow[:-1][full], axis=0)
    return out


def spmm(crow, col, val, B, perm=None):
    v = val if perm is None else val[perm]
    return _row_sums(v[:, None] * B[col], crow)


def spmm_abs(crow, col, val, B, perm=None):
    return spmm(crow, col, np.abs(val), np.abs(B), perm)


def coo_sddmm(row, col, R, Cm, alpha):
    return alpha * np.einsum("kp,kp->k", R[row], Cm[col])


def coo_sddmm_abs(row, col, R, Cm, alpha):
    return coo_sddmm(row, col, np.abs(R), np.abs(Cm), abs(alpha))


def sddmm(crow, col, R, Cm, alpha):
    return coo_sddmm(_rows_of(crow), col, R, Cm, alpha)


def sddmm_abs(crow, col, R, Cm, alpha):
    return coo_sddmm_abs(_rows_of(crow), col, R, Cm, alpha)


def transpose(crow, col, m):
    """(tptr, tidx, tperm) of the transposed pattern: entries of column j in A's order (a stable sort by column)."""
    tperm = np.argsort(col, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=m))]).astype(np.int64)
    return tptr, _rows_of(crow)[tperm], tperm


def backward(crow, col, val, G, B):
    """(gradA, gradB) of C = A·B for the upstream gradient G: gradA[k] = <G[row k], B[col k]>, gradB = Aᵀ·G."""
    tptr, tidx, tperm = transpose(crow, col, B.shape[0])
    return sddmm(crow, col, G, B, 1.0), spmm(tptr, tidx, val, G, tperm)


def backward_abs(crow, col, val, G, B):
    return backward(crow, col, np.abs(val), np.abs(G), np.abs(B))


def dot_partial(C, W, rows_per_workgroup):
    """partial[vb, c] = Σ_{rows of workgroup vb} C[row, c] · W[row, c]."""
    n = C.shape[0]
    starts = np.arange(0, n, rows_per_workgroup)
    return np.add.reduceat(C * W, starts, axis=0) if n else np.zeros((0, C.shape[1]))


def dot_partial_abs(C, W, rows_per_workgroup):
    return dot_partial(np.abs(C), np.abs(W), rows_per_workgroup)


# ---- patterns -----------------------------------------------------------------------------------------------------------------------

def columns(rng, lens, m):
    """(crow, col): rows of `lens` entries, columns distinct and ascending inside a row, below m."""
    lens = np.asarray(lens, dtype=np.int64)
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(crow[-1])
    if nnz == 0:
        return crow, np.zeros(0, dtype=np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)
    first = crow[:-1][rows]
    gap_max = np.minimum(np.maximum((m - 1) // lens[rows], 1), 9)
    gaps = rng.integers(1, gap_max + 1)
    gaps[first == np.arange(nnz)] = 0
    off = np.cumsum(gaps)
    off -= off[first]
    span = np.zeros(len(lens), dtype=np.int64)
    full = lens > 0
    span[full] = off[crow[1:][full] - 1]
    assert span.max() < m
    start = rng.integers(0, m - span)
    col = start[rows] + off
    assert col.min() >= 0 and col.max() < m
    return crow, col


def _finish(name, rng, lens, g, claim, honest=True):
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    m = max(n, int(lens.max()) if n else 0) + 7
    crow, col = columns(rng, lens, m)
    return Pattern(name, crow, col, n, m, lens, g, claim, honest)


def _settle(query, lens_for, honest=True):
    """lens_for(Geom) -> row lengths; asked again with what was built until the geometry is the one it was built for."""
    g = query(1024, 2048, 0)
    for _ in range(6):
        lens = np.asarray(lens_for(g), dtype=np.int64)
        got = query(len(lens), int(lens.sum()), int(lens.max()) if honest and len(lens) else 0)
        if got == g:
            return lens, g
        g = got
    raise AssertionError("the geometry did not settle")


def slices(crow, g):
    """Stored entries of every workgroup's slice."""
    n = len(crow) - 1
    w = rpb(g) * g.runs
    edges = np.minimum(np.arange(0, n + w, w), n)
    return np.diff(crow[edges])


def ragged(query, rng):
    lens, g = _settle(query, lambda g: rng.integers(0, 6, 2 * 8 * rpb(g) + 3))
    n, w = len(lens), rpb(g) * g.runs
    claim = dict(partial_last_workgroup=n % w != 0, partial_last_run=n % rpb(g) != 0, blocks=-(-n // w),
                 has_empty_rows=bool((lens == 0).any()), max_len=int(lens.max()))
    return _finish("ragged", rng, lens, g, claim)


UNIFORM_KINDS = ("runs1", "runsmid", "runs8", "fits", "stream")


def uniform(query, rng, kind):
    """n = 2·RPB + 3 rows of L entries, L from spmm_row_mult's rule (row_runs = ⌊1536 / (L·RPB)⌋ clipped to 1 … 8): 1024 / RPB gives 1,
    ⌈384 / RPB⌉ a value between, 1 gives 8 — with RPB = 256 only a mean below 1 does, so every other row is empty there — then
    S / RPB (the slice of a full workgroup is exactly S) and S / RPB + 1 (it streams)."""
    def lens_for(g):
        r, n = rpb(g), 2 * rpb(g) + 3
        length = {"runs1": 1024 // r, "runsmid": -(-384 // r), "runs8": 1, "fits": g.stage // r, "stream": g.stage // r + 1}[kind]
        lens = np.full(n, length)
        if kind == "runs8" and r > 192:
            lens[1::2] = 0
        return lens

    lens, g = _settle(query, lens_for)
    crow = np.concatenate([[0], np.cumsum(lens)])
    sl = slices(crow, g)
    r = rpb(g)
    straddles = True
    if kind == "stream":     # every full run has a row that lies across a pass boundary (passes start at the run's first entry)
        for s0 in range(0, len(lens) - r + 1, r):
            cut = crow[s0] + g.stage
            straddles &= bool(((crow[s0:s0 + r] < cut) & (crow[s0 + 1:s0 + r + 1] > cut)).any())
    claim = dict(runs=g.runs, first_slice=int(sl[0]), max_slice=int(sl.max()), straddles=straddles, one_lane_per_row=r == BLOCK,
                 blocks=len(sl))
    return _finish("uniform-" + kind, rng, lens, g, claim)


def long_among_short(query, rng, honest):
    def lens_for(g):
        lens = np.full(3 * 256 + 1, 2)
        lens[len(lens) // 2] = g.stage + 50
        return lens

    lens, g = _settle(query, lens_for, honest)
    crow = np.concatenate([[0], np.cumsum(lens)])
    claim = dict(runs=g.runs, max_slice=int(slices(crow, g).max()), one_lane_per_row=rpb(g) == BLOCK)
    return _finish("long-among-short" + ("" if honest else "-unknown-longest"), rng, lens, g, claim, honest)


def pass_edges(query, rng):
    """Rows of S − 1, S, S + 1 and 2S + 1 entries, each alone in its workgroup, at another place in it each time."""
    def lens_for(g):
        w = rpb(g) * g.runs
        lens = np.zeros(4 * w + 3, dtype=np.int64)
        for b, length in enumerate((g.stage - 1, g.stage, g.stage + 1, 2 * g.stage + 1)):
            lens[b * w + (5 * b + 1) % w] = length
        return lens

    lens, g = _settle(query, lens_for)
    crow = np.concatenate([[0], np.cumsum(lens)])
    sl = slices(crow, g)
    claim = dict(passes=[int(-(-s // g.stage)) for s in sl[:4]], slices=[int(s) for s in sl[:4]], rows_with_entries=int((lens > 0).sum()))
    return _finish("pass-edges", rng, lens, g, claim)


EMPTY_KINDS = ("all-empty", "outer-workgroups-empty", "one-entry", "short-block")


def empties(query, rng, kind):
    def lens_for(g):
        r, w = rpb(g), rpb(g) * g.runs
        if kind == "all-empty":
            return np.zeros(2 * r + 3, dtype=np.int64)
        if kind == "outer-workgroups-empty":
            lens = np.zeros(3 * w, dtype=np.int64)
            lens[w:2 * w] = 3
            return lens
        if kind == "one-entry":
            return np.ones(1, dtype=np.int64)
        return np.full(r - 1, 2)

    lens, g = _settle(query, lens_for)
    crow = np.concatenate([[0], np.cumsum(lens)])
    claim = dict(n=len(lens), nnz=int(lens.sum()), slices=[int(s) for s in slices(crow, g)], rows_per_run=rpb(g))
    return _finish("empties-" + kind, rng, lens, g, claim)


BUILDERS = (["ragged"] + ["uniform-" + k for k in UNIFORM_KINDS] + ["long-among-short", "long-among-short-unknown-longest", "pass-edges"]
            + ["empties-" + k for k in EMPTY_KINDS])


def build(name, query, rng):
    if name == "ragged":
        return ragged(query, rng)
    if name.startswith("uniform-"):
        return uniform(query, rng, name[len("uniform-"):])
    if name.startswith("long-among-short"):
        return long_among_short(query, rng, honest=name == "long-among-short")
    if name == "pass-edges":
        return pass_edges(query, rng)
    return empties(query, rng, name[len("empties-"):])


def check_claim(pat, spmm_rules=True):
    """Assert that the pattern is what its builder is for.  `spmm_rules`: the kernel has row runs and a fits / streaming split
    (CSR SpMM); the others stage their slice in passes of S whatever its size and always report one run."""
    g, c, lost = pat.geom, pat.claim, f"{pat.name}: the case has lost its point: "
    n, s = pat.n, g.stage
    assert pat.crow[0] == 0 and len(pat.crow) == n + 1 and pat.crow[-1] == len(pat.col) and pat.m == max(n, int(pat.lens.max())) + 7
    if len(pat.col):
        rows = _rows_of(pat.crow)
        same = rows[1:] == rows[:-1]
        assert (np.diff(pat.col)[same] > 0).all() and pat.col.min() >= 0 and pat.col.max() < pat.m, "columns ascend inside a row"
    if not spmm_rules:
        assert g.runs == 1
    if pat.name == "ragged":
        assert c["partial_last_workgroup"] and c["partial_last_run"] and c["has_empty_rows"] and c["max_len"] == 5, lost + str(c)
        assert c["blocks"] >= 2
    elif pat.name.startswith("uniform-"):
        kind = pat.name[len("uniform-"):]
        # two full runs of rows and a partial third: in several workgroups, or (row_runs > 2) as the runs of one
        assert n == 2 * rpb(g) + 3 and c["blocks"] == -(-3 // g.runs), lost + str(c)
        if kind == "fits":
            assert c["first_slice"] == s == c["max_slice"] and g.runs == 1, lost + str(c)
        elif kind == "stream":
            assert c["first_slice"] == s + rpb(g) and c["straddles"] and g.runs == 1, lost + str(c)
        elif spmm_rules:
            want = {"runs1": g.runs == 1, "runsmid": 1 < g.runs < 8, "runs8": g.runs == 8}[kind]
            assert want and c["max_slice"] <= s, lost + str(c)
    elif pat.name.startswith("long-among-short"):
        assert c["max_slice"] > s, lost + str(c)
        if spmm_rules:     # one lane per row keeps 256 rows per run, and with them one run
            assert (g.runs == 1) if c["one_lane_per_row"] else (g.runs > 1), lost + str(c)
    elif pat.name == "pass-edges":
        assert c["passes"] == [1, 1, 2, 3] and c["slices"] == [s - 1, s, s + 1, 2 * s + 1] and c["rows_with_entries"] == 4, lost + str(c)
    else:
        kind = pat.name[len("empties-"):]
        if kind == "all-empty":
            assert c["nnz"] == 0 and n > rpb(g), lost + str(c)
        elif kind == "outer-workgroups-empty":
            assert len(c["slices"]) == 3 and c["slices"][0] == 0 == c["slices"][2] and c["slices"][1] > 0, lost + str(c)
        elif kind == "one-entry":
            assert n == 1 and c["nnz"] == 1, lost + str(c)
        else:
            assert n == rpb(g) - 1 and c["nnz"] == 2 * n, lost + str(c)
