"""The plan-free CSR kernels — csr_spmm, csr_sddmm, coo_sddmm and the fused csr_mm_backward — called directly (`_backend`), in every
lane geometry, against the float64 restatement of tests/_csr_ref.py.  These kernels are what the plan families and the Krylov solvers
are compared with elsewhere in the suite; here they are compared with plain sums.

Cases (tests/_csr_cases.py): 21 widths per value type — `wide`·{1, 2, 3, 4, 8, 16, 32, 64, 65, 130} in 16-byte lanes, {1, 3, 5, 9, 17,
33, 65, 129} and 2 in scalar lanes, two multiples of `wide` whose operand forbids 16-byte lanes — paired with the 13 pattern builders
and both index types: 78 different pairs per kernel (the fused backward: the 17 widths of one column tile).  Every case asserts what `tsgu_csr_geometry` answers for it (vec, column lanes, entry lanes, column tiles)
against the table it was written for, and its pattern's claim (one pass or several, row runs, empty workgroups, ...).

Exact: integer operands in [−3, 3].  A term is at most 9 and a row has at most 2·2048 + 1 entries, a dot at most 1040 columns: every sum
stays below 2^24 and is exact in float32 and float64 accumulators, so the results must EQUAL the restatement — a bfloat16 result the
exact value rounded once; an SDDMM result the exact dot times alpha (alpha as the accumulator holds it), rounded once per format.

Random: operands uniform in (−1, 1), rounded to the value type first.  Bounds are counted, eps the accumulator's machine epsilon
(2^-23 for float32 and bfloat16 operands, 2^-52 for float64):
  a row sum of len fma terms, in any order and association   (len + 2) eps Σ|terms|
  an SDDMM dot over p columns, times alpha                   (p + 3) eps |alpha| Σ|r c|
  a bfloat16 result is rounded once more                     + 2^-8 (|exact| + bound)
  a dot partial over the W rows of a workgroup               (W + 2) eps Σ|C W|, against the float64 sum of the C the kernel stored
Every case prints max |err| / bound; the last test prints the largest per kernel and value type.
"""

import types

import numpy as np
import pytest
import torch

import _csr_cases as cc
import _csr_ref as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.bfloat16: 2.0 ** -23}
NAME = dict(zip(cc.DTYPES, cc.IDS))
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _be():
    from torchsparsegradutils_amd import _backend

    return _backend


# ---- operands ---------------------------------------------------------------------------------------------------------------------

def _values(rng, shape, dtype, ints):
    """(float64 numpy values representable in `dtype`, the CPU tensor of that type)."""
    x = rng.integers(-3, 4, shape).astype(np.float64) if ints else rng.uniform(-1.0, 1.0, shape)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    return t.double().numpy(), t


def _dense(rng, rows, p, dtype, ints, mode="ok", pad=0):
    """A rows × p operand on the device.  mode "ld": a column slice of a buffer one column wider; "ptr": a contiguous matrix one
    element off a 16-byte boundary; pad: a column slice of a buffer `pad` columns wider (lanes kept when pad is a multiple of `wide`)."""
    x, t = _values(rng, (rows, p), dtype, ints)
    if mode == "ld" or pad:
        buf = torch.zeros((rows, p + (pad or 1)), dtype=dtype, device=DEV)
        d = buf[:, :p]
    elif mode == "ptr":
        buf = torch.zeros(rows * p + 1, dtype=dtype, device=DEV)
        d = buf[1:].view(rows, p)
        assert d.data_ptr() % 16 != 0 or DEV == "cpu"
    else:
        d = torch.empty((rows, p), dtype=dtype, device=DEV)
        assert d.data_ptr() % 16 == 0 or DEV == "cpu"
    d.copy_(t)
    return x, d


def _index(a, itype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(itype).to(DEV)


def _stored(x, dtype):
    """Exact float64 values as a kernel stores them: rounded once to the value type."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).double().numpy()


def _host(t):
    return t.double().cpu().numpy()


def _hold(kernel, dtype, what, got, ref, abs_terms, count):
    """|got − ref| <= (count + 2) eps Σ|terms| elementwise (bfloat16: + 2^-8 (|ref| + that)); where the bound is zero, equality."""
    bound = (np.asarray(count, dtype=np.float64) + 2.0) * EPS[dtype] * abs_terms
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)
    err = np.abs(got - ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    zero = bound == 0
    assert (err[zero] == 0).all(), f"{what}: an element with no terms is not zero"
    ratio = float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0
    print(f"{cc.KERNELS[kernel]} {NAME[dtype]} {what}: max |err| / bound = {ratio:.4f}")
    key = (cc.KERNELS[kernel], NAME[dtype])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    worst = np.unravel_index(np.argmax(np.where(zero, 0.0, err / np.where(zero, 1.0, bound))), err.shape) if err.size else ()
    assert ratio <= 1.0, f"{what}: |err| / bound = {ratio} at {worst}: got {got[worst]}, float64 {ref[worst]}"


def _same(what, got, want):
    bad = np.flatnonzero((got != want).reshape(-1))
    assert got.shape == want.shape and not len(bad), \
        f"{what}: {len(bad)} of {got.size} elements differ, the first at {np.unravel_index(bad[0], got.shape)}: " \
        f"{got.reshape(-1)[bad[0]]} for {want.reshape(-1)[bad[0]]}"


def _longest(pat):
    return int(pat.lens.max()) if pat.honest and pat.n else 0


CASES = list(range(cc.N_CASES))


# ---- csr_spmm ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", CASES)
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm(dtype, i):
    p, mode, itype, pat = cc.pattern(cc.SPMM, dtype, i)
    rng = np.random.default_rng(i)
    crow, col = _index(pat.crow, itype), _index(pat.col, itype)
    what = f"case {i} p={p} {mode} {pat.name} {str(itype)[6:]} {tuple(pat.geom)}"
    for ints in (True, False):
        v, vt = _values(rng, len(pat.col), dtype, ints)
        b, B = _dense(rng, pat.m, p, dtype, ints, mode)
        C = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
        ref = cr.spmm(pat.crow, pat.col, v, b)
        if ints:
            _same(what + " exact", _host(C), _stored(ref, dtype))
        else:
            _hold(cc.SPMM, dtype, what, _host(C), ref, cr.spmm_abs(pat.crow, pat.col, v, b), pat.lens[:, None])
            again = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
            assert torch.equal(C, again), what + ": two runs differ"


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm_the_longest_row_decides_one_lane_per_row(dtype):
    """The two long-among-short cases at p = wide: the honest longest row keeps 8 entry lanes and 8 row runs (MULTI with a streaming
    slice), an unknown one gives every row one lane — the long row too."""
    w = cc.WIDE[dtype]
    for honest, ep, runs in ((True, 8, 8), (False, 1, 1)):
        name = "long-among-short" + ("" if honest else "-unknown-longest")
        pat = cr.build(name, cc.query(cc.SPMM, dtype, w), np.random.default_rng(5))
        cr.check_claim(pat)
        assert (pat.geom.vec, pat.geom.cl, pat.geom.ep, pat.geom.runs) == (w, 1, ep, runs) and pat.claim["max_slice"] > pat.geom.stage
        rng = np.random.default_rng(6)
        v, vt = _values(rng, len(pat.col), dtype, True)
        b, B = _dense(rng, pat.m, w, dtype, True)
        C = _be().csr_spmm(_index(pat.crow, torch.int32), _index(pat.col, torch.int32), vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
        _same(name, _host(C), _stored(cr.spmm(pat.crow, pat.col, v, b), dtype))


@pytest.mark.parametrize("kind", cr.UNIFORM_KINDS)
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm_one_lane_per_row(dtype, kind):
    """p = wide and short rows: 256 rows per run, each walked by one lane — 1, 3 and 8 runs, a slice of exactly S and one that streams."""
    w = cc.WIDE[dtype]
    pat = cr.build("uniform-" + kind, cc.query(cc.SPMM, dtype, w), np.random.default_rng(25))
    cr.check_claim(pat)
    g = pat.geom
    assert (g.vec, g.cl, g.ep, g.tiles) == (w, 1, 1, 1) and pat.claim["one_lane_per_row"] and pat.n == 515
    assert g.runs == {"runs1": 1, "runsmid": 3, "runs8": 8, "fits": 1, "stream": 1}[kind]
    rng = np.random.default_rng(26)
    crow, col = _index(pat.crow, torch.int64), _index(pat.col, torch.int64)
    for ints in (True, False):
        v, vt = _values(rng, len(pat.col), dtype, ints)
        b, B = _dense(rng, pat.m, w, dtype, ints)
        C = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
        ref = cr.spmm(pat.crow, pat.col, v, b)
        if ints:
            _same(f"one lane per row {kind} exact", _host(C), _stored(ref, dtype))
        else:
            _hold(cc.SPMM, dtype, f"one lane per row {kind}", _host(C), ref, cr.spmm_abs(pat.crow, pat.col, v, b), pat.lens[:, None])
    if dtype != torch.bfloat16:
        _dot_case(dtype, w, pat, torch.int32, f"dot one lane per row {kind}")


@pytest.mark.parametrize("itype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm_value_permutation_and_transposed_walk(dtype, itype):
    from torchsparsegradutils_amd import _pattern

    w = cc.WIDE[dtype]
    for p, name in ((2 * w, "ragged"), (3, "pass-edges"), (w, "uniform-stream")):
        pat = cr.build(name, cc.query(cc.SPMM, dtype, p), np.random.default_rng(7))
        cr.check_claim(pat)
        rng = np.random.default_rng(8)
        crow, col = _index(pat.crow, itype), _index(pat.col, itype)
        for ints in (True, False):
            # PERM: entry k uses val[q[k]]
            v, vt = _values(rng, len(pat.col), dtype, ints)
            q = rng.permutation(len(pat.col))
            assert len(q) < 2 or (q != np.arange(len(q))).any()
            b, B = _dense(rng, pat.m, p, dtype, ints)
            C = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, perm=_index(q, itype), max_row_nnz=_longest(pat))
            ref = cr.spmm(pat.crow, pat.col, v, b, perm=q)
            if ints:
                _same(f"perm {name} exact", _host(C), _stored(ref, dtype))
            else:
                _hold(cc.SPMM, dtype, f"perm p={p} {name}", _host(C), ref, cr.spmm_abs(pat.crow, pat.col, v, b, perm=q), pat.lens[:, None])
            # Aᵀ·G through the transposed pattern, whose perm addresses A's own values
            t = _pattern.RowGather(crow, col, pat.n, pat.m).transposed
            tptr, tidx, tperm = cr.transpose(pat.crow, pat.col, pat.m)
            assert t.crow.dtype == t.col.dtype == t.perm.dtype == itype
            assert np.array_equal(t.crow.cpu().numpy(), tptr) and np.array_equal(t.col.cpu().numpy(), tidx) and \
                np.array_equal(t.perm.cpu().numpy(), tperm)
            g, G = _dense(rng, pat.n, p, dtype, ints)
            tl = np.diff(tptr)
            geo = cr.Geom(*_be().csr_geometry(cc.SPMM, dtype, pat.m, len(pat.col), p, int(tl.max())))
            assert geo[:4] == cc.expected(cc.SPMM, dtype, p, "ok", pat.m, len(pat.col), int(tl.max()))
            Ct = _be().csr_spmm(t.crow, t.col, vt.to(DEV), G, pat.m, pat.n, perm=t.perm, max_row_nnz=int(tl.max()))
            ref = cr.spmm(tptr, tidx, v, g, perm=tperm)
            if ints:
                _same(f"transposed {name} exact", _host(Ct), _stored(ref, dtype))
            else:
                _hold(cc.SPMM, dtype, f"transposed p={p} {name}", _host(Ct), ref, cr.spmm_abs(tptr, tidx, v, g, perm=tperm), tl[:, None])


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm_out_view_batches_and_degenerate_sizes(dtype):
    w = cc.WIDE[dtype]
    p = 2 * w
    pat = cr.build("ragged", cc.query(cc.SPMM, dtype, p), np.random.default_rng(9))
    rng = np.random.default_rng(10)
    crow, col = _index(pat.crow, torch.int32), _index(pat.col, torch.int32)
    # out=: a view with ldc = p + wide
    v, vt = _values(rng, len(pat.col), dtype, True)
    b, B = _dense(rng, pat.m, p, dtype, True)
    buf = torch.full((pat.n, p + w), 7.0, dtype=dtype, device=DEV)
    out = buf[:, :p]
    assert _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, out=out, max_row_nnz=5) is out
    _same("out view", _host(out), _stored(cr.spmm(pat.crow, pat.col, v, b), dtype))
    assert (buf[:, p:] == 7.0).all(), "columns beyond p of the out buffer were written"
    # a batch of 3: the same row lengths, other columns; contiguous operands keep 16-byte lanes, an item stride of m·p + 1 does not
    cols = [cr.columns(np.random.default_rng(11 + k), pat.lens, pat.m)[1] for k in range(3)]
    bcrow = _index(np.stack([pat.crow] * 3), torch.int64)
    bcol = _index(np.stack(cols), torch.int64)
    for keeps in (True, False):
        geo = cr.Geom(*_be().csr_geometry(cc.SPMM, dtype, pat.n, len(pat.col), p, 5, wide_ok=keeps))
        assert (geo.vec, geo.cl, geo.ep) == ((w, 2, 4) if keeps else (1, 2 * w if 2 * w >= 8 else 4, 1 if 2 * w >= 8 else 2))
        for ints in (True, False):
            v3, v3t = _values(rng, (3, len(pat.col)), dtype, ints)
            b3, b3t = _values(rng, (3, pat.m, p), dtype, ints)
            if keeps:
                B3 = b3t.to(DEV)
            else:
                flat = torch.zeros(3 * (pat.m * p + 1), dtype=dtype, device=DEV)
                B3 = flat.as_strided((3, pat.m, p), (pat.m * p + 1, p, 1))
                B3.copy_(b3t)
            assert (B3.stride(0) % w == 0) == keeps
            C3 = _be().csr_spmm(bcrow, bcol, v3t.to(DEV), B3, pat.n, pat.m, max_row_nnz=5)
            assert C3.shape == (3, pat.n, p)
            for k in range(3):
                ref = cr.spmm(pat.crow, cols[k], v3[k], b3[k])
                if ints:
                    _same(f"batch item {k} lanes={keeps}", _host(C3[k]), _stored(ref, dtype))
                else:
                    _hold(cc.SPMM, dtype, f"batch item {k} lanes={keeps}", _host(C3[k]), ref, cr.spmm_abs(pat.crow, cols[k], v3[k], b3[k]),
                          pat.lens[:, None])
    # no columns; no entries (with rows and columns)
    C0 = _be().csr_spmm(crow, col, vt.to(DEV), torch.empty((pat.m, 0), dtype=dtype, device=DEV), pat.n, pat.m)
    assert C0.shape == (pat.n, 0)
    none = _index(np.zeros(pat.n + 1), torch.int32)
    Cz = _be().csr_spmm(none, col[:0], vt[:0].to(DEV), B, pat.n, pat.m)
    assert Cz.shape == (pat.n, p) and not Cz.any()


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_spmm_column_strided_operand(dtype):
    """B = Bt.t(): one column per grid.z slice, lanes along the rows — one lane per row for nnz <= 16 n, 8 entry lanes beyond."""
    w = cc.WIDE[dtype]
    rng = np.random.default_rng(12)
    for p, dense_rows in ((3, False), (w, True), (2 * w + 1, False)):
        q = cc.query(cc.SPMM, dtype, p, col_strided=True)
        if dense_rows:
            lens = np.full(2 * 32 + 3, 20)
            crow, col = cr.columns(rng, lens, 80)
            pat = cr.Pattern("rows of 20", crow, col, len(lens), 80, lens, q(len(lens), len(col), 20), {}, True)
        else:
            pat = cr.build("ragged", q, rng)
            cr.check_claim(pat)
        g = pat.geom
        assert (g.vec, g.cl, g.ep, g.tiles) == (1, 1, 8 if dense_rows else 1, p), g
        assert (len(pat.col) > 16 * pat.n) == dense_rows
        for ints in (True, False):
            v, vt = _values(rng, len(pat.col), dtype, ints)
            b, bt = _values(rng, (pat.m, p), dtype, ints)
            B = bt.t().contiguous().to(DEV).t()
            assert B.shape == (pat.m, p) and B.stride() == (1, pat.m) and _be().is_transposed_view(B)
            C = _be().csr_spmm(_index(pat.crow, torch.int64), _index(pat.col, torch.int64), vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
            assert C.shape == (pat.n, p) and C.stride() == (1, pat.n), "the product comes back in the operand's layout"
            ref = cr.spmm(pat.crow, pat.col, v, b)
            if ints:
                _same(f"column-strided p={p} exact", _host(C), _stored(ref, dtype))
            else:
                _hold(cc.SPMM, dtype, f"column-strided p={p} {pat.name}", _host(C), ref, cr.spmm_abs(pat.crow, pat.col, v, b), pat.lens[:, None])


# ---- the dot epilogue -------------------------------------------------------------------------------------------------------------

def _dot_case(dtype, p, pat, itype, what):
    g = pat.geom
    rows = cr.rpb(g) * g.runs
    rng = np.random.default_rng(13)
    v, vt = _values(rng, len(pat.col), dtype, False)
    b, B = _dense(rng, pat.m, p, dtype, False)
    wv, W = _dense(rng, pat.n, p, dtype, False)
    crow, col = _index(pat.crow, itype), _index(pat.col, itype)
    C, partial = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, dot_w=W, max_row_nnz=_longest(pat))
    nblk = _be().load_library().tsgu_spmm_num_blocks(_be()._VTYPE[dtype], pat.n, len(pat.col), p, _longest(pat))
    assert partial.shape == (nblk, p) and nblk == -(-pat.n // rows), f"{what}: {partial.shape} partial rows for {nblk} / {rows} rows each"
    plain = _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, max_row_nnz=_longest(pat))
    assert torch.equal(C, plain), what + ": the product with the epilogue differs from the product without"
    _hold(cc.SPMM, dtype, what + " product", _host(C), cr.spmm(pat.crow, pat.col, v, b), cr.spmm_abs(pat.crow, pat.col, v, b), pat.lens[:, None])
    c = _host(C)
    _hold(cc.SPMM, dtype, what + " partial", _host(partial), cr.dot_partial(c, wv, rows), cr.dot_partial_abs(c, wv, rows), rows)


@pytest.mark.parametrize("i", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_csr_spmm_dot_partials(dtype, i):
    p, mode, itype, pat = cc.pattern(cc.SPMM, dtype, i)
    what = f"dot case {i} p={p} {mode} {pat.name} {tuple(pat.geom)}"
    if mode != "ok" and p % cc.WIDE[dtype] == 0:
        # the partial buffer is sized for 16-byte lanes whenever p allows them: operands that forbid them are refused
        rng = np.random.default_rng(14)
        v, vt = _values(rng, len(pat.col), dtype, False)
        _, B = _dense(rng, pat.m, p, dtype, False, mode)
        _, W = _dense(rng, pat.n, p, dtype, False)
        with pytest.raises(RuntimeError, match=r"tsgu_csr_spmm failed.*status -2"):
            _be().csr_spmm(_index(pat.crow, itype), _index(pat.col, itype), vt.to(DEV), B, pat.n, pat.m, dot_w=W, max_row_nnz=_longest(pat))
        return
    _dot_case(dtype, p, pat, itype, what)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_csr_spmm_dot_partials_with_row_runs_in_every_geometry(dtype):
    seen = set()
    for k, (p, mode) in enumerate(cc.widths(dtype)):
        if mode != "ok":
            continue
        pat = cr.build(("uniform-runsmid", "uniform-runs8")[k % 2], cc.query(cc.SPMM, dtype, p), np.random.default_rng(15))
        cr.check_claim(pat)
        assert pat.geom.runs > 1
        _dot_case(dtype, p, pat, (torch.int32, torch.int64)[k // 2 % 2], f"dot runs={pat.geom.runs} p={p} {pat.name}")
        seen.add((pat.geom.vec > 1, pat.geom.cl, pat.geom.ep))
    assert len(seen) >= 13, seen      # 7 column-lane counts in 16-byte lanes, 6 (7 where 2 is no multiple of `wide`) in scalar lanes


def test_csr_spmm_dot_refuses_a_value_permutation_and_bfloat16():
    pat = cr.build("ragged", cc.query(cc.SPMM, torch.float32, 8), np.random.default_rng(16))
    rng = np.random.default_rng(17)
    crow, col = _index(pat.crow, torch.int32), _index(pat.col, torch.int32)
    for dtype, perm in ((torch.float32, True), (torch.bfloat16, False)):
        _, vt = _values(rng, len(pat.col), dtype, False)
        _, B = _dense(rng, pat.m, 8, dtype, False)
        _, W = _dense(rng, pat.n, 8, dtype, False)
        q = _index(rng.permutation(len(pat.col)), torch.int32) if perm else None
        with pytest.raises(RuntimeError, match=r"tsgu_csr_spmm failed.*status -2"):
            _be().csr_spmm(crow, col, vt.to(DEV), B, pat.n, pat.m, perm=q, dot_w=W, max_row_nnz=5)


# ---- csr_sddmm --------------------------------------------------------------------------------------------------------------------

def _alpha_exact(d, alpha, dtype):
    """alpha · (an exact integer dot) as the kernel forms it: alpha in the accumulator's type, one rounding per format."""
    if dtype == torch.float64:
        return alpha * d
    return _stored((np.float32(alpha) * d.astype(np.float32)).astype(np.float64), dtype)


@pytest.mark.parametrize("i", CASES)
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_sddmm(dtype, i):
    p, mode, itype, pat = cc.pattern(cc.SDDMM, dtype, i)
    rng = np.random.default_rng(100 + i)
    crow, col = _index(pat.crow, itype), _index(pat.col, itype)
    alpha = (1.0, -0.37)[i % 2]
    what = f"case {i} p={p} {mode} {pat.name} {str(itype)[6:]} alpha={alpha} {tuple(pat.geom)}"
    for ints in (True, False):
        r, R = _dense(rng, pat.n, p, dtype, ints)
        c, Cm = _dense(rng, pat.m, p, dtype, ints, mode)
        out = _be().csr_sddmm(crow, col, R, Cm, pat.n, pat.m, alpha=alpha)
        assert out.shape == (len(pat.col),) and out.dtype == dtype
        if ints:
            _same(what + " exact", _host(out), _alpha_exact(cr.sddmm(pat.crow, pat.col, r, c, 1.0), alpha, dtype))
        elif len(pat.col):
            _hold(cc.SDDMM, dtype, what, _host(out), cr.sddmm(pat.crow, pat.col, r, c, alpha), cr.sddmm_abs(pat.crow, pat.col, r, c, alpha), p + 1)
            assert torch.equal(out, _be().csr_sddmm(crow, col, R, Cm, pat.n, pat.m, alpha=alpha)), what + ": two runs differ"


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_csr_sddmm_swapped_roles_batches_and_no_columns(dtype):
    w = cc.WIDE[dtype]
    rng = np.random.default_rng(18)
    for p in (3 * w, 5):
        pat = cr.build("ragged", cc.query(cc.SDDMM, dtype, p), np.random.default_rng(19))
        assert pat.m != pat.n
        crow, col = _index(pat.crow, torch.int32), _index(pat.col, torch.int32)
        rows = np.repeat(np.arange(pat.n), pat.lens)
        for ints in (True, False):
            # swapped roles: out[k] = alpha <G[col k], B[row k]>; G in a buffer `wide` columns wider, B contiguous
            g, G = _dense(rng, pat.m, p, dtype, ints, pad=w)
            b, B = _dense(rng, pat.n, p, dtype, ints)
            assert G.stride(0) == p + w and B.stride(0) == p
            out = _be().csr_sddmm(crow, col, G, B, pat.n, pat.m, alpha=-0.37, swap_roles=True)
            if ints:
                _same(f"swapped p={p} exact", _host(out), _alpha_exact(cr.coo_sddmm(pat.col, rows, g, b, 1.0), -0.37, dtype))
            else:
                _hold(cc.SDDMM, dtype, f"swapped p={p}", _host(out), cr.coo_sddmm(pat.col, rows, g, b, -0.37),
                      cr.coo_sddmm_abs(pat.col, rows, g, b, -0.37), p + 1)
            # a batch of 3
            cols = [cr.columns(np.random.default_rng(20 + k), pat.lens, pat.m)[1] for k in range(3)]
            r3, r3t = _values(rng, (3, pat.n, p), dtype, ints)
            c3, c3t = _values(rng, (3, pat.m, p), dtype, ints)
            out3 = _be().csr_sddmm(_index(np.stack([pat.crow] * 3), torch.int64), _index(np.stack(cols), torch.int64), r3t.to(DEV), c3t.to(DEV),
                                   pat.n, pat.m, alpha=1.0)
            assert out3.shape == (3, len(pat.col))
            for k in range(3):
                if ints:
                    _same(f"batch item {k} p={p}", _host(out3[k]), _stored(cr.sddmm(pat.crow, cols[k], r3[k], c3[k], 1.0), dtype))
                else:
                    _hold(cc.SDDMM, dtype, f"batch item {k} p={p}", _host(out3[k]), cr.sddmm(pat.crow, cols[k], r3[k], c3[k], 1.0),
                          cr.sddmm_abs(pat.crow, cols[k], r3[k], c3[k], 1.0), p + 1)
    zero = _be().csr_sddmm(crow, col, torch.empty((pat.n, 0), dtype=dtype, device=DEV), torch.empty((pat.m, 0), dtype=dtype, device=DEV),
                           pat.n, pat.m, alpha=-0.37)
    assert zero.shape == (len(pat.col),) and not zero.any(), "no columns: every dot is zero"


# ---- coo_sddmm --------------------------------------------------------------------------------------------------------------------

def _coo_check(dtype, p, mode, row, col, n, m, itype, alpha, rng, what):
    for ints in (True, False):
        r, R = _dense(rng, n, p, dtype, ints)
        c, Cm = _dense(rng, m, p, dtype, ints, mode)
        out = _be().coo_sddmm(_index(row, itype), _index(col, itype), R, Cm, alpha=alpha)
        assert out.shape == (len(row),) and out.dtype == dtype
        if ints:
            _same(what + " exact", _host(out), _alpha_exact(cr.coo_sddmm(row, col, r, c, 1.0), alpha, dtype))
        elif len(row):
            _hold(cc.COO, dtype, what, _host(out), cr.coo_sddmm(row, col, r, c, alpha), cr.coo_sddmm_abs(row, col, r, c, alpha), p + 1)


@pytest.mark.parametrize("i", CASES)
@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_coo_sddmm(dtype, i):
    """The entries of the case's pattern, a fifth of them twice, in a shuffled order."""
    p, mode, itype, pat = cc.pattern(cc.COO, dtype, i)
    rng = np.random.default_rng(200 + i)
    row, col = np.repeat(np.arange(pat.n), pat.lens), pat.col
    pick = rng.permutation(np.concatenate([np.arange(len(col)), rng.integers(0, max(len(col), 1), len(col) // 5)]))
    row, col = row[pick], col[pick]
    if len(col) >= 10:
        assert (np.diff(row) < 0).any() and len(np.unique(row * pat.m + col)) < len(col), "unsorted, with duplicates"
    _coo_check(dtype, p, mode, row, col, pat.n, pat.m, itype, (1.0, -0.37)[i % 2], rng, f"case {i} p={p} {mode} {pat.name} {tuple(pat.geom)}")


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_coo_sddmm_entry_counts_around_a_workgroup(dtype):
    rng = np.random.default_rng(21)
    for k, (p, mode) in enumerate(cc.widths(dtype)):
        g = cc.query(cc.COO, dtype, p, mode)(0, 1, 0)
        assert (g.vec, g.cl, g.ep, g.tiles) == cc.expected(cc.COO, dtype, p, mode)
        epb = 256 // g.cl
        for nnz in (1, epb - 1, epb + 1, 3 * epb + 5):
            row, col = rng.integers(0, 37, nnz), rng.integers(0, 41, nnz)
            _coo_check(dtype, p, mode, row, col, 37, 41, (torch.int32, torch.int64)[k % 2], -0.37, rng, f"p={p} {mode} nnz={nnz}")
    out = _be().coo_sddmm(_index(row, torch.int32), _index(col, torch.int32), torch.empty((37, 0), dtype=dtype, device=DEV),
                          torch.empty((41, 0), dtype=dtype, device=DEV), alpha=2.0)
    assert out.shape == (nnz,) and not out.any()


def test_coo_sddmm_grid_stride():
    """More entries than the 2^20 workgroups of the largest grid cover in one pass (4 entries each at p = 256): rows and columns of 8
    dense rows, so that the float64 reference is an 8 × 8 table."""
    dtype, p, nnz = torch.float32, 256, 4 * 2 ** 20 + 7
    g = cc.query(cc.COO, dtype, p)(0, nnz, 0)
    assert (g.vec, g.cl, g.tiles) == (4, 64, 1) and -(-nnz // (256 // g.cl)) > 2 ** 20, "the case has lost its point: one pass covers it"
    rng = np.random.default_rng(22)
    r, R = _dense(rng, 8, p, dtype, False)
    c, Cm = _dense(rng, 8, p, dtype, False)
    row = torch.randint(0, 8, (nnz,), dtype=torch.int32, device=DEV)
    col = torch.randint(0, 8, (nnz,), dtype=torch.int32, device=DEV)
    out = _be().coo_sddmm(row, col, R, Cm, alpha=-0.37)
    table = -0.37 * (r @ c.T)
    bound = (p + 3) * EPS[dtype] * 0.37 * (np.abs(r) @ np.abs(c).T)
    flat = (row.long() * 8 + col.long())
    ref = torch.from_numpy(table).to(DEV).reshape(-1)[flat]
    lim = torch.from_numpy(bound).to(DEV).reshape(-1)[flat]
    ratio = float(((out.double() - ref).abs() / lim).max())
    print(f"coo_sddmm f32 grid stride nnz={nnz}: max |err| / bound = {ratio:.4f}")
    RATIOS[("coo_sddmm", "f32")] = max(RATIOS.get(("coo_sddmm", "f32"), 0.0), ratio)
    assert ratio <= 1.0
    # every entry of a (row, column) pair holds the same bits, the tail beyond the last full pass included
    last = torch.full((64,), -1, dtype=torch.long, device=DEV).scatter_reduce(0, flat, torch.arange(nnz, device=DEV), "amax")
    assert (last >= 0).all() and torch.equal(out, out[last][flat])


# ---- csr_mm_backward --------------------------------------------------------------------------------------------------------------

def _backward_operands(pat, itype):
    """The walked pattern `pat` is Aᵀ: A (pat.m × pat.n) in CSR, and A's transposed plan — pat itself, with the position of each of its
    entries in A's value array (a non-trivial permutation as soon as two rows of Aᵀ share a column)."""
    a_crow, a_col, a_from = cr.transpose(pat.crow, pat.col, pat.m)
    tperm = np.argsort(a_from, kind="stable")
    tptr, tidx, tp = cr.transpose(a_crow, a_col, pat.n)
    assert np.array_equal(tptr, pat.crow) and np.array_equal(tidx, pat.col) and np.array_equal(tp, tperm)
    plan = types.SimpleNamespace(crow=_index(pat.crow, itype), col=_index(pat.col, itype), perm=_index(tperm, itype))
    return a_crow, a_col, tperm, plan


@pytest.mark.parametrize("i", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_csr_mm_backward(dtype, i):
    p, mode, itype, pat = cc.pattern(cc.BACKWARD, dtype, i, True)
    assert pat.geom.tiles == 1 and pat.geom.stage == 1024
    a_crow, a_col, tperm, plan = _backward_operands(pat, itype)
    if pat.name in ("ragged", "pass-edges", "uniform-stream") and len(pat.col) > 1:
        assert (tperm != np.arange(len(tperm))).any(), "the case has lost its point: the permutation is the identity"
    rng = np.random.default_rng(300 + i)
    what = f"case {i} p={p} {mode} {pat.name} {str(itype)[6:]} {tuple(pat.geom)}"
    for ints in (True, False):
        v, vt = _values(rng, len(pat.col), dtype, ints)
        g, G = _dense(rng, pat.m, p, dtype, ints, mode)
        b, B = _dense(rng, pat.n, p, dtype, ints)
        gradA, gradB = _be().csr_mm_backward(plan, vt.to(DEV), G, B, pat.m, pat.n)
        assert gradA.shape == (len(pat.col),) and gradB.shape == (pat.n, p)
        ra, rb = cr.backward(a_crow, a_col, v, g, b)
        if ints:
            _same(what + " gradA exact", _host(gradA), _stored(ra, dtype))
            _same(what + " gradB exact", _host(gradB), _stored(rb, dtype))
            continue
        aa, ab = cr.backward_abs(a_crow, a_col, v, g, b)
        if len(pat.col):
            _hold(cc.BACKWARD, dtype, what + " gradA", _host(gradA), ra, aa, p + 1)
        _hold(cc.BACKWARD, dtype, what + " gradB", _host(gradB), rb, ab, pat.lens[:, None])
        # the pair K3 + K2 on the same operands.  Both sum a row of Aᵀ in entry order when a row has ONE entry lane; with several,
        # the lanes take the entries of a pass round-robin and a pass is 1024 entries here and 2048 there (and one lane per row is
        # the product's geometry alone), so the orders differ and the bound above is the statement.
        two = cr.Geom(*_be().csr_geometry(cc.SPMM, dtype, pat.n, len(pat.col), p, _longest(pat), mode == "ok"))
        if dtype == torch.float32 and pat.geom.ep == 1 and two.ep == 1 and len(pat.col):
            assert two.vec == pat.geom.vec and two.cl == pat.geom.cl
            pair = _be().csr_spmm(plan.crow, plan.col, vt.to(DEV), G, pat.n, pat.m, perm=plan.perm, max_row_nnz=_longest(pat))
            assert torch.equal(pair, gradB), what + ": gradB differs from csr_spmm(perm) in bits"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_csr_mm_backward_refuses_several_column_tiles_and_takes_a_pattern_plan(dtype):
    from torchsparsegradutils_amd import _pattern

    w = cc.WIDE[dtype]
    pat = cr.build("ragged", cc.query(cc.BACKWARD, dtype, 2 * w), np.random.default_rng(23))
    a_crow, a_col, tperm, plan = _backward_operands(pat, torch.int32)
    rng = np.random.default_rng(24)
    for p in (65 * w, 65):
        _, vt = _values(rng, len(pat.col), dtype, True)
        _, G = _dense(rng, pat.m, p, dtype, True)
        _, B = _dense(rng, pat.n, p, dtype, True)
        with pytest.raises(RuntimeError, match="tsgu_csr_geometry"):
            _be().csr_geometry(cc.BACKWARD, dtype, pat.n, len(pat.col), p)
        with pytest.raises(RuntimeError, match=r"tsgu_csr_mm_backward failed.*status -2"):
            _be().csr_mm_backward(plan, vt.to(DEV), G, B, pat.m, pat.n)
    # the plan the operator builds for A, `RowGather(...).transposed`, is the one above
    t = _pattern.RowGather(_index(a_crow, torch.int32), _index(a_col, torch.int32), pat.m, pat.n).transposed
    assert torch.equal(t.crow, plan.crow) and torch.equal(t.col, plan.col) and torch.equal(t.perm, plan.perm)
    v, vt = _values(rng, len(pat.col), dtype, True)
    g, G = _dense(rng, pat.m, 2 * w, dtype, True)
    b, B = _dense(rng, pat.n, 2 * w, dtype, True)
    gradA, gradB = _be().csr_mm_backward(t, vt.to(DEV), G, B, pat.m, pat.n)
    ra, rb = cr.backward(a_crow, a_col, v, g, b)
    _same("gradA", _host(gradA), _stored(ra, dtype))
    _same("gradB", _host(gradB), _stored(rb, dtype))


def test_zz_largest_error_to_bound_ratios():
    for (kernel, dtype), ratio in sorted(RATIOS.items()):
        print(f"largest |err| / bound: {kernel} {dtype} {ratio:.4f}")
    assert all(r <= 1.0 for r in RATIOS.values())
