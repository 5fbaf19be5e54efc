"""The colour sweep kernel (csrc/color_impl.h, `tsgu_csr_color_sweep`) on an MI355X: whole triangular sweeps, one launch per colour
class between guard words, against the float64 substitution and the componentwise bound of tests/_trsm_ref.py (`ratio <= 1`; the
bound and its reachability are shown without a GPU in tests/test_coloring_cpu.py), the same bits on a second run and at every
group width, the edge cases of a class, and the refusals.  Needs an MI355X: `pytest -m gpu`."""

import numpy as np
import pytest
import torch

import _coloring_ref as CR
import _factor_ref as FR
import _trsm_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
TD = {"f32": torch.float32, "f64": torch.float64}
WIDTHS_P = (1, 3, 8, 33, 65)
GUARD = 64
MODES = {"lower": (True, False, 0), "upper": (False, False, 0), "lower_unit": (True, True, 1), "upper_scaled": (False, False, 2)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_extension():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _matrix(kind):
    if kind == "trsm":
        return CR.trsm_matrix(300, TR.SEED)
    ptr, idx = FR.stencil(5, 4, 3, 27)
    return ptr, idx, FR.dominant_values(ptr, idx, 3)


_CASES = {}


def case(kind, dtype):
    """The permuted matrix, its classes and, per mode, (x64, bound) at the widest p — computed once, read-only."""
    key = (kind, dtype)
    if key not in _CASES:
        ptr, idx, val = _matrix(kind)
        val = TR.round_to(val, dtype)
        n = len(ptr) - 1
        perm, inverse, offsets = CR.permutation(CR.greedy(ptr, idx))
        pptr, pidx, pval, order = CR.permute_csr(ptr, idx, val, inverse)
        B = TR.round_to(np.random.default_rng(12).standard_normal((n, max(WIDTHS_P))), dtype)
        real = np.longdouble if dtype == "f64" else np.float64
        refs = {}
        for mode, (lower, unit, code) in MODES.items():
            rhs = CR.diagonal(pptr, pidx, pval)[:, None] * B if code == 2 else B
            x64 = TR.solve64(pptr, pidx, pval, rhs, lower, unit, real=real)
            refs[mode] = (x64, TR.bound(pptr, pidx, pval, x64, lower, unit, TR.U[dtype]))
        _CASES[key] = dict(n=n, val=val, perm=perm, inverse=inverse, offsets=offsets, pptr=pptr, pidx=pidx, pval=pval, order=order, B=B,
                           arrays=CR.sweep_arrays(pptr, pidx), refs=refs)
    return _CASES[key]


def guarded(n, p, ld, dtype, fill=float("nan")):
    """An (n, p) view with leading dimension ld between two runs of GUARD guard words, and the whole buffer."""
    whole = torch.full((2 * GUARD + n * ld,), 777.0, dtype=dtype, device=DEV)
    body = whole[GUARD:GUARD + n * ld].view(n, ld)
    body.fill_(fill)
    return body[:, :p], whole


def guards_intact(whole, n, p, ld):
    body = whole[GUARD:GUARD + n * ld].view(n, ld)
    pad = body[:, p:]
    return bool((whole[:GUARD] == 777.0).all() and (whole[GUARD + n * ld:] == 777.0).all() and (pad.numel() == 0 or torch.isnan(pad).all()))


def run_sweep(c, dtype, mode, p, ld_extra, maps, group, idt, inplace=False):
    """One whole sweep through the launcher: (x in the permuted numbering, `out` in the original numbering or None)."""
    from torchsparsegradutils_amd import _backend

    lower, unit, code = MODES[mode]
    n, offsets = c["n"], c["offsets"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(idt)      # noqa: E731
    (bl, el), (bu, eu), diag = c["arrays"]
    begin, end = (t(bl), t(el)) if lower else (t(bu), t(eu))
    ld = p + ld_extra
    X, xw = guarded(n, p, ld, TD[dtype])
    Bp = c["B"][:, :p]
    if maps:
        val = torch.as_tensor(c["val"].astype(NP[dtype]), device=DEV)
        vmap, rows = t(c["order"]), t(c["perm"])
        Bsrc = Bp[c["inverse"]]
        out, ow = guarded(n, p, ld + 1, TD[dtype])
    else:
        val = torch.as_tensor(c["pval"].astype(NP[dtype]), device=DEV)
        vmap = rows = out = ow = None
        Bsrc = Bp
    if inplace:
        X.copy_(torch.as_tensor(Bsrc.astype(NP[dtype]), device=DEV))
        Bt = X
    else:
        Bt, _ = guarded(n, p, ld + 2, TD[dtype])
        Bt.copy_(torch.as_tensor(Bsrc.astype(NP[dtype]), device=DEV))
    k = len(offsets) - 1
    idx, dg = t(c["pidx"]), None if unit else t(diag)
    for cls in (range(k) if lower else range(k - 1, -1, -1)):
        _backend.csr_color_sweep(code, begin, end, idx, dg, val, Bt, X, int(offsets[cls]), int(offsets[cls + 1]),
                                 vmap=vmap, bmap=None if inplace else rows, out=out, out_rows=rows, group=group)
    torch.cuda.synchronize()
    assert guards_intact(xw, n, p, ld), "the sweep wrote outside x"
    if out is not None:
        assert guards_intact(ow, n, p, ld + 1), "the sweep wrote outside out"
    return X.cpu().numpy().copy(), None if out is None else out.cpu().numpy().copy()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["trsm", "stencil"])
def test_sweeps_within_the_bound_and_bit_stable(kind, mode, dtype):
    from torchsparsegradutils_amd import _backend

    c = case(kind, dtype)
    x64, bnd = c["refs"][mode]
    widths = _backend.color_geometry()[2]
    worst = 0.0
    for p in WIDTHS_P:
        first = None
        for group in widths:
            x, _ = run_sweep(c, dtype, mode, p, 0, False, group, torch.int32)
            if first is None:
                first = x
                r = TR.ratio(x, x64[:, :p], bnd[:, :p])
                worst = max(worst, r)
                assert np.isfinite(x).all() and r <= 1.0, (kind, mode, dtype, p, r)
                again, _ = run_sweep(c, dtype, mode, p, 0, False, group, torch.int32)
                assert np.array_equal(again.view(np.uint8), first.view(np.uint8)), "two runs differ"
            assert np.array_equal(x.view(np.uint8), first.view(np.uint8)), (kind, mode, dtype, p, group)
        # leading dimensions above p, the maps (values, right-hand side and result in the ORIGINAL numbering), 64-bit indices
        x, out = run_sweep(c, dtype, mode, p, 5, True, widths[0], torch.int64)
        assert np.array_equal(x.view(np.uint8), first.view(np.uint8)), (kind, mode, dtype, p, "maps")
        assert np.array_equal(out[c["perm"]].view(np.uint8), first.view(np.uint8)), (kind, mode, dtype, p, "out_rows")
        if mode != "lower":        # the second sweep of an application runs in place (b is x)
            x, _ = run_sweep(c, dtype, mode, p, 3, False, widths[-1], torch.int32, inplace=True)
            assert np.array_equal(x.view(np.uint8), first.view(np.uint8)), (kind, mode, dtype, p, "in place")
    print(f"{kind} {mode} {dtype}: worst error / bound = {worst:.3f}, {len(c['offsets']) - 1} colours")


def test_an_empty_class_and_a_class_of_one_row():
    from torchsparsegradutils_amd import _backend

    c = case("stencil", "f32")
    n = c["n"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(torch.int32)      # noqa: E731
    (bl, el), _, diag = c["arrays"]
    val = torch.as_tensor(c["pval"].astype(np.float32), device=DEV)
    B = torch.as_tensor(c["B"][:, :3].astype(np.float32), device=DEV).contiguous()
    X, xw = guarded(n, 3, 3, torch.float32, fill=5.0)
    before = xw.clone()
    for row in (0, 7, n):
        _backend.csr_color_sweep(0, t(bl), t(el), t(c["pidx"]), t(diag), val, B, X, row, row)
    torch.cuda.synchronize()
    assert torch.equal(xw, before)
    # row 0 of the first class has no entry below the diagonal: x = b / d, and nothing else is written
    _backend.csr_color_sweep(0, t(bl), t(el), t(c["pidx"]), t(diag), val, B, X, 0, 1)
    torch.cuda.synchronize()
    assert torch.equal(X[0], B[0] / val[int(diag[0])]) and torch.equal(xw[GUARD + 3:], before[GUARD + 3:]) and torch.equal(xw[:GUARD], before[:GUARD])


def test_refusals():
    from torchsparsegradutils_amd import _backend

    c = case("stencil", "f32")
    n = c["n"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(torch.int32)      # noqa: E731
    (bl, el), _, diag = c["arrays"]
    begin, end, idx, dg = t(bl), t(el), t(c["pidx"]), t(diag)
    B = torch.zeros((n, 4), dtype=torch.float32, device=DEV)
    X = torch.zeros((n, 4), dtype=torch.float32, device=DEV)
    val = torch.as_tensor(c["pval"].astype(np.float32), device=DEV)
    with pytest.raises(RuntimeError, match="unsupported value/index dtype"):
        _backend.csr_color_sweep(0, begin, end, idx, dg, val.bfloat16(), B.bfloat16(), X.bfloat16(), 0, 1)
    with pytest.raises(RuntimeError, match="tsgu_csr_color_sweep"):
        _backend.csr_color_sweep(0, begin, end[:-1], idx, dg, val, B, X, 0, 1)
    with pytest.raises(RuntimeError, match="tsgu_csr_color_sweep"):
        _backend.csr_color_sweep(0, begin, end, idx, dg, val, B.cpu(), X, 0, 1)
    with pytest.raises(RuntimeError, match="bad argument"):
        _backend.csr_color_sweep(0, begin, end, idx, dg, val, B, X, 0, 1, group=4)
    with pytest.raises(RuntimeError, match="bad argument"):
        big = torch.zeros((n + 1, 4), dtype=torch.float32, device=DEV)
        _backend.csr_color_sweep(0, begin, end, idx, dg, val, big[1:], big[:-1], 0, 1)      # b overlaps x without being x
    lib = _backend.load_library()
    nnz = idx.numel()

    def raw(**ch):
        a = dict(vtype=0, itype=0, mode=0, n=n, nnz=nnz, n_val=nnz, row0=0, row1=n, p=4, begin=begin.data_ptr(), end=end.data_ptr(),
                 idx=idx.data_ptr(), diag=dg.data_ptr(), vmap=None, val=val.data_ptr(), b=B.data_ptr(), ldb=4, bmap=None, x=X.data_ptr(),
                 ldx=4, out=None, ldo=0, out_rows=None, group=8)
        a.update(ch)
        return lib.tsgu_csr_color_sweep(*a.values(), 0, None)

    assert raw(vtype=2) == -1 and raw(itype=3) == -1
    for key in ("begin", "end", "idx", "diag", "val", "b", "x"):
        assert raw(**{key: None}) == -2, key
    for key, ptr in (("begin", begin), ("idx", idx), ("val", val), ("b", B), ("x", X)):
        assert raw(**{key: ptr.data_ptr() + 2}) == -2, key
    assert raw(ldb=3) == -2 and raw(ldx=3) == -2 and raw(out=B.data_ptr(), ldo=3) == -2
    torch.cuda.synchronize()
    assert not X.any()                     # nothing was launched
