"""`sparse_coloring`, the coloured `sparse_ilu0` / `sparse_ic0` and `sparse_sgs` without a GPU: the torch-op forms of `_cpu.py` against
the plain numpy reference (tests/_coloring_ref.py), the staged header csrc/tsgu_hip_color.h against its ctypes table and the
library, and the refusals of the public functions.

The error bounds are derived in `_coloring_ref`'s docstring.  `_trsm_ref.emulate` (random summation order in the value type) is held
against the same bounds on the same inputs: they are neither vacuous nor unreachable."""

import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import _abi_cases as A
import _coloring_ref as CR
import _factor_ref as FR
import _trsm_ref as TR
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _cpu, _pattern
from torchsparsegradutils_amd.utils import BICGSTABSettings, GMRESSettings, bicgstab, gmres, last_solve_info, linear_cg

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_color.h")
ENTRIES = ("tsgu_color_geometry", "tsgu_csr_color_round", "tsgu_csr_color_check", "tsgu_csr_color_sweep")
NP = {"f32": np.float32, "f64": np.float64}
TD = {"f32": torch.float32, "f64": torch.float64}


def csr(ptr, idx, val=None, idt=torch.int64, dtype=torch.float64):
    n = len(ptr) - 1
    val = np.ones(len(idx)) if val is None else val
    return torch.sparse_csr_tensor(torch.as_tensor(ptr).to(idt), torch.as_tensor(idx).to(idt), torch.as_tensor(np.asarray(val)).to(dtype), (n, n))


# ---- surface and refusals ------------------------------------------------------------------------------------------------------------

def test_surface():
    names = {"sparse_coloring", "SparseColoring", "sparse_sgs", "SparseSGS", "SparseColoredILU0", "SparseColoredIC0"}
    assert names <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_coloring import __all__ as mod_all

    assert set(mod_all) == names


def test_refusals():
    ptr, idx, _ = CR.case("stencil7_5x4x3")
    M = csr(ptr, idx)
    for f in (tsgu.sparse_coloring, tsgu.sparse_sgs):
        with pytest.raises(ValueError, match="COO or CSR sparse format"):
            f(torch.eye(4))
        with pytest.raises(ValueError, match="must be square"):
            f(torch.sparse_coo_tensor(torch.tensor([[0, 1], [0, 2]]), torch.ones(2), (2, 3)))
        with pytest.raises(ValueError, match="batched operands are not supported"):
            f(torch.stack([M.to_dense(), M.to_dense()]).to_sparse_csr())
    for f in (tsgu.sparse_ilu0, tsgu.sparse_ic0, tsgu.sparse_sgs):
        with pytest.raises(ValueError, match='ordering must be None, "multicolor" or a SparseColoring, got \'nonsense\''):
            f(M, ordering="nonsense")
    with pytest.raises(ValueError, match="colors must be 60 integers"):
        tsgu.sparse_coloring(M, colors=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="colors must be 60 integers"):
        tsgu.sparse_coloring(M, colors=torch.zeros(60))
    with pytest.raises(ValueError, match="made for another pattern"):
        tsgu.sparse_sgs(csr(*CR.case("path257")[:2]), ordering=tsgu.sparse_coloring(M))
    with pytest.raises(TypeError, match="float32 and float64 operands only"):
        tsgu.sparse_sgs(csr(ptr, idx, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="does not store its diagonal"):
        tsgu.sparse_sgs(csr(*CR.case("star300")[:2]))


# ---- the staged header ----------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_COLOR == {"tsgu_hip_color.h": _backend.SIGNATURES_COLOR}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES)
    assert not any(set(_backend.STAGED_COLOR) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_COLOR)
    assert not any(names & set(table) for reg in others for table in reg.values())
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_color.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_COLOR)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_COLOR[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION


def test_geometry_and_host_refusals():
    widths, window, sweep_widths, tile = _backend.color_geometry()
    assert widths == _backend.amg_geometry()[0] == (4, 8, 16, 32, 64) and window == 64 and sweep_widths == (8, 16, 32, 64) and tile == 8
    lib = _backend.load_library()
    refs = [ctypes.byref(ctypes.c_int()) for _ in range(6)]
    for k in range(6):
        assert lib.tsgu_color_geometry(*[None if j == k else r for j, r in enumerate(refs)]) == A.BAD_ARG
    # every call below is refused before the device is touched (fake addresses, device = -1: nothing is dereferenced)
    p = 0x10000
    rnd = dict(itype=0, n=8, nnz=8, ptr=p, idx=2 * p, nnz_t=8, tptr=3 * p, tidx=4 * p, a=5 * p, b=6 * p, word=7 * p, group=8)

    def call(name, args, **changes):
        return getattr(lib, name)(*{**args, **changes}.values(), -1, None)

    for name, third in (("tsgu_csr_color_round", "b"), ("tsgu_csr_color_check", None)):
        args = dict(rnd)
        if third is None:
            args = {k: (8 if k == "b" else v) for k, v in rnd.items()}      # (the check takes n_colors where the round takes `out`)
        assert call(name, args) == A.BAD_ARG                                  # set_device(-1): every argument check passed
        assert call(name, args, itype=2) == A.BAD_DTYPE
        assert call(name, args, n=1 << 31) == A.TOO_LARGE
        for key in ("ptr", "idx", "a", "word", "tidx"):
            assert call(name, args, **{key: None}) == A.BAD_ARG, (name, key)
        for key in ("ptr", "idx", "tptr", "tidx", "a", "word"):
            assert call(name, args, **{key: args[key] + 2}) == A.BAD_ARG, (name, key)
        for g in (0, 2, 3, 12, 128):
            assert call(name, args, group=g) == A.BAD_ARG
        assert call(name, args, n=-1) == A.BAD_ARG and call(name, args, nnz=-1) == A.BAD_ARG
        assert call(name, args, tptr=None, tidx=None, nnz_t=0) == A.BAD_ARG     # symmetric: accepted up to set_device
        assert call(name, args, tptr=None) == A.BAD_ARG
    assert call("tsgu_csr_color_round", rnd, b=rnd["a"] + 16) == A.BAD_ARG      # in and out overlap
    sw = dict(vtype=0, itype=0, mode=0, n=8, nnz=8, n_val=8, row0=0, row1=8, p=3, begin=p, end=2 * p, idx=3 * p, diag=4 * p, vmap=5 * p,
              val=6 * p, b=7 * p, ldb=3, bmap=8 * p, x=9 * p, ldx=3, out=10 * p, ldo=3, out_rows=11 * p, group=8)
    name = "tsgu_csr_color_sweep"
    assert call(name, sw) == A.BAD_ARG                                          # set_device(-1)
    assert call(name, sw, row0=4, row1=4) == A.OK and call(name, sw, p=0) == A.OK      # nothing to do
    assert call(name, sw, vtype=2) == A.BAD_DTYPE and call(name, sw, itype=2) == A.BAD_DTYPE
    for key in ("begin", "end", "idx", "diag", "val", "b", "x"):
        assert call(name, sw, **{key: None}) == A.BAD_ARG, key
    assert call(name, sw, out=None) == A.BAD_ARG                                # out_rows without out
    for key in ("begin", "end", "idx", "diag", "vmap", "val", "b", "bmap", "x", "out", "out_rows"):
        assert call(name, sw, **{key: sw[key] + 2}) == A.BAD_ARG, key
    for key in ("ldb", "ldx", "ldo"):
        assert call(name, sw, **{key: 2}) == A.BAD_ARG, key
    for bad in (dict(mode=3), dict(mode=-1), dict(row0=-1), dict(row1=9), dict(row0=5, row1=4), dict(n=-1), dict(nnz=-1), dict(group=4),
                dict(group=12), dict(group=128), dict(b=sw["x"] + 4), dict(out=sw["x"] + 4), dict(b=sw["x"]), dict(b=sw["x"], bmap=None, ldb=4)):
        assert call(name, sw, **bad) == A.BAD_ARG, bad
    assert call(name, sw, n=1 << 31, row1=8) == A.TOO_LARGE
    assert call(name, sw, mode=1, diag=None) == A.BAD_ARG                       # unit: no diagonal needed, refused by set_device only
    wide = dict(p=8 * 70000, ldb=8 * 70000, ldx=8 * 70000, ldo=8 * 70000, b=1 << 40, x=2 << 40, out=3 << 40)
    assert call(name, sw, **wide) == A.TOO_LARGE                                # more than 65535 column tiles


# ---- the colouring ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CR.PATTERNS))
def test_colouring_equals_the_reference(name):
    ptr, idx, ref = CR.case(name)
    assert CR.is_valid(ptr, idx, ref) and ref.max() + 1 <= CR.max_degree(ptr, idx) + 1       # first fit: a theorem, not a measurement
    for idt in (torch.int32, torch.int64):
        c = tsgu.sparse_coloring(csr(ptr, idx, idt=idt))
        assert c.colors.dtype == torch.int32 and np.array_equal(c.colors.numpy(), ref), name
        assert c.n_colors == ref.max() + 1
        perm, inverse, offsets = CR.permutation(ref)
        assert np.array_equal(c.perm.numpy(), perm) and np.array_equal(c.inverse.numpy(), inverse) and c.offsets == tuple(offsets)
    g = _pattern.from_csr(csr(ptr, idx))
    assert _pattern.check_colors(g, torch.as_tensor(ref), int(ref.max()) + 1) == 0
    assert (_pattern._color_lists(g)[2] is None) == (name not in ("one_sided300", "random1031"))
    if len(ptr) > 2 and ptr[-1] > len(ptr) - 1:
        bad = ref.copy()
        i = next(i for i, a in enumerate(CR.neighbours(ptr, idx)) if a)
        j = min(CR.neighbours(ptr, idx)[i])
        bad[i] = bad[j]
        want = CR.first_clash(ptr, idx, bad, int(ref.max()) + 1)
        assert want == min(i, j) + 1 == _pattern.check_colors(g, torch.as_tensor(bad), int(ref.max()) + 1)
    assert _pattern.check_colors(g, torch.as_tensor(ref), int(ref.max())) == int(np.argmax(ref == ref.max())) + 1      # a colour out of range


def test_complete_graph_uses_the_second_window():
    assert CR.case("complete70")[2].max() == 69 and sorted(CR.case("complete70")[2]) == list(range(70))


def test_coo_and_unsorted_operands():
    ptr, idx, ref = CR.case("one_sided300")
    M = csr(ptr, idx, val=np.arange(1, len(idx) + 1, dtype=np.float64))
    coo = M.to_sparse_coo()
    assert np.array_equal(tsgu.sparse_coloring(coo).colors.numpy(), ref)
    flip = torch.randperm(coo._nnz(), generator=torch.Generator().manual_seed(0))
    shuffled = torch.sparse_coo_tensor(coo.indices()[:, flip], coo.values()[flip], coo.shape)
    c = tsgu.sparse_coloring(shuffled)
    assert np.array_equal(c.colors.numpy(), ref)
    assert torch.equal(c.permute(shuffled).to_dense(), M.to_dense()[c.perm][:, c.perm])


# ---- permutation ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["stencil7_5x4x3", "one_sided300", "complete70"])
def test_permutation(name):
    ptr, idx, ref = CR.case(name)
    rng = np.random.default_rng(1)
    val = rng.standard_normal(len(idx))
    M = csr(ptr, idx, val)
    c = tsgu.sparse_coloring(M)
    perm = c.perm.numpy()
    assert sorted(perm) == list(range(len(ref)))
    key = ref[perm].astype(np.int64) * len(ref) + perm
    assert np.all(np.diff(key) > 0)                                                             # ordered by (colour, index)
    PA = c.permute(M)
    assert PA.layout == torch.sparse_csr and torch.equal(PA.to_dense(), M.to_dense()[c.perm][:, c.perm])
    pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, val, c.inverse.numpy())
    assert np.array_equal(PA.crow_indices().numpy(), pptr) and np.array_equal(PA.col_indices().numpy(), pidx)
    assert np.array_equal(PA.values().numpy(), pval)
    X = torch.arange(len(ref) * 2, dtype=torch.float64).reshape(-1, 2)
    assert torch.equal(c.permute_rows(X), X[c.perm]) and torch.equal(c.unpermute_rows(c.permute_rows(X)), X)
    rows = np.repeat(np.arange(len(ref)), np.diff(pptr))
    assert not np.any((ref[perm][rows] == ref[perm][pidx]) & (rows != pidx))                    # no two rows of one colour are coupled


def test_gradients_flow_through_permute():
    ptr, idx, _ = CR.case("stencil7_5x4x3")
    c = tsgu.sparse_coloring(csr(ptr, idx))
    crow, col = torch.as_tensor(ptr), torch.as_tensor(idx)
    v0 = torch.randn(len(idx), dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    w = torch.randn(len(idx), dtype=torch.float64, generator=torch.Generator().manual_seed(3))

    def f(v):
        return (c.permute(torch.sparse_csr_tensor(crow, col, v, (60, 60))).values() * w).sum()

    assert torch.autograd.gradcheck(f, (v0,))
    coo = torch.sparse_coo_tensor(csr(ptr, idx).to_sparse_coo().indices(), v0, (60, 60)).coalesce()
    (g,) = torch.autograd.grad(c.permute(coo).values().sum(), v0)
    assert torch.equal(g, torch.ones_like(g))


def test_user_colours():
    ptr, idx = FR.stencil(5, 4, 3, 7)
    x, y, z = (a.ravel() for a in np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"))
    rb = (x + y + z) % 2
    M = csr(ptr, idx)
    c = tsgu.sparse_coloring(M, colors=torch.as_tensor(rb))
    assert c.n_colors == 2 and np.array_equal(c.colors.numpy(), rb) and c.offsets == (0, 30, 60)
    assert tsgu.sparse_coloring(M, colors=rb.tolist()).n_colors == 2
    assert tsgu.sparse_coloring(M).n_colors > 2 and tsgu.sparse_coloring(M).colors is tsgu.sparse_coloring(M).colors      # cached; not replaced
    bad = rb.copy()
    bad[17] = 1 - bad[17]
    low = CR.first_clash(ptr, idx, bad, 2) - 1
    assert low < 17
    with pytest.raises(ValueError, match=f"row {low} has a neighbour of its own colour"):
        tsgu.sparse_coloring(M, colors=torch.as_tensor(bad))
    with pytest.raises(ValueError, match="non-negative"):
        tsgu.sparse_coloring(M, colors=torch.as_tensor(rb - 1))


# ---- sweeps and applications within the bounds -------------------------------------------------------------------------------------------

def _within(x, x64, bnd, what):
    r = TR.ratio(x, x64, bnd)
    assert np.isfinite(r) and r <= 1.0, (what, r)
    return r


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_cpu_sweeps_within_the_bound(dtype):
    n, p = 200, 3
    ptr, idx, val = CR.trsm_matrix(n, TR.SEED)
    val = TR.round_to(val, dtype)
    colors = CR.greedy(ptr, idx)
    perm, inverse, offsets = CR.permutation(colors)
    pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, val, inverse)
    (bl, el), (bu, eu), diag = CR.sweep_arrays(pptr, pidx)
    B = TR.round_to(np.random.default_rng(4).standard_normal((n, p)), dtype)
    real = np.longdouble if dtype == "f64" else np.float64
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a))                       # noqa: E731
    tv, tb = t(pval.astype(NP[dtype])), t(B.astype(NP[dtype]))
    for lower, unit, mode, (b, e) in ((True, False, 0, (bl, el)), (False, False, 0, (bu, eu)), (True, True, 1, (bl, el)),
                                      (False, False, 2, (bu, eu))):
        rhs = CR.diagonal(pptr, pidx, pval)[:, None] * B if mode == 2 else B
        x64 = TR.solve64(pptr, pidx, pval, rhs, lower, unit, real=real)
        assert np.allclose(np.asarray(CR.sweep64(pptr, pidx, pval, B, offsets, lower, unit, scaled=mode == 2), dtype=np.float64),
                           np.asarray(x64, dtype=np.float64), rtol=1e-12, atol=1e-13)
        bnd = TR.bound(pptr, pidx, pval, x64, lower, unit, TR.U[dtype])
        X = torch.full((n, p), float("nan"), dtype=TD[dtype])
        k = len(offsets) - 1
        for c in (range(k) if lower else range(k - 1, -1, -1)):
            _cpu.csr_color_sweep(mode, t(b), t(e), t(pidx), None if unit else t(diag), tv, tb, X, int(offsets[c]), int(offsets[c + 1]))
        _within(X.numpy(), x64, bnd, (dtype, lower, unit, mode))
        em = TR.emulate(pptr, pidx, pval, rhs.astype(NP[dtype]), dtype, 9, lower=lower, unit=unit)
        r = _within(em, x64, bnd, ("emulation", dtype, lower, unit, mode))
        assert r > 1e-3, ("the bound is vacuous", r)


def _object(kind, M, **kw):
    return {"ilu0": tsgu.sparse_ilu0, "ic0": tsgu.sparse_ic0, "sgs": tsgu.sparse_sgs}[kind](M, **kw)


def application_case(kind, name, dtype, M_obj, transpose=False):
    """(x64, bound, stages, perm) of an application object's solve on a named problem: the reference of what the object holds."""
    c = M_obj.coloring
    inverse, perm = c.inverse.cpu().numpy(), c.perm.cpu().numpy()
    ptr, idx, val, _ = CR.problem(name)
    if kind == "sgs":
        pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, TR.round_to(val, dtype), inverse)
    else:
        pptr, pidx, _, _ = CR.permute_csr(ptr, idx, None, inverse)
        pval = M_obj.values.cpu().numpy().astype(np.float64)
    return CR.stages(kind, pptr, pidx, pval, transpose), perm


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,name", CR.APPLICATIONS)
def test_cpu_applications_within_the_bound(kind, name, dtype):
    ptr, idx, val, _ = CR.problem(name)
    n = len(ptr) - 1
    M = _object(kind, csr(ptr, idx, TR.round_to(val, dtype), dtype=TD[dtype]), ordering="multicolor")
    assert isinstance(M.coloring, tsgu.SparseColoring) and int(M.info) == 0
    real = np.longdouble if dtype == "f64" else np.float64
    rng = np.random.default_rng(6)
    for shape in ((n,), (n, 3)):
        R = TR.round_to(rng.standard_normal(shape), dtype)
        Rt = torch.as_tensor(R.astype(NP[dtype]))
        for transpose in (False, True):
            (first, second), perm = application_case(kind, name, dtype, M, transpose)
            x64, bnd = CR.application(first, second, R.reshape(n, -1)[perm], TR.U[dtype], real=real)
            for X in (M.solve(Rt, transpose=transpose), (M.T(Rt) if transpose else M(Rt))):
                assert X.shape == Rt.shape and X.dtype == Rt.dtype
                _within(X.numpy().reshape(n, -1)[perm], x64, bnd, (kind, name, dtype, shape, transpose))
            em = CR.emulate_application(first, second, R.reshape(n, -1)[perm].astype(NP[dtype]), dtype, 21)
            r = _within(em, x64, bnd, ("emulation", kind, name, dtype, shape, transpose))
            assert r > 1e-3, ("the bound is vacuous", r)


def test_factors_are_those_of_the_permuted_matrix():
    ptr, idx, val, _ = CR.problem("lap27_4x4x4")
    M = csr(ptr, idx, val)
    c = tsgu.sparse_coloring(M)
    ilu = tsgu.sparse_ilu0(M, ordering="multicolor")
    pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, val, c.inverse.numpy())
    assert np.array_equal(ilu.values.numpy(), FR.ilu0(pptr, pidx, pval)[0])
    assert torch.equal(ilu.values, tsgu.sparse_ilu0(c.permute(M)).values)
    ic = tsgu.sparse_ic0(M, ordering=c)
    assert torch.equal(ic.values, tsgu.sparse_ic0(c.permute(M)).values)
    L, U = ilu.L.to_dense(), ilu.U.to_dense()
    assert torch.equal(torch.tril(L, -1) + torch.triu(U), FR_dense(pptr, pidx, ilu.values.numpy())) and torch.equal(torch.diag(L), torch.ones(64, dtype=torch.float64))
    assert torch.equal(ic.U.to_dense(), ic.L.to_dense().t())
    assert ic.T is ic and ilu.T.T.solve(torch.ones(64, dtype=torch.float64)).equal(ilu.solve(torch.ones(64, dtype=torch.float64)))
    assert isinstance(ilu, tsgu.SparseColoredILU0) and isinstance(ic, tsgu.SparseColoredIC0)
    assert isinstance(tsgu.sparse_ilu0(M), tsgu.SparseILU0) and isinstance(tsgu.sparse_ic0(M), tsgu.SparseIC0)      # the default is untouched


def FR_dense(ptr, idx, val):
    return torch.as_tensor(FR.dense(ptr, idx, val))


def test_sgs_refresh_equals_a_fresh_build():
    ptr, idx, val, _ = CR.problem("convdiff7_5x4x3")
    M = tsgu.sparse_sgs(csr(ptr, idx, val))
    new = csr(ptr, idx, FR.dominant_values(ptr, idx, 99))
    R = torch.randn(60, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert M.refresh(new) is M
    fresh = tsgu.sparse_sgs(new)
    assert torch.equal(M(R), fresh(R)) and torch.equal(M.T(R), fresh.T(R))
    with pytest.raises(ValueError, match="must have the pattern and the dtype"):
        M.refresh(csr(*CR.case("path257")[:2]))


# ---- in the Krylov loops ---------------------------------------------------------------------------------------------------------------

def _rel_residual(Mat, x, b):
    return float(torch.linalg.norm(Mat @ x - b) / torch.linalg.norm(b))


@pytest.mark.parametrize("kind", ["ilu0", "ic0", "sgs"])
def test_krylov_loops_reach_their_tolerance(kind):
    b = torch.randn(120, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    ptr, idx, val, _ = CR.problem("lap7_6x5x4")
    S = csr(ptr, idx, val)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = linear_cg(S, b, tolerance=1e-10, eps=1e-20, stop_updating_after=1e-20, max_iter=200, max_tridiag_iter=0,
                      preconditioner=_object(kind, S, ordering="multicolor"))
    assert last_solve_info("linear_cg")["tolerance_reached"] and _rel_residual(S.to_dense(), x, b) < 1e-8
    if kind == "ic0":
        return
    ptr, idx, val, _ = CR.problem("convdiff7_5x4x3")
    N = csr(ptr, idx, val)
    b = b[:60]
    M = _object(kind, N, ordering="multicolor")
    x = bicgstab(N, b[:, 0], settings=BICGSTABSettings(reltol=1e-10, precon=M))
    assert _rel_residual(N.to_dense(), x, b[:, 0]) < 1e-8
    x = gmres(N, b, settings=GMRESSettings(reltol=1e-10, precon=M))
    assert _rel_residual(N.to_dense(), x, b) < 1e-8
    Ng = csr(ptr, idx, val).requires_grad_(True)
    x = tsgu.sparse_generic_solve(Ng, b, solve=lambda A_, B_: bicgstab(A_, B_, settings=BICGSTABSettings(reltol=1e-12, precon=M)),
                                  transpose_solve=lambda A_, B_: bicgstab(A_.t() if A_.layout != torch.sparse_csr else A_.to_dense().t(), B_,
                                                                          settings=BICGSTABSettings(reltol=1e-12, precon=M.T)))
    x.sum().backward()
    assert _rel_residual(N.to_dense(), x.detach(), b) < 1e-8 and Ng.grad is not None


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coloured_preconditioners_save_iterations_on_the_anisotropic_lattice(dtype):
    ptr, idx, val = CR.lattice7(8, 8, 8, (1.0, 1.0, 1000.0))
    S = csr(ptr, idx, val, dtype=TD[dtype])
    D = S.to_dense()
    b = torch.randn(512, dtype=TD[dtype], generator=torch.Generator().manual_seed(0))
    plain = CR.cg_iterations(D, b, None)
    ic = CR.cg_iterations(D, b, tsgu.sparse_ic0(S, ordering="multicolor"))
    sgs = CR.cg_iterations(D, b, tsgu.sparse_sgs(S))
    print(f"CG to 1e-4 on the 8x8x8 1:1:1000 lattice ({dtype}): plain {plain}, coloured IC(0) {ic}, SGS {sgs}")
    assert ic < plain and sgs < plain
