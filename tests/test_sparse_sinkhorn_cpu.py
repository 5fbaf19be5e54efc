"""sparse_sinkhorn without a GPU: the torch-op path against the dense float64 restatement (tests/_sinkhorn_ref.py) in values,
potentials and all three gradients, the entry-wise restatement against the dense one, the result's index tensors, the refusals,
and the staged header csrc/tsgu_hip_sinkhorn.h against its ctypes table and the library.

Tolerance of the float64 comparisons.  Both sides compute the same T iterations in float64; the half-step maps are non-expansive
in the sup norm, so the roundings of the 2T half steps add: at most 2T·c·ε·M with ε = 2⁻⁵³, c ≤ 53 + 10 roundings on an entry's
way into a group of at most 53 entries, and M = |S| + |u| + |v| + |log marginal| < 100 here: below 1e-11 for T ≤ 5.  The
gradients are sums of at most 2T·nnz such terms weighted by cotangents of size O(1): 1e-9 (absolute, and relative to the largest
entry of the gradient) leaves two further digits.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _sinkhorn_ref as ref
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_sinkhorn

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_sinkhorn.h")
ENTRIES = ("tsgu_sinkhorn_workspace", "tsgu_sinkhorn_half", "tsgu_sinkhorn_plan", "tsgu_sinkhorn_half_backward", "tsgu_segment_sum")
F64 = torch.float64
N, M = 37, 53
POT_TOL, GRAD_TOL = 1e-11, 1e-9


def _pattern(seed, n=N, m=M, density=0.25, empty_row=5, empty_col=11):
    """Distinct sorted (row, col) positions of an n × m matrix without entries in one row and one column."""
    rng = np.random.default_rng(seed)
    keep = rng.random((n, m)) < density
    keep[np.arange(n), rng.integers(0, m, n)] = True      # every other row and column keeps an entry
    keep[rng.integers(0, n, m), np.arange(m)] = True
    if empty_row is not None:
        keep[empty_row, :] = False
    if empty_col is not None:
        keep[:, empty_col] = False
    r, c = np.nonzero(keep)       # (views with a stride into one array: copied, the index helpers want contiguous input)
    return torch.from_numpy(np.ascontiguousarray(r)), torch.from_numpy(np.ascontiguousarray(c))


def _problem(seed, given=True, **kw):
    rows, cols = _pattern(seed, **kw)
    g = torch.Generator().manual_seed(seed)
    vals = torch.randn(rows.numel(), dtype=F64, generator=g) * 3.0
    la = torch.randn(N, dtype=F64, generator=g) if given else None
    lb = torch.randn(M, dtype=F64, generator=g) if given else None
    cot = (torch.randn(rows.numel(), dtype=F64, generator=g), torch.randn(N, dtype=F64, generator=g),
           torch.randn(M, dtype=F64, generator=g))
    return rows, cols, vals, la, lb, cot


def _sparse(layout, rows, cols, vals, shape=(N, M), index_dtype=torch.int64):
    """The entries (row-major order) as a tensor of `layout` and, for CSC, the permutation of the values into its order."""
    if layout == "coo":
        return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, shape, is_coalesced=True), None
    if layout == "csr":
        crow = torch._convert_indices_from_coo_to_csr(rows, shape[0], out_int32=False)
        return torch.sparse_csr_tensor(crow.to(index_dtype), cols.to(index_dtype), vals, shape), None
    order = torch.argsort(cols * shape[0] + rows)
    ccol = torch._convert_indices_from_coo_to_csr(cols[order], shape[1], out_int32=False)
    return torch.sparse_csc_tensor(ccol.to(index_dtype), rows[order].to(index_dtype), vals[order], shape), order


def _values(X):
    return X._values() if X.layout == torch.sparse_coo else X.values()


def _close(got, want, tol, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    inf = want.isinf()
    assert torch.equal(got.isinf(), inf) and torch.equal(got[inf], want[inf]), (what, "infinities")
    assert not got.isnan().any(), (what, "NaN")
    err = (got[~inf] - want[~inf]).abs().max().item() if (~inf).any() else 0.0
    scale = max(1.0, want[~inf].abs().max().item()) if (~inf).any() else 1.0
    assert err <= tol * scale, (what, err, tol * scale)


def _run_and_compare(layout, seed, T, given, index_dtype=torch.int64, ninf_at=None):
    rows, cols, vals, la, lb, cot = _problem(seed, given)
    if ninf_at is not None:
        vals[ninf_at] = float("-inf")
    (lp_r, u_r, v_r), (dS_r, dla_r, dlb_r) = ref.with_grads(ref.dense, rows, cols, vals, N, M, la, lb, T, cot)
    leaf = vals.clone().requires_grad_(True)
    S, order = _sparse(layout, rows, cols, leaf, index_dtype=index_dtype)
    a = None if la is None else la.clone().requires_grad_(True)
    b = None if lb is None else lb.clone().requires_grad_(True)
    lp, u, v = sparse_sinkhorn(S, a, b, T)
    assert lp.layout == S.layout and lp.shape == S.shape
    pick = (lambda t: t) if order is None else (lambda t: t[order])
    _close(_values(lp).detach(), pick(lp_r), 3 * POT_TOL, "log_P")
    _close(u.detach(), u_r, POT_TOL, "u")
    _close(v.detach(), v_r, POT_TOL, "v")
    assert u_r[5] == float("inf") and v_r[11] == float("inf"), "the empty row and column"
    leaves = [leaf] + [t for t in (a, b) if t is not None]
    grads = list(torch.autograd.grad((lp, u, v), leaves, (_rebuild(lp, pick(cot[0])), cot[1], cot[2])))
    _close(grads.pop(0), dS_r, GRAD_TOL, "dS")
    if given:
        _close(grads.pop(0), dla_r, GRAD_TOL, "dlog_a")
        _close(grads.pop(0), dlb_r, GRAD_TOL, "dlog_b")
    return lp, S


def _rebuild(like, values):
    if like.layout == torch.sparse_csr:
        return torch.sparse_csr_tensor(like.crow_indices(), like.col_indices(), values, like.shape)
    if like.layout == torch.sparse_csc:
        return torch.sparse_csc_tensor(like.ccol_indices(), like.row_indices(), values, like.shape)
    return torch.sparse_coo_tensor(like._indices(), values, like.shape, is_coalesced=True)


def test_exported():
    assert {"sparse_sinkhorn", "SparseSinkhorn"} <= set(tsgu.__all__) and tsgu.sparse_sinkhorn is sparse_sinkhorn
    assert "sparse_sinkhorn" in tsgu.__doc__


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
@pytest.mark.parametrize("given", [True, False], ids=["marginals", "balancing"])
def test_against_the_dense_restatement(layout, T, given):
    _run_and_compare(layout, 3, T, given)


def test_int32_indices():
    _run_and_compare("csr", 4, 2, True, index_dtype=torch.int32)
    _run_and_compare("csc", 4, 2, True, index_dtype=torch.int32)


def test_dense_cotangent_of_log_P():
    rows, cols, vals, la, lb, cot = _problem(8)
    _, (dS_r, _, _) = ref.with_grads(ref.dense, rows, cols, vals, N, M, la, lb, 2, cot)
    leaf = vals.clone().requires_grad_(True)
    S, _ = _sparse("csr", rows, cols, leaf)
    lp, u, v = sparse_sinkhorn(S, la, lb, 2)
    G = torch.zeros(N, M, dtype=F64).index_put((rows, cols), cot[0])
    (dS,) = torch.autograd.grad((lp, u, v), leaf, (G, cot[1], cot[2]))
    _close(dS, dS_r, GRAD_TOL, "dS")


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_a_stored_minus_infinity_is_an_absent_entry(layout):
    rows, cols = _pattern(3)
    # an entry whose row and column both keep another, finite, entry
    counts_r, counts_c = torch.bincount(rows, minlength=N), torch.bincount(cols, minlength=M)
    at = int(torch.nonzero((counts_r[rows] > 1) & (counts_c[cols] > 1))[0])
    lp, S = _run_and_compare(layout, 3, 2, True, ninf_at=at)
    assert (_values(lp) == float("-inf")).sum() == 1


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_a_stored_minus_infinity_alone_in_its_row_and_in_its_column(layout):
    """The only entry of a column, and the only entry of a row, are −inf: those groups are empty for the forward (+inf potentials)
    and for the backward — no NaN anywhere, log_P stays −inf there, and every gradient is the restatement's."""
    rows, cols, vals, la, lb, cot = _problem(3)
    extra_r = torch.tensor([0, 5])           # (0, 11): alone in the empty column 11; (5, 0): alone in the empty row 5
    extra_c = torch.tensor([11, 0])
    key = torch.cat([rows, extra_r]) * M + torch.cat([cols, extra_c])
    order = torch.argsort(key)
    rows, cols = torch.cat([rows, extra_r])[order], torch.cat([cols, extra_c])[order]
    g = torch.Generator().manual_seed(31)
    vals = torch.cat([vals, torch.full((2,), float("-inf"), dtype=F64)])[order]
    gP = torch.randn(vals.numel(), dtype=F64, generator=g)
    alone = vals == float("-inf")
    T = 3
    (lp_r, u_r, v_r), (dS_r, dla_r, dlb_r) = ref.with_grads(ref.dense, rows, cols, vals, N, M, la, lb, T, (gP, cot[1], cot[2]))
    assert u_r[5] == float("inf") and v_r[11] == float("inf") and bool(lp_r[alone].isnan().all()) and not dS_r.isnan().any()
    leaf = vals.clone().requires_grad_(True)
    S, perm = _sparse(layout, rows, cols, leaf)
    a, b = la.clone().requires_grad_(True), lb.clone().requires_grad_(True)
    lp, u, v = sparse_sinkhorn(S, a, b, T)
    pick = (lambda t: t) if perm is None else (lambda t: t[perm])
    got = _values(lp).detach()
    assert bool((got[pick(alone)] == float("-inf")).all()), "an absent entry stays −inf beside the +inf potential"
    _close(got[~pick(alone)], pick(lp_r)[~pick(alone)], 3 * POT_TOL, "log_P")
    _close(u.detach(), u_r, POT_TOL, "u")
    _close(v.detach(), v_r, POT_TOL, "v")
    dS, dla, dlb = torch.autograd.grad((lp, u, v), (leaf, a, b), (_rebuild(lp, pick(gP)), cot[1], cot[2]))
    _close(dS, dS_r, GRAD_TOL, "dS")
    _close(dla, dla_r, GRAD_TOL, "dlog_a")
    _close(dlb, dlb_r, GRAD_TOL, "dlog_b")


def test_the_entrywise_restatement_is_the_dense_one():
    for T in (1, 5):
        for given in (True, False):
            rows, cols, vals, la, lb, cot = _problem(6, given)
            vals[7] = float("-inf")
            want = ref.with_grads(ref.dense, rows, cols, vals, N, M, la, lb, T, cot)
            got = ref.with_grads(ref.entries, rows, cols, vals, N, M, la, lb, T, cot)
            for g, w, what in zip(got[0] + tuple(t for t in got[1] if t is not None),
                                  want[0] + tuple(t for t in want[1] if t is not None), "P u v dS da db".split()):
                _close(g, w, GRAD_TOL, what)


def test_batched_items_with_different_patterns():
    T = 2
    items = [_problem(11, density=0.2), _problem(12, density=0.35)]
    refs = [ref.with_grads(ref.dense, r, c, x, N, M, la, lb, T, cot) for r, c, x, la, lb, cot in items]
    idx = torch.cat([torch.stack([torch.full_like(r, i), r, c]) for i, (r, c, *_) in enumerate(items)], dim=1)
    assert items[0][0].numel() != items[1][0].numel()
    leaf = torch.cat([it[2] for it in items]).requires_grad_(True)
    S = torch.sparse_coo_tensor(idx, leaf, (2, N, M), is_coalesced=True)
    la = torch.stack([it[3] for it in items]).requires_grad_(True)
    lb = torch.stack([it[4] for it in items]).requires_grad_(True)
    lp, u, v = sparse_sinkhorn(S, la, lb, T)
    assert u.shape == (2, N) and v.shape == (2, M) and lp.shape == (2, N, M)
    _close(lp._values().detach(), torch.cat([r[0][0] for r in refs]), 3 * POT_TOL, "log_P")
    _close(u.detach(), torch.stack([r[0][1] for r in refs]), POT_TOL, "u")
    _close(v.detach(), torch.stack([r[0][2] for r in refs]), POT_TOL, "v")
    gP = torch.sparse_coo_tensor(idx, torch.cat([it[5][0] for it in items]), (2, N, M), is_coalesced=True)
    gu, gv = torch.stack([it[5][1] for it in items]), torch.stack([it[5][2] for it in items])
    dS, dla, dlb = torch.autograd.grad((lp, u, v), (leaf, la, lb), (gP, gu, gv))
    _close(dS, torch.cat([r[1][0] for r in refs]), GRAD_TOL, "dS")
    _close(dla, torch.stack([r[1][1] for r in refs]), GRAD_TOL, "dlog_a")
    _close(dlb, torch.stack([r[1][2] for r in refs]), GRAD_TOL, "dlog_b")


def test_batched_csr():
    T = 2
    rows, cols, vals, la, lb, cot = _problem(13)
    rows2 = (N - 1) - rows.flip(0)          # another pattern with the same number of entries
    cols2 = cols.flip(0)
    vals2 = vals.flip(0) * 0.5
    r1 = ref.dense(rows, cols, vals, N, M, la, lb, T)
    r2 = ref.dense(rows2, cols2, vals2, N, M, la, lb, T)
    crow = torch.stack([torch._convert_indices_from_coo_to_csr(r, N, out_int32=False) for r in (rows, rows2)])
    S = torch.sparse_csr_tensor(crow, torch.stack([cols, cols2]), torch.stack([vals, vals2]), (2, N, M))
    lp, u, v = sparse_sinkhorn(S, torch.stack([la, la]), torch.stack([lb, lb]), T)
    _close(lp.values(), torch.stack([r1[0], r2[0]]), 3 * POT_TOL, "log_P")
    _close(u, torch.stack([r1[1], r2[1]]), POT_TOL, "u")
    _close(v, torch.stack([r1[2], r2[2]]), POT_TOL, "v")


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_no_entries(layout):
    e = torch.zeros(0, dtype=torch.int64)
    leaf = torch.zeros(0, dtype=F64, requires_grad=True)
    S, _ = _sparse(layout, e, e, leaf)
    la = torch.randn(N, dtype=F64, requires_grad=True)
    lp, u, v = sparse_sinkhorn(S, la, None, 3)
    assert _values(lp).numel() == 0 and (u == float("inf")).all() and (v == float("inf")).all()
    dS, dla = torch.autograd.grad((u, v), (leaf, la), (torch.ones(N, dtype=F64), torch.ones(M, dtype=F64)))
    assert dS.numel() == 0 and torch.equal(dla, torch.ones(N, dtype=F64))


def test_uncoalesced_coo_is_coalesced_first():
    rows, cols, vals, la, lb, cot = _problem(14)
    want = ref.dense(rows, cols, vals, N, M, la, lb, 2)
    idx = torch.stack([rows, cols])
    half = (vals * 0.5).requires_grad_(True)
    S = torch.sparse_coo_tensor(torch.cat([idx, idx], dim=1), torch.cat([half, half]), (N, M))
    lp, u, v = sparse_sinkhorn(S, la, lb, 2)
    _close(lp._values().detach(), want[0], 3 * POT_TOL, "log_P")
    (g,) = torch.autograd.grad(u[torch.isfinite(u)].sum(), half)
    assert g.shape == half.shape and g.abs().sum() > 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_accumulator_types(dtype):
    rows, cols, vals, la, lb, _ = _problem(15)
    x = vals.to(dtype)
    want = ref.dense(rows, cols, x.to(F64), N, M, la.float().to(F64), lb.float().to(F64), 3)
    S, _ = _sparse("csr", rows, cols, x)
    lp, u, v = sparse_sinkhorn(S, la.float(), lb.float(), 3)
    assert lp.dtype == dtype and u.dtype == torch.float32 and v.dtype == torch.float32
    # 2T half steps of at most (53 + 10) float32 roundings each on values below M = 100
    bound = 2 * 3 * 63 * 2.0 ** -24 * 100
    fin = want[1].isfinite()
    assert (u[fin].to(F64) - want[1][fin]).abs().max() <= bound and (v[want[2].isfinite()].to(F64) - want[2][want[2].isfinite()]).abs().max() <= bound
    err = (lp.values().to(F64) - want[0]).abs()
    # (one rounding to bfloat16: half a unit in the last of its 8 significant bits, at most 2⁻⁸·|log_P|)
    half_ulp = torch.ldexp(torch.ones_like(err), torch.frexp(want[0])[1] - 9) if dtype == torch.bfloat16 else 0
    assert (err <= 3 * bound + half_ulp).all()
    with pytest.raises(TypeError, match="log_a must have dtype torch.float32"):
        sparse_sinkhorn(S, la, lb.float(), 3)


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_the_result_carries_the_inputs_index_tensors(layout):
    rows, cols, vals, la, lb, _ = _problem(16)
    S, _ = _sparse(layout, rows, cols, vals.requires_grad_(True))
    lp, u, v = sparse_sinkhorn(S, la, lb, 2)
    (g,) = torch.autograd.grad(lp, S, _rebuild(lp, torch.ones_like(_values(lp))))

    def idx(X):
        if X.layout == torch.sparse_csr:
            return X.crow_indices(), X.col_indices()
        if X.layout == torch.sparse_csc:
            return X.ccol_indices(), X.row_indices()
        return (X._indices(),)
    for out in (lp, g):
        assert out.layout == S.layout and out.shape == S.shape
        for a, b in zip(idx(S), idx(out)):
            assert a.data_ptr() == b.data_ptr() and a.dtype == b.dtype and a.shape == b.shape


def test_a_second_differentiation_raises():
    rows, cols, vals, la, lb, _ = _problem(17)
    S, _ = _sparse("csr", rows, cols, vals.requires_grad_(True))
    la = la.requires_grad_(True)
    lp, u, v = sparse_sinkhorn(S, la, lb, 2)
    w = torch.ones(N, dtype=F64, requires_grad=True)
    (g,) = torch.autograd.grad(u, la, w, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        g.sum().backward()


def test_only_needed_gradients_are_returned():
    rows, cols, vals, la, lb, cot = _problem(18)
    S, _ = _sparse("csr", rows, cols, vals)
    lb = lb.requires_grad_(True)
    lp, u, v = sparse_sinkhorn(S, la, lb, 3)
    assert not S.requires_grad and lp.requires_grad
    (dlb,) = torch.autograd.grad((u, v), lb, (cot[1], cot[2]))
    _, (_, _, want) = ref.with_grads(ref.dense, rows, cols, vals, N, M, la, lb.detach(), 3, (cot[0] * 0, cot[1], cot[2]))
    _close(dlb, want, GRAD_TOL, "dlog_b")
    assert not any(t.requires_grad for t in sparse_sinkhorn(S, la, lb.detach(), 3))


def test_refusals():
    rows, cols, vals, la, lb, _ = _problem(19)
    S, _ = _sparse("csr", rows, cols, vals)
    with pytest.raises(NotImplementedError, match=r"sparse_sinkhorn supports 2-D or batched 3-D sparse tensors, got ndim=4"):
        sparse_sinkhorn(torch.zeros(1, 1, 2, 2).to_sparse(), None, None)
    with pytest.raises(NotImplementedError, match=r"sparse_sinkhorn does not support layout torch.strided"):
        sparse_sinkhorn(torch.zeros(3, 3))
    with pytest.raises(ValueError, match=r"sparse_sinkhorn requires a sparse tensor with zero dense dimensions"):
        sparse_sinkhorn(torch.zeros(3, 3, 2).to_sparse(2))
    with pytest.raises(TypeError, match=r"values must be float32, float64 or bfloat16, got torch.float16"):
        sparse_sinkhorn(_sparse("csr", rows, cols, vals.half())[0])
    with pytest.raises(ValueError, match=r"n_iters must be at least 1, got 0"):
        sparse_sinkhorn(S, la, lb, 0)
    with pytest.raises(TypeError, match=r"n_iters must be an int"):
        sparse_sinkhorn(S, la, lb, 2.0)
    with pytest.raises(ValueError, match=r"log_a must have shape \(37,\) for S of shape \(37, 53\), got \(53,\)"):
        sparse_sinkhorn(S, lb, lb)
    with pytest.raises(ValueError, match=r"log_b must have shape \(53,\)"):
        sparse_sinkhorn(S, la, lb[None])
    with pytest.raises(TypeError, match=r"log_b must have dtype torch.float64 for torch.float64 values, got torch.float32"):
        sparse_sinkhorn(S, la, lb.float())
    with pytest.raises(TypeError, match=r"log_a must be a dense tensor or None"):
        sparse_sinkhorn(S, S, lb)
    batched = torch.sparse_coo_tensor(torch.zeros(3, 1, dtype=torch.int64), torch.ones(1, dtype=F64), (2, N, M))
    with pytest.raises(ValueError, match=r"log_a must have shape \(2, 37\)"):
        sparse_sinkhorn(batched, la, None)


# ---- the staged header ----------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_SINKHORN == {"tsgu_hip_sinkhorn.h": _backend.SIGNATURES_SINKHORN}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR, _backend.STAGED_QUADRATURE,
              _backend.STAGED_CIQ, _backend.STAGED_EXPM, _backend.STAGED_TOPK, _backend.STAGED_SEMI)
    assert len(others) + 1 == 11, "the eleven registries"
    assert not any(set(_backend.STAGED_SINKHORN) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_SINKHORN)
    assert not any(names & set(table) for reg in others for table in reg.values())
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_sinkhorn.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_SINKHORN)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_SINKHORN[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
        if name != "tsgu_sinkhorn_workspace":
            assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION
    src = os.path.join(os.path.dirname(STAGED_HEADER), "sinkhorn.hip")
    assert os.path.exists(src) and '#include "tsgu_hip_sinkhorn.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"


def test_host_refusals_of_the_entries():
    """Fake pointers and device = -1: the refusals come before anything is dereferenced or launched."""
    lib = _backend.load_library()
    p = 4096
    out = ctypes.c_int64(0)
    assert lib.tsgu_sinkhorn_workspace(_backend.TSGU_F32, 5000, ctypes.byref(out)) == A.OK
    assert out.value == 3 * (4 * 4 + 8), "three ranges of 2048 entries: four accumulator words and one tail group each"
    assert lib.tsgu_sinkhorn_workspace(7, 10, ctypes.byref(out)) == A.BAD_DTYPE
    assert lib.tsgu_sinkhorn_workspace(_backend.TSGU_F32, -1, ctypes.byref(out)) == A.BAD_ARG
    half = lambda vt=0, it=0, n=4, nnz=8, ptr=p, out_=p, ws=None, wsb=0, dev=-1: lib.tsgu_sinkhorn_half(   # noqa: E731
        vt, it, n, nnz, ptr, None, p, p, p, None, out_, ws, wsb, dev, None)
    assert half(vt=9) == A.BAD_DTYPE and half(it=5) == A.BAD_DTYPE
    assert half(n=-1) == A.BAD_ARG and half(nnz=-1) == A.BAD_ARG and half(ptr=None) == A.BAD_ARG and half(out_=None) == A.BAD_ARG
    assert half(ws=p + 1, wsb=1 << 20) == A.BAD_ARG and half(ws=p, wsb=8) == A.BAD_ARG and half(ws=None, wsb=64) == A.BAD_ARG
    assert half(n=0) == A.OK, "no groups: nothing to do"
    assert half() == A.BAD_ARG, "device -1 is refused after the operands passed"
    assert lib.tsgu_sinkhorn_plan(0, 0, 4, 0, None, None, None, None, None, None, -1, None) == A.OK
    assert lib.tsgu_sinkhorn_plan(0, 0, 4, 8, p, p, None, p, p, p, -1, None) == A.BAD_ARG
    assert lib.tsgu_sinkhorn_half_backward(0, 0, 4, 8, p, None, p, None, p, p, p, None, p, p, p, 0, None, 0, -1, None) == A.BAD_ARG
    assert lib.tsgu_segment_sum(2, 0, 4, 8, p, None, None, None, p, None, 0, -1, None) == A.BAD_ARG
    assert lib.tsgu_segment_sum(0, 0, 0, 8, None, None, None, None, None, None, 0, -1, None) == A.OK
