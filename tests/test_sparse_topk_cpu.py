"""sparse_topk_mm without a GPU: the torch-op path against the numpy restatement (tests/_topk_ref.py), the gradients against
`torch.autograd.gradcheck` and the dense `topk` composition, every refusal, the staged header csrc/tsgu_hip_topk.h against its ctypes
table and the library, and the host refusals of the launcher (fake pointers, device = -1: nothing is dereferenced).

The exact cases hold integers in [−3, 3] (every product and sum is exact in float32, float64 and bfloat16's float32 accumulator), so
crow, col and the values must be EQUAL to the restatement's; a bfloat16 value is the exact score rounded once."""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _topk_ref as tr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_topk_mm
from torchsparsegradutils_amd.sparse_topk import nnz_of, row_counts

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_topk.h")
ENTRIES = ("tsgu_topk_geometry", "tsgu_topk_mm")
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
F64 = torch.float64


def _ints(rng, shape):
    return rng.integers(-3, 4, shape).astype(np.float64)


def _t(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _check(Q, K, k, dtype, index_dtype=torch.int32, key_bias=None, scale=1.0, **flags):
    """The CPU path for one 2-D case against the restatement: equality of crow, col and values, and the structure."""
    n, m = Q.shape[0], K.shape[0]
    out = sparse_topk_mm(_t(Q, dtype), _t(K, dtype), k, key_bias=_t(key_bias, dtype), scale=scale, index_dtype=index_dtype, **flags)
    assert out.layout == torch.sparse_csr and out.dtype == dtype and tuple(out.shape) == (n, m)
    assert out.crow_indices().dtype == index_dtype == out.col_indices().dtype
    ok = tr.allowed(n, m, **flags)
    S = tr.scores(Q, K, scale, key_bias)
    crow, col, val = tr.select(S, k, ok)
    assert np.array_equal(crow, tr.crow(n, m, k, **flags)), "the restatement's own crow is the closed form"
    assert np.array_equal(out.crow_indices().numpy(), crow)
    assert np.array_equal(out.col_indices().numpy(), col)
    assert np.array_equal(out.values().double().numpy(), _t(val, dtype).double().numpy(), equal_nan=True)
    for i in range(n):
        c = col[crow[i]:crow[i + 1]]
        assert np.all(np.diff(c) > 0) and np.all(ok[i, c]), "ascending, unique, allowed"
    return out


# ---- the torch-op path ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_cpu_path_matches_the_restatement(dtype, index_dtype):
    rng = np.random.default_rng(0)
    Q, K = _ints(rng, (70, 40)), _ints(rng, (333, 40))
    S = tr.scores(Q, K)
    assert tr.boundary_ties(S, 16, tr.allowed(70, 333)).sum() * 4 >= 70, "ties across the k-th boundary: the lower column decides"
    _check(Q, K, 16, dtype, index_dtype)
    _check(Q, K, 16, dtype, index_dtype, key_bias=_ints(rng, 333))
    _check(Q, K, 1, dtype, index_dtype)
    _check(Q[:9], K[:12], 20, dtype, index_dtype)                                     # m < k
    _check(Q[:9], K[:12], 20, dtype, index_dtype, exclude_self=True)
    for n, m in ((9, 30), (21, 21), (30, 9)):                                         # n < m, n = m, n > m: empty leading rows
        for flags in (dict(causal=True), dict(exclude_self=True), dict(causal=True, exclude_self=True)):
            out = _check(Q[:n], K[:m], 4, dtype, index_dtype, key_bias=_ints(rng, m), **flags)
        if n > m:
            assert int(out.crow_indices()[n - m]) == 0
    _check(_ints(rng, (0, 5)), K[:7, :5], 3, dtype, index_dtype)                        # n = 0
    empty = _check(Q[:6, :5], _ints(rng, (0, 5)), 3, dtype, index_dtype)               # m = 0
    assert empty.values().numel() == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_special_values(dtype):
    rng = np.random.default_rng(1)
    Q, K = _ints(rng, (11, 6)), _ints(rng, (40, 6))
    bias = np.full(40, -np.inf)
    bias[[3, 17, 29]] = 0.0
    out = _check(Q, K, 5, dtype, key_bias=bias)                                        # -inf only where finite scores run out
    assert out.col_indices()[:5].tolist() == [0, 1, 3, 17, 29]
    Kn = K.copy()
    Kn[20] = np.nan
    bias = np.zeros(40)
    bias[[5, 33]] = np.inf
    for k in (1, 2, 5):
        out = _check(Q, Kn, k, dtype, key_bias=bias)                                   # NaN first, +inf next, the lower column first
        rows = out.col_indices().reshape(11, k)
        assert bool((rows == 20).any(1).all()) and (k < 2 or bool((rows == 5).any(1).all()))
    assert sparse_topk_mm(_t(np.zeros((2, 3)), dtype), _t(-np.zeros((4, 3)), dtype), 2).col_indices().tolist() == [0, 1, 0, 1], "-0 = +0"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batched(dtype):
    rng = np.random.default_rng(2)
    Q, K, bias = _ints(rng, (3, 9, 5)), _ints(rng, (3, 14, 5)), _ints(rng, (3, 14))
    for index_dtype in (torch.int32, torch.int64):
        out = sparse_topk_mm(_t(Q, dtype), _t(K, dtype), 4, key_bias=_t(bias, dtype), causal=True, index_dtype=index_dtype)
        assert tuple(out.shape) == (3, 9, 14) and out.crow_indices().shape == (3, 10) and out.col_indices().dtype == index_dtype
        for i in range(3):
            crow, col, val = tr.select(tr.scores(Q[i], K[i], 1.0, bias[i]), 4, tr.allowed(9, 14, causal=True))
            assert np.array_equal(out.crow_indices()[i].numpy(), crow) and np.array_equal(out.col_indices()[i].numpy(), col)
            assert np.array_equal(out.values()[i].double().numpy(), _t(val, dtype).double().numpy())
    assert not torch.equal(out.col_indices()[0], out.col_indices()[1])


def test_row_counts_are_the_closed_form():
    for n, m, k in ((5, 9, 3), (9, 5, 3), (7, 7, 7), (4, 6, 9), (0, 3, 2), (3, 0, 2)):
        for causal in (False, True):
            for exclude_self in (False, True):
                want = np.diff(tr.crow(n, m, k, causal, exclude_self))
                assert np.array_equal(row_counts(n, m, k, causal, exclude_self).numpy(), want)
                assert np.array_equal(want, np.minimum(tr.allowed(n, m, causal, exclude_self).sum(1), k))


def test_nnz_in_integer_arithmetic_is_the_sum_of_the_row_counts():
    for n in range(0, 8):
        for m in range(0, 8):
            for k in (1, 2, 3, 5, 9):
                for causal in (False, True):
                    for exclude_self in (False, True):
                        want = int(np.minimum(tr.allowed(n, m, causal, exclude_self).sum(1), k).sum())
                        assert nnz_of(n, m, k, causal, exclude_self) == want, (n, m, k, causal, exclude_self)
    assert nnz_of(70000, 70000, 128, False, True) == 70000 * 128 and nnz_of(1 << 20, 1 << 20, 4096, True, False) >= 2 ** 31


def test_scale_and_the_knn_recipe():
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(50, 6, generator=gen, dtype=F64)
    graph = sparse_topk_mm(X, X, 5, key_bias=-0.5 * (X * X).sum(-1), exclude_self=True)
    dist = torch.cdist(X, X)
    dist.fill_diagonal_(float("inf"))
    want = dist.topk(5, largest=False).indices.sort(1).values
    assert torch.equal(graph.col_indices().reshape(50, 5).long(), want)
    lowest = sparse_topk_mm(X, X, 3, scale=-1.0)                                      # smallest: negate scale
    assert torch.equal(lowest.col_indices().reshape(50, 3).long(), (X @ X.t()).topk(3, largest=False).indices.sort(1).values)


# ---- gradients ------------------------------------------------------------------------------------------------------------------------

def _grad_operands(batched=False):
    gen = torch.Generator().manual_seed(4)
    lead = (2,) if batched else ()
    Q, K, b = (torch.randn(lead + s, generator=gen, dtype=F64) for s in ((6, 4), (9, 4), (9,)))
    return Q, K, b


@pytest.mark.parametrize("batched", [False, True], ids=["2d", "batched"])
def test_gradcheck(batched):
    Q, K, b = (x.requires_grad_(True) for x in _grad_operands(batched))
    S = 0.7 * Q.detach() @ K.detach().transpose(-1, -2) + b.detach().unsqueeze(-2)
    gaps = S.sort(-1).values.diff(dim=-1).abs().min()
    # gradcheck moves one operand entry by 1e-6, a score by less than 1e-5: the selection is constant around the point
    assert float(gaps) > 1e-4, "no ties near the evaluation point"

    def values(q, k, kb):
        return sparse_topk_mm(q, k, 3, scale=0.7, key_bias=kb, causal=True).values()

    assert torch.autograd.gradcheck(values, (Q, K, b), eps=1e-6, atol=1e-8)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gradients_equal_the_dense_topk_composition(dtype):
    Q, K, b = (x.to(dtype).requires_grad_(True) for x in _grad_operands())
    out = sparse_topk_mm(Q, K, 3, scale=0.5, key_bias=b)
    gen = torch.Generator().manual_seed(5)
    W = torch.randn(6, 9, generator=gen, dtype=F64).to(dtype)
    got = torch.autograd.grad(out, (Q, K, b), W)                                       # a dense cotangent is gathered on the pattern
    Qd, Kd, bd = (x.detach().double().requires_grad_(True) for x in (Q, K, b))
    S = 0.5 * Qd @ Kd.t() + bd
    val, idx = S.topk(3, dim=1)
    want = torch.autograd.grad(val, (Qd, Kd, bd), W.double().gather(1, idx))
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else float(torch.finfo(dtype).eps)
    for g, w in zip(got, want):
        assert g.dtype == dtype and g.shape == w.shape
        assert float((g.double() - w).abs().max()) <= 16 * eps * float(w.abs().max()), "a handful of roundings of sums of 3 to 6 terms"
    sparse_cot = torch.sparse_csr_tensor(out.crow_indices(), out.col_indices(), W.gather(1, out.col_indices().reshape(6, 3).long()).reshape(-1),
                                         out.shape)
    again = torch.autograd.grad(sparse_topk_mm(Q, K, 3, scale=0.5, key_bias=b), (Q, K, b), sparse_cot)
    assert all(torch.equal(x, y) for x, y in zip(got, again)), "a cotangent on the result's own pattern gives the same gradients"
    only_q = torch.autograd.grad(sparse_topk_mm(Q, K.detach(), 3), Q, W)[0]
    assert only_q.shape == Q.shape


def test_double_backward_raises():
    Q, K, _ = (x.requires_grad_(True) for x in _grad_operands())
    out = sparse_topk_mm(Q, K, 3)
    (gq,) = torch.autograd.grad((out.values() ** 2).sum(), Q, create_graph=True)      # a cotangent that depends on the operands
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gq.sum().backward()
    (gq,) = torch.autograd.grad(sparse_topk_mm(Q, K, 3), Q, torch.ones(6, 9, dtype=F64), create_graph=True)      # ... and a constant one
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gq.sum().backward()


# ---- the surface ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    Q, K = torch.randn(5, 4), torch.randn(7, 4)

    def fails(kind, text, *args, **kw):
        with pytest.raises(kind, match=text):
            sparse_topk_mm(*args, **kw)

    fails(TypeError, "sparse_topk_mm: Q must be a dense tensor", Q.to_sparse(), K, 2)
    fails(TypeError, "sparse_topk_mm: K must be a dense tensor", Q, K.to_sparse_csr(), 2)
    fails(TypeError, "sparse_topk_mm: key_bias must be a dense tensor", Q, K, 2, key_bias=torch.randn(7).to_sparse())
    fails(TypeError, "sparse_topk_mm: Q must be a dense tensor", Q.numpy(), K, 2)
    fails(TypeError, "one dtype, got torch.float32 and torch.float64", Q, K.double(), 2)
    fails(TypeError, "one dtype, got torch.float32 and torch.bfloat16", Q, K, 2, key_bias=torch.randn(7).bfloat16())
    fails(TypeError, "float32, float64 or bfloat16, got torch.float16", Q.half(), K.half(), 2)
    fails(ValueError, r"Q must be \[n, d\] or \[b, n, d\]", Q[0], K, 2)
    fails(ValueError, r"K must be \[m, d\] with Q's d", Q, torch.randn(7, 3), 2)
    fails(ValueError, r"K must be \[b, m, d\] with Q's d and b", Q[None], K, 2)
    fails(ValueError, r"K must be \[b, m, d\] with Q's d and b", Q[None], K[None].expand(2, -1, -1), 2)
    fails(ValueError, "at least one column", torch.randn(5, 0), torch.randn(7, 0), 2)
    fails(ValueError, r"key_bias must be \(7,\)", Q, K, 2, key_bias=torch.randn(5))
    fails(ValueError, r"key_bias must be \(1, 7\)", Q[None], K[None], 2, key_bias=torch.randn(7))
    for k in (0, -1, 2.0, True):
        fails(ValueError, "k must be an integer of at least 1", Q, K, k)
    for scale in (float("inf"), float("nan"), "1", None, True):
        fails(ValueError, "scale must be a finite number", Q, K, 2, scale=scale)
    fails(ValueError, "index_dtype must be torch.int32 or torch.int64", Q, K, 2, index_dtype=torch.int16)
    assert "sparse_topk_mm" in tsgu.__all__ and tsgu.sparse_topk_mm is sparse_topk_mm and "sparse_topk_mm" in tsgu.__doc__
    assert "fold the heads into the batch" in sparse_topk_mm.__doc__ and "exclude_self=True" in sparse_topk_mm.__doc__


def test_int32_is_refused_when_the_result_does_not_fit(monkeypatch):
    from torchsparsegradutils_amd import sparse_topk as st

    monkeypatch.setattr(st, "_row_pointer", lambda n, m, k, c, e, idt, dev: (torch.zeros(n + 1, dtype=idt), 2 ** 31))
    with pytest.raises(ValueError, match=r"sparse_topk_mm: the result has 2147483648 stored entries per matrix, which needs index_dtype=torch.int64"):
        sparse_topk_mm(torch.randn(3, 2), torch.randn(4, 2), 2)


def test_the_cap_on_k_is_named_for_gpu_operands(monkeypatch):
    """The refusal is decided before any kernel runs: a tensor that only claims to live on the GPU reaches it."""
    cap = _backend.topk_geometry(torch.float32)[0]
    assert cap >= 128 and all(_backend.topk_geometry(dt)[0] == cap for dt in DTYPES)

    class OnGpu(torch.Tensor):
        is_cuda = True

    Q, K = torch.randn(4, 3).as_subclass(OnGpu), torch.randn(6, 3).as_subclass(OnGpu)
    with pytest.raises(ValueError, match=rf"sparse_topk_mm: the gfx950 kernels select at most k = {cap} entries per row, got k = {cap + 1}"):
        sparse_topk_mm(Q, K, cap + 1)


# ---- the staged header ----------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_TOPK == {"tsgu_hip_topk.h": _backend.SIGNATURES_TOPK}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR, _backend.STAGED_QUADRATURE,
              _backend.STAGED_CIQ, _backend.STAGED_EXPM)
    assert len(others) + 1 == 9, "the nine registries"
    assert not any(set(_backend.STAGED_TOPK) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_TOPK)
    assert not any(names & set(table) for reg in others for table in reg.values())
    every = [name for reg in others for table in reg.values() for name in table]
    assert len(every) == len(set(every)), "the registries are disjoint"
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_topk.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_TOPK)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_TOPK[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    assert protos[1][1][-2:] == [("device", "int"), ("stream", "void*")]
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION
    src = os.path.join(os.path.dirname(STAGED_HEADER), "topk.hip")
    assert os.path.exists(src) and '#include "tsgu_hip_topk.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"
    assert (_backend.TOPK_CAUSAL, _backend.TOPK_EXCLUDE_SELF) == (1, 2)
    assert "#define TSGU_TOPK_CAUSAL 1" in text and "#define TSGU_TOPK_EXCLUDE_SELF 2" in text


def test_geometry():
    for dtype, kc in ((torch.float32, 64), (F64, 32), (torch.bfloat16, 128)):
        cap, rows, keys, stage, lds = _backend.topk_geometry(dtype, 64, 128)
        assert cap >= 128 and rows % 16 == 0 and keys % 16 == 0 and stage == kc
        assert 0 < lds <= 80 * 1024, "two workgroups per CU at the largest k: half of the CU's 160 KiB"
        assert _backend.topk_geometry(dtype, 1, 1)[4] < lds
        with pytest.raises(RuntimeError, match="tsgu_topk_geometry"):
            _backend.topk_geometry(dtype, 64, cap + 1)
    lib = _backend.load_library()
    slots = [ctypes.c_int() for _ in range(5)]
    refs = [ctypes.byref(x) for x in slots]
    assert lib.tsgu_topk_geometry(0, 8, 4, *refs) == A.OK and lib.tsgu_topk_geometry(2, 8, 4, *refs) == A.OK
    assert lib.tsgu_topk_geometry(3, 8, 4, *refs) == A.BAD_DTYPE and lib.tsgu_topk_geometry(-1, 8, 4, *refs) == A.BAD_DTYPE
    assert lib.tsgu_topk_geometry(0, 0, 4, *refs) == A.BAD_ARG and lib.tsgu_topk_geometry(0, 8, 0, *refs) == A.BAD_ARG
    assert lib.tsgu_topk_geometry(0, 8, slots[0].value + 1, *refs) == A.TOO_LARGE and slots[0].value >= 128
    for k in range(5):
        assert lib.tsgu_topk_geometry(0, 8, 4, *(None if j == k else r for j, r in enumerate(refs))) == A.BAD_ARG


# ---- host refusals: every call below is refused before the device is touched (the base call only by set_device(-1)) ------------------

BASE = dict(vtype=0, Q=0x10000, K=0x20000, key_bias=0x30000, n=100, m=200, d=24, k=8, scale=0.5, flags=3, causal_offset=100, crow=0x40000,
            col=0x50000, val=0x60000, itype=0, batch=2, q_stride=2400, k_stride=4800, bias_stride=200, out_stride=800)


def _call(**changes):
    a = dict(BASE)
    a.update(changes)
    return _backend.load_library().tsgu_topk_mm(*a.values(), -1, None)


def test_host_refusals():
    params = dict(A.prototypes(STAGED_HEADER))["tsgu_topk_mm"]
    assert [q[0] for q in params[:-2]] == list(BASE), "the base call names the header's parameters"
    cap = _backend.topk_geometry(torch.float32)[0]
    assert _call() == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    assert _call(key_bias=None) == A.BAD_ARG, "a NULL key_bias reaches set_device as well"
    for pn in ("Q", "K", "crow", "col", "val"):
        assert _call(**{pn: None}) == A.BAD_ARG, pn
    assert _call(vtype=3) == A.BAD_DTYPE and _call(vtype=-1) == A.BAD_DTYPE and _call(itype=2) == A.BAD_DTYPE
    for ch in (dict(n=-1), dict(m=-1), dict(d=0), dict(k=0), dict(batch=-1), dict(flags=4), dict(flags=-1), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(q_stride=-1), dict(k_stride=-1), dict(bias_stride=-1), dict(out_stride=-1)):
        assert _call(**ch) == A.BAD_ARG, ch
    for pn in ("Q", "K", "key_bias", "val", "crow", "col"):
        assert _call(**{pn: BASE[pn] + 2}) == A.BAD_ARG, f"{pn}: element alignment (float32 / int32)"
        assert _call(vtype=2, **{pn: BASE[pn] + 1}) == A.BAD_ARG
    assert _call(vtype=2, Q=BASE["Q"] + 2) == A.BAD_ARG == _call(vtype=1, itype=1, Q=BASE["Q"] + 8), "an aligned pointer goes on to set_device"
    assert _call(vtype=1, Q=BASE["Q"] + 4) == A.BAD_ARG and _call(itype=1, col=BASE["col"] + 4) == A.BAD_ARG
    assert _call(k=cap + 1) == A.TOO_LARGE
    assert _call(n=2 ** 31 - 1) == A.TOO_LARGE and _call(m=2 ** 31 - 1) == A.TOO_LARGE
    assert _call(n=2 ** 31 - 2, batch=1 << 20) == A.TOO_LARGE, "more workgroups than a grid holds"
