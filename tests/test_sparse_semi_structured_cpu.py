"""The 2:4 semi-structured operand without a GPU: prune, indices and to_dense of the torch-op path against the numpy restatement
(tests/_semi_ref.py), the gradients against `torch.autograd.gradcheck`, every refusal, the staged header csrc/tsgu_hip_semi.h against
its ctypes table and the library, and the host refusals of the launchers (fake pointers, device = -1: nothing is dereferenced)."""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _semi_ref as sr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import (SemiStructured, _backend, sparse_semi_structured_linear, sparse_semi_structured_mm,
                                      sparse_semi_structured_prune)

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_semi.h")
ENTRIES = ("tsgu_semi_geometry", "tsgu_semi_prune", "tsgu_semi_expand", "tsgu_semi_mm", "tsgu_semi_mm_t", "tsgu_semi_sddmm")
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
F64 = torch.float64
NAN, INF = float("nan"), float("inf")

# groups of four: ties, signed zeros, NaN and inf, 0 .. 4 non-zeros
GROUPS = [
    [0, 0, 0, 0], [0, 0, 0, 5], [0, 3, 0, 0], [1, 0, 0, 2], [0, 1, 2, 0], [1, 2, 3, 0], [0, 3, 2, 1], [4, 3, 2, 1], [1, 2, 3, 4],
    [1, 1, 1, 1], [-1, 1, -1, 1], [2, -2, 1, 2], [1, 2, 2, 2], [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 1, -0.0], [-0.0, -0.0, -0.0, -1],
    [NAN, 1, 2, 3], [1, INF, NAN, 2], [INF, -INF, NAN, NAN], [NAN, NAN, NAN, NAN], [-INF, 1, INF, 7], [INF, INF, -INF, INF],
    [1, NAN, INF, -INF], [0, NAN, 0, 0], [-3, 3, -3, 3], [0.5, -0.25, 0.25, -0.5],
]


def _special(dtype):
    rows = [sum((GROUPS[(i + j) % len(GROUPS)] for j in range(len(GROUPS))), []) for i in range(3)]
    return torch.tensor(rows, dtype=F64).to(dtype)


def _same(a, b):
    """Equal including NaN places and the signs of zeros."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_prune_matches_the_restatement(dtype):
    rng = np.random.default_rng(0)
    for W in (_special(dtype), torch.from_numpy(rng.integers(-2, 3, (7, 132)).astype(np.float64)).to(dtype),
              torch.from_numpy(rng.standard_normal((5, 260))).to(dtype), torch.zeros((2, 4), dtype=dtype), torch.zeros((0, 8), dtype=dtype),
              torch.zeros((3, 0), dtype=dtype)):
        S = sparse_semi_structured_prune(W)
        values, cols = sr.prune(W.double().numpy())
        m, k = W.shape
        assert S.shape == (m, k) and S.dtype == dtype and S.device == W.device
        assert S.values.shape == (m, k // 2) and S.meta.dtype == torch.int32 and S.meta.shape == (m, 4 * ((k + 127) // 128))
        assert S.indices().dtype == torch.int64 and np.array_equal(S.indices().numpy(), cols)
        assert _same(S.values.double().numpy(), values)
        assert _same(S.to_dense().double().numpy(), sr.to_dense(values, cols, k))
        if k:
            idx = S.indices().reshape(m, k // 4, 2)
            assert bool((idx[..., 0] < idx[..., 1]).all()) and bool((idx // 4 == torch.arange(k // 4)[None, :, None]).all())


def test_group_rules():
    S = sparse_semi_structured_prune(torch.tensor([[0., 0, 0, 5, 1, 1, 1, 1, NAN, INF, 9, -INF, -0.0, 0.0, 2, -0.0]]))
    assert S.indices().tolist() == [[0, 3, 4, 5, 8, 9, 12, 14]]
    assert _same(S.values.numpy(), [[0, 5, 1, 1, NAN, INF, -0.0, 2]])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_2_4_matrix_round_trips_bit_for_bit(dtype):
    rng = np.random.default_rng(1)
    m, k = 9, 136
    W = rng.standard_normal((m, k))
    keep = np.zeros((m, k // 4, 4), dtype=bool)
    for i in range(m):
        for g in range(k // 4):
            keep[i, g, rng.choice(4, size=rng.integers(0, 3), replace=False)] = True       # 0, 1 or 2 non-zeros
    W = torch.from_numpy(np.where(keep.reshape(m, k), W, 0.0)).to(dtype)
    W[0, 0:4] = torch.tensor([-0.0, 0.0, -1.0, 0.0], dtype=F64).to(dtype)
    S = SemiStructured.from_dense(W)
    bits = {torch.bfloat16: torch.int16, torch.float32: torch.int32, F64: torch.int64}[dtype]
    assert torch.equal(S.to_dense().view(bits), W.view(bits)), "the kept -0 keeps its sign, every dropped position was +0"
    again = SemiStructured.from_dense(S.to_dense())
    assert torch.equal(again.indices(), S.indices()) and _same(again.values.double().numpy(), S.values.double().numpy())
    assert _same(again.to_dense().double().numpy(), S.to_dense().double().numpy())


def test_from_dense_refuses_a_dropped_non_zero():
    W = torch.zeros(3, 8)
    W[1, 4:7] = torch.tensor([1.0, -2.0, 3.0])
    with pytest.raises(ValueError, match="SemiStructured.from_dense: the matrix is not 2:4 sparse"):
        SemiStructured.from_dense(W)
    W[1, 4] = 0
    assert SemiStructured.from_dense(W).indices()[1].tolist() == [0, 1, 5, 6]


def test_with_values_keeps_the_pattern():
    S = sparse_semi_structured_prune(torch.randn(4, 16))
    T = S.with_values(torch.ones(4, 8))
    assert T.meta is S.meta and T.shape == S.shape and torch.equal(T.to_dense(), (S.to_dense() != 0).float())
    with pytest.raises(ValueError, match=r"SemiStructured: values must be \(4, 8\) for shape \(4, 16\), got \(4, 7\)"):
        S.with_values(torch.ones(4, 7))


# ---- products and gradients ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_products_match_the_restatement_on_integers(dtype):
    """Integers in [-3, 3]: every product and sum is exact in all three accumulators, so the results are EQUAL."""
    rng = np.random.default_rng(2)
    m, k, p = 7, 36, 5
    W, B, G = (torch.from_numpy(rng.integers(-3, 4, s).astype(np.float64)).to(dtype) for s in ((m, k), (k, p), (m, p)))
    S = sparse_semi_structured_prune(W)
    values, cols = sr.prune(W.double().numpy())
    v = S.values.clone().requires_grad_(True)
    Bq = B.clone().requires_grad_(True)
    out = sparse_semi_structured_mm(S.with_values(v), Bq)
    assert out.dtype == dtype and np.array_equal(out.detach().double().numpy(), sr.mm(values, cols, k, B.double().numpy())[0])
    out.backward(G)
    assert np.array_equal(v.grad.double().numpy(), sr.sddmm(cols, G.double().numpy(), B.double().numpy())[0])
    assert np.array_equal(Bq.grad.double().numpy(), sr.mm_t(values, cols, k, G.double().numpy())[0])
    X = B.t().contiguous().reshape(1, p, k).clone().requires_grad_(True)
    bias = torch.arange(m, dtype=F64).to(dtype).requires_grad_(True)
    v2 = S.values.clone().requires_grad_(True)
    lin = sparse_semi_structured_linear(X, S.with_values(v2), bias)
    assert lin.shape == (1, p, m) and np.array_equal(lin.detach().double().numpy()[0], out.detach().double().numpy().T + np.arange(m)[None, :])
    lin.backward(G.t().contiguous().reshape(1, p, m))
    assert torch.equal(v2.grad, v.grad) and torch.equal(X.grad[0], Bq.grad.t()) and torch.equal(bias.grad, G.sum(1))


def test_gradcheck_mm():
    torch.manual_seed(0)
    S = sparse_semi_structured_prune(torch.randn(6, 12, dtype=F64))
    v, B = S.values.clone().requires_grad_(True), torch.randn(12, 5, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v, B: sparse_semi_structured_mm(S.with_values(v), B), (v, B))


def test_gradcheck_linear_with_bias_and_leading_dimensions():
    torch.manual_seed(1)
    S = sparse_semi_structured_prune(torch.randn(5, 8, dtype=F64))
    v = S.values.clone().requires_grad_(True)
    X, bias = torch.randn(2, 3, 8, dtype=F64, requires_grad=True), torch.randn(5, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda X, v, b: sparse_semi_structured_linear(X, S.with_values(v), b), (X, v, bias))
    assert torch.autograd.gradcheck(lambda X, v: sparse_semi_structured_linear(X, S.with_values(v)), (X, v))
    out = sparse_semi_structured_linear(X, S, bias)
    assert out.shape == (2, 3, 5) and torch.allclose(out, torch.nn.functional.linear(X, S.to_dense(), bias))


def test_gradcheck_prune_and_to_dense():
    torch.manual_seed(2)
    W = torch.randn(4, 12, dtype=F64, requires_grad=True)                 # distinct magnitudes: the selection is locally constant
    assert torch.autograd.gradcheck(lambda W: sparse_semi_structured_prune(W).values, (W,))
    assert torch.autograd.gradcheck(lambda W: sparse_semi_structured_prune(W).to_dense(), (W,))
    S = sparse_semi_structured_prune(W)
    Gv = torch.randn(4, 6, dtype=F64)
    (gW,) = torch.autograd.grad(S.values, W, Gv)
    assert torch.equal(gW, S.with_values(Gv).to_dense().detach()) and int((gW != 0).sum()) == 24
    # the whole chain of a pruned layer: W -> prune -> linear
    X = torch.randn(3, 12, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda W, X: sparse_semi_structured_linear(X, sparse_semi_structured_prune(W)), (W, X))


def test_a_second_differentiation_raises():
    W = torch.randn(4, 8, dtype=F64, requires_grad=True)
    B = torch.randn(8, 3, dtype=F64, requires_grad=True)
    S = sparse_semi_structured_prune(W)
    for out, wrt in ((sparse_semi_structured_mm(S, B), B), (sparse_semi_structured_linear(B.t(), S), B), (S.values, W), (S.to_dense(), W)):
        (g,) = torch.autograd.grad(out.sum(), wrt, create_graph=True, retain_graph=True)
        with pytest.raises(RuntimeError, match="differentiate twice"):
            g.sum().backward()


# ---- the surface ----------------------------------------------------------------------------------------------------------------------

def test_refusals():
    W = torch.randn(6, 8)
    S = sparse_semi_structured_prune(W)

    def fails(text, fn, *args, **kw):
        with pytest.raises(ValueError, match=text):
            fn(*args, **kw)

    prune, mm, lin = sparse_semi_structured_prune, sparse_semi_structured_mm, sparse_semi_structured_linear
    fails(r"sparse_semi_structured_prune: W must be a 2-D matrix \(m, k\), got \(2, 6, 8\)", prune, torch.randn(2, 6, 8))
    fails(r"sparse_semi_structured_prune: W must be a 2-D matrix \(m, k\), got \(8,\)", prune, torch.randn(8))
    fails("sparse_semi_structured_prune: k must be a multiple of 4, got k = 6", prune, torch.randn(3, 6))
    fails("sparse_semi_structured_prune: W must be float32, float64 or bfloat16, got torch.int64", prune, torch.ones(3, 8, dtype=torch.int64))
    fails("sparse_semi_structured_prune: W must be float32, float64 or bfloat16, got torch.float16", prune, torch.ones(3, 8).half())
    fails("sparse_semi_structured_prune: W must be a dense tensor", prune, W.to_sparse())
    fails("SemiStructured.from_dense: the matrix is not 2:4 sparse", SemiStructured.from_dense, torch.ones(1, 4))
    fails("SemiStructured: k must be a multiple of 4, got k = 6", SemiStructured, torch.randn(6, 3), S.meta, (6, 6))
    fails(r"SemiStructured: the shape must be \(m, k\), got \(2, 6, 8\)", SemiStructured, S.values, S.meta, (2, 6, 8))
    fails("SemiStructured: values must be float32, float64 or bfloat16, got torch.int32", SemiStructured, S.values.int(), S.meta, (6, 8))
    fails(r"SemiStructured: meta must be a contiguous int32 tensor of shape \(6, 4\)", SemiStructured, S.values, S.meta.long(), (6, 8))
    fails(r"SemiStructured: meta must be a contiguous int32 tensor of shape \(6, 4\)", SemiStructured, S.values, S.meta[:, :3], (6, 8))
    fails("SemiStructured: values and meta must be on one device", SemiStructured, S.values, S.meta.to("meta"), (6, 8))
    fails("sparse_semi_structured_mm: A must be a SemiStructured matrix, got Tensor", mm, W, torch.randn(8, 3))
    fails(r"sparse_semi_structured_mm: B must be \(k, p\) with k = 8, got \(6, 3\)", mm, S, torch.randn(6, 3))
    fails(r"sparse_semi_structured_mm: B must be \(k, p\) with k = 8, got \(8,\)", mm, S, torch.randn(8))
    fails("sparse_semi_structured_mm: A and B must have one dtype, got torch.float32 and torch.float64", mm, S, torch.randn(8, 3).double())
    fails("sparse_semi_structured_mm: B must be float32, float64 or bfloat16, got torch.int64", mm, S, torch.ones(8, 3, dtype=torch.int64))
    fails("sparse_semi_structured_mm: B must be a dense tensor", mm, S, torch.randn(8, 3).to_sparse())
    fails("sparse_semi_structured_mm: A and B must be on one device, got cpu and meta", mm, S, torch.randn(8, 3, device="meta"))
    fails(r"sparse_semi_structured_linear: X must be \(\.\.\., k\) with k = 8, got \(2, 6\)", lin, torch.randn(2, 6), S)
    fails("sparse_semi_structured_linear: A and X must have one dtype", lin, torch.randn(2, 8).bfloat16(), S)
    fails(r"sparse_semi_structured_linear: bias must be \(6,\), got \(8,\)", lin, torch.randn(2, 8), S, torch.randn(8))
    fails("sparse_semi_structured_linear: A and bias must have one dtype", lin, torch.randn(2, 8), S, torch.randn(6).double())
    fails("sparse_semi_structured_linear: A must be a SemiStructured matrix", lin, torch.randn(2, 8), W)
    names = {"SemiStructured", "sparse_semi_structured_prune", "sparse_semi_structured_mm", "sparse_semi_structured_linear"}
    assert names <= set(tsgu.__all__) and all(n in tsgu.__doc__ for n in names if n != "SemiStructured")
    from torchsparsegradutils_amd.sparse_semi_structured import __all__ as mod_all
    assert set(mod_all) == names
    assert "unspecified" in mm.__doc__ and "never read by the sparse" in mm.__doc__ and "sparse_semi_structured_mm" in lin.__doc__


def test_gpu_kernels_refuse_cpu_tensors():
    S = sparse_semi_structured_prune(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="CPU operands are served by the torch-op path"):
        _backend.semi_prune(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="CPU operands are served by the torch-op path"):
        _backend.semi_mm(S.values, S.meta, 8, torch.randn(8, 2), None, False, True)


# ---- the staged header ----------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_SEMI == {"tsgu_hip_semi.h": _backend.SIGNATURES_SEMI}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG, _backend.STAGED_GMRES, _backend.STAGED_COLOR, _backend.STAGED_QUADRATURE,
              _backend.STAGED_CIQ, _backend.STAGED_EXPM, _backend.STAGED_TOPK)
    assert len(others) + 1 == 10, "the ten registries"
    assert not any(set(_backend.STAGED_SEMI) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_SEMI)
    assert not any(names & set(table) for reg in others for table in reg.values())
    every = [name for reg in others for table in reg.values() for name in table]
    assert len(every) == len(set(every)), "the registries are disjoint"
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_semi.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_SEMI)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_SEMI[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for _, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")]
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION
    src = os.path.join(os.path.dirname(STAGED_HEADER), "semi.hip")
    assert os.path.exists(src) and '#include "tsgu_hip_semi.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"
    assert (_backend.SEMI_DENSE_T, _backend.SEMI_OUT_T) == (1, 2)
    assert "#define TSGU_SEMI_DENSE_T 1" in text and "#define TSGU_SEMI_OUT_T 2" in text


def test_geometry():
    for dtype, kc, sparse in ((torch.float32, 64, 0), (F64, 32, 0), (torch.bfloat16, 128, 1)):
        words, rows, cols, stage, smfmac = _backend.semi_geometry(dtype, 260)
        assert (words, stage, smfmac) == (12, kc, sparse) and rows % 16 == 0 and cols % 16 == 0
        assert _backend.semi_geometry(dtype, 0)[0] == 0 and _backend.semi_geometry(dtype, 128)[0] == 4 == _backend.semi_meta_words(128)
        assert _backend.semi_meta_words(132) == 8 == _backend.semi_geometry(dtype, 132)[0]
        with pytest.raises(RuntimeError, match="tsgu_semi_geometry"):
            _backend.semi_geometry(dtype, 6)
    lib = _backend.load_library()
    slots = [ctypes.c_int64()] + [ctypes.c_int() for _ in range(4)]
    refs = [ctypes.byref(x) for x in slots]
    assert lib.tsgu_semi_geometry(0, 8, *refs) == A.OK and lib.tsgu_semi_geometry(3, 8, *refs) == A.BAD_DTYPE
    assert lib.tsgu_semi_geometry(0, -4, *refs) == A.BAD_ARG and lib.tsgu_semi_geometry(0, 2, *refs) == A.BAD_ARG
    for j in range(5):
        assert lib.tsgu_semi_geometry(0, 8, *(None if i == j else r for i, r in enumerate(refs))) == A.BAD_ARG


# ---- host refusals: every call below is refused before the device is touched (the base calls only by set_device(-1)) ------------------

BASES = {
    "tsgu_semi_prune": dict(vtype=0, W=0x10000, ldw=256, m=100, k=256, val=0x20000, ldv=128, meta=0x30000, ldm=8),
    "tsgu_semi_expand": dict(vtype=0, val=0x20000, ldv=128, meta=0x30000, ldm=8, m=100, k=256, out=0x10000, ldo=256),
    "tsgu_semi_mm": dict(vtype=2, val=0x20000, ldv=128, meta=0x30000, ldm=8, Y=0x40000, ldy=256, bias=0x60000, C=0x50000, ldc=100, m=100,
                         k=256, p=40, flags=2, path=1),
    "tsgu_semi_mm_t": dict(vtype=0, val=0x20000, ldv=128, meta=0x30000, ldm=8, G=0x40000, ldg=40, D=0x50000, ldd=40, m=100, k=256, p=40,
                           flags=0),
    "tsgu_semi_sddmm": dict(vtype=0, G=0x40000, ldg=40, Y=0x50000, ldy=40, meta=0x30000, ldm=8, out=0x20000, ldo=128, m=100, k=256, p=40,
                            flags=0),
}


def _call(name, **changes):
    a = dict(BASES[name])
    a.update(changes)
    return getattr(_backend.load_library(), name)(*a.values(), -1, None)


@pytest.mark.parametrize("name", list(BASES))
def test_host_refusals(name):
    params = dict(A.prototypes(STAGED_HEADER))[name]
    base = BASES[name]
    assert [q[0] for q in params[:-2]] == list(base), "the base call names the header's parameters"
    assert _call(name) == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    for (pn, pt) in params[:-2]:
        if pt.endswith("*") and pn != "bias":
            assert _call(name, **{pn: None}) == A.BAD_ARG, pn
            assert _call(name, **{pn: base[pn] + 2}) == A.BAD_ARG, f"{pn}: element alignment"
    assert _call(name, meta=base["meta"] + 4) == A.BAD_ARG, "the position words are read in 16-byte rows"
    assert _call(name, vtype=3) == A.BAD_DTYPE and _call(name, vtype=-1) == A.BAD_DTYPE
    for ch in (dict(m=-1), dict(k=-4), dict(k=254), dict(k=6), dict(ldm=4), dict(ldm=9), dict(m=2 ** 31 - 1)):
        assert _call(name, **ch) == (A.TOO_LARGE if ch.get("m", 0) > 0 else A.BAD_ARG), ch
    lds = [pn for pn, _ in params if pn.startswith("ld") and pn != "ldm"]
    for pn in lds:
        assert _call(name, **{pn: base[pn] - 1}) == A.BAD_ARG, pn
    if "p" in base:
        assert _call(name, p=-1) == A.BAD_ARG
        big = {pn: 2 ** 31 for pn in ("ldg", "ldy", "ldc", "ldd") if pn in base}
        assert _call(name, p=2 ** 31 - 1, **big) == A.TOO_LARGE
        assert _call(name, flags=4) == A.BAD_ARG and _call(name, flags=-1) == A.BAD_ARG
    if name == "tsgu_semi_mm":
        assert _call(name, bias=None) == A.BAD_ARG, "a NULL bias reaches set_device as well"
        assert _call(name, bias=base["bias"] + 1) == A.BAD_ARG
        assert _call(name, path=2) == A.BAD_ARG and _call(name, path=-1) == A.BAD_ARG
        assert _call(name, vtype=0, path=1) == A.BAD_ARG, "the sparse instruction is bfloat16's"
        # the layouts decide which stride bounds which extent
        assert _call(name, flags=0, ldc=39) == A.BAD_ARG and _call(name, flags=3, ldy=39) == A.BAD_ARG
    if name == "tsgu_semi_sddmm":
        assert _call(name, flags=2) == A.BAD_ARG, "the kept values have one layout"
