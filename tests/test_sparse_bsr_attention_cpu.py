"""sparse_bsr_attention without a GPU: exports, argument refusals, CPU operands against the dense float64 oracle
(tests/_attention_ref.py, the block mask expanded to an element mask), the forms of the gradients torch allows for a BSR operand,
the pattern cache, and the C-ABI header of the block-sparse attention kernels with its host-side refusals."""

import ctypes
import os
import re
import warnings

import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import _attention_ref as ar
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern, sparse_bsr_attention

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
TINY64 = 2.2250738585072014e-308
CROW = [0, 3, 3, 5, 6]                         # an empty block row
COL = [3, 0, 1, 4, 2, 1]                       # unsorted block columns
NCB = 5


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _bsr(bh, bw, index_dtype=torch.int64, dtype=torch.float64, crow=CROW, col=COL, ncb=NCB, seed=1):
    val = _randn((len(col), bh, bw), seed).to(dtype)
    return torch.sparse_bsr_tensor(torch.tensor(crow, dtype=index_dtype), torch.tensor(col, dtype=index_dtype), val,
                                   ((len(crow) - 1) * bh, ncb * bw))


def _dense(A):
    """(mask, bias) [n, m] of a 2-D BSR tensor without repeated blocks."""
    crow, col, val = A.crow_indices().tolist(), A.col_indices().tolist(), A.values()
    bh, bw = val.shape[1:]
    mask, B = torch.zeros(A.shape, dtype=torch.bool), torch.zeros(A.shape, dtype=torch.float64)
    for i in range(len(crow) - 1):
        for e in range(crow[i], crow[i + 1]):
            mask[i * bh:(i + 1) * bh, col[e] * bw:(col[e] + 1) * bw] = True
            B[i * bh:(i + 1) * bh, col[e] * bw:(col[e] + 1) * bw] = val[e].double()
    return mask, B


def _blocks_of(A, D):
    crow, col = A.crow_indices().tolist(), A.col_indices().tolist()
    bh, bw = A.values().shape[1:]
    return torch.stack([D[i * bh:(i + 1) * bh, col[e] * bw:(col[e] + 1) * bw] for i in range(len(crow) - 1)
                        for e in range(crow[i], crow[i + 1])])


def _within(got, want, bound, what):
    assert torch.equal(got.isnan(), want.isnan()), what
    assert bool(((got.double() - want).abs() <= bound).all()), (what, float(((got.double() - want).abs() - bound).max()))


def _check_item(A, Q, K, V, dO, got, scale, use_bias=True):
    """got = (O, dQ, dK, dV, dA blocks or None) of one 2-D item against the oracle, within error_bounds(u = 2^-53)."""
    mask, B = _dense(A)
    live = mask & B.isfinite()                 # a -inf inside a block masks the element: the oracle's mask without it
    Bf = B.masked_fill(~live, 0.0)
    multi = Q.dim() == 3
    q, k, v, g = (ar.heads_view(x, multi) for x in (Q, K, V, dO))
    O, dQ, dK, dV, dB, P = ar.dense_oracle(live, Bf, q, k, v, g, scale, use_bias)
    bounds = ar.error_bounds(live, Bf, q, k, v, g, scale, use_bias, U64, TINY64, P, O)
    for name, a, w, b in zip(("O", "dQ", "dK", "dV"), got, (O, dQ, dK, dV), bounds):
        _within(a.reshape(w.shape), w, b, name)
    if got[4] is not None:
        _within(got[4], _blocks_of(A, dB.masked_fill(~live, 0.0)), _blocks_of(A, bounds[4]), "dA")
        assert bool((got[4][_blocks_of(A, (mask & ~live).double()) > 0] == 0).all())


def test_exports():
    assert {"sparse_bsr_attention", "SparseBSRAttention"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_bsr_attention) and issubclass(tsgu.SparseBSRAttention, torch.autograd.Function)
    from torchsparsegradutils_amd.sparse_bsr_attention import __all__ as mod_all

    assert mod_all == ["sparse_bsr_attention", "SparseBSRAttention"]
    for name in ("bsr_attention_supported", "bsr_attention_geometry", "bsr_attention", "bsr_attention_backward"):
        assert callable(getattr(_backend, name))
    for what in ("autograd.grad", "values", ".backward()", "AccumulateGrad", "bf16 MFMA", "-inf"):
        assert what in sparse_bsr_attention.__doc__, what


# ---------------------------------------------------------------------------------------------------------------------------
# refusals


def test_refusals():
    A = _bsr(2, 4, dtype=torch.float32)
    n, m = A.shape
    Q, K, V = torch.zeros(n, 3, 8), torch.zeros(m, 3, 8), torch.zeros(m, 3, 8)
    pre = "sparse_bsr_attention: "
    dense = A.to_dense()
    for other in (dense, dense.to_sparse_csr(), dense.to_sparse_coo(), dense.to_sparse_bsc((2, 4)), None):
        with pytest.raises(TypeError, match=re.escape(pre + "A must be a torch.sparse_bsr tensor")):
            sparse_bsr_attention(other, Q, K, V)
    hybrid = torch.sparse_bsr_tensor(torch.tensor([0, 1]), torch.tensor([0]), torch.zeros(1, 2, 4, 3), (2, 4, 3))
    with pytest.raises(ValueError, match=re.escape(pre + "A must not have dense dimensions, got dense_dim() = 1")):
        sparse_bsr_attention(hybrid, Q, K, V)
    half = torch.sparse_bsr_tensor(A.crow_indices(), A.col_indices(), A.values().half(), A.shape)
    with pytest.raises(TypeError, match=re.escape(pre + "values must be float32, float64 or bfloat16, got torch.float16")):
        sparse_bsr_attention(half, Q.half(), K.half(), V.half())
    with pytest.raises(TypeError, match=re.escape(pre + "K must be a dense tensor")):
        sparse_bsr_attention(A, Q, K.to_sparse(), V)
    with pytest.raises(TypeError, match=re.escape(pre + "A, Q, K and V must have one dtype, got torch.float32 for A and torch.float64 for V")):
        sparse_bsr_attention(A, Q, K, V.double())
    with pytest.raises(ValueError, match=re.escape(pre + "Q must be [n, d] or [n, H, d], got (8,)")):
        sparse_bsr_attention(A, Q[:, 0, 0], K, V)
    with pytest.raises(ValueError, match=re.escape(pre + "Q, K and V must have the same number of dimensions, got 3, 2 and 3")):
        sparse_bsr_attention(A, Q, K[:, 0], V)
    with pytest.raises(ValueError, match=re.escape(pre + f"Q must be ({n}, 3, 8) for A of shape ({n}, {m}), got ({n + 1}, 3, 8)")):
        sparse_bsr_attention(A, torch.zeros(n + 1, 3, 8), K, V)
    with pytest.raises(ValueError, match=re.escape(pre + f"K must be ({m}, 3, 8) for A of shape ({n}, {m}) and Q of shape ({n}, 3, 8), got")):
        sparse_bsr_attention(A, Q, torch.zeros(m, 2, 8), V)
    with pytest.raises(ValueError, match=re.escape(pre + f"V must have K's shape ({m}, 3, 8), got ({m}, 3, 4)")):
        sparse_bsr_attention(A, Q, K, torch.zeros(m, 3, 4))
    with pytest.raises(ValueError, match=re.escape(pre + "Q needs at least one head and one column")):
        sparse_bsr_attention(A, torch.zeros(n, 0), torch.zeros(m, 0), torch.zeros(m, 0))
    with pytest.raises(RuntimeError, match=re.escape("all operands must be on the same device, got cpu and meta")):
        sparse_bsr_attention(A, Q, K.to("meta"), V)
    for bad in (float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match=re.escape(pre + "scale must be a finite number, got")):
            sparse_bsr_attention(A, Q, K, V, scale=bad)
    batched = torch.sparse_bsr_tensor(torch.stack([A.crow_indices()] * 2), torch.stack([A.col_indices()] * 2),
                                      torch.stack([A.values()] * 2), (2, n, m))
    with pytest.raises(ValueError, match=re.escape(pre + "Q must be [b, n, d] or [b, n, H, d] for a batched A, got")):
        sparse_bsr_attention(batched, Q[:, 0], K[:, 0], V[:, 0])
    # the GPU limits are told by the library without a device
    assert _backend.bsr_attention_supported(torch.float32, 1, 16, 16, 16) and _backend.bsr_attention_supported(torch.bfloat16, 9, 128, 160, 48)
    for heads, d, bh, bw in ((1, 8, 16, 16), (1, 48, 16, 16), (1, 256, 16, 16), (0, 16, 16, 16), (1, 16, 8, 16), (1, 16, 16, 24), (1, 16, 0, 16)):
        assert not _backend.bsr_attention_supported(torch.float32, heads, d, bh, bw)
    assert not _backend.bsr_attention_supported(torch.float16, 1, 16, 16, 16)
    assert "multiples of 16" in _backend.BSR_ATTENTION_LIMITS and "{16, 32, 64, 128}" in _backend.BSR_ATTENTION_LIMITS


# ---------------------------------------------------------------------------------------------------------------------------
# CPU operands against the oracle


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("block", [(2, 4), (16, 16)])
@pytest.mark.parametrize("heads", [None, 3])
def test_cpu_operands_against_the_oracle(block, index_dtype, heads):
    bh, bw = block
    A = _bsr(bh, bw, index_dtype).requires_grad_(True)
    n, m, d = A.size(0), A.size(1), 5
    hd = (d,) if heads is None else (heads, d)
    Q, K, V, dO = (_randn(s + hd, 3 + i).requires_grad_(i < 3) for i, s in enumerate(((n,), (m,), (m,), (n,))))
    O = sparse_bsr_attention(A, Q, K, V, scale=0.3)
    gA, gQ, gK, gV = torch.autograd.grad(O, (A, Q, K, V), dO)
    assert O.shape == Q.shape and gA.layout == torch.sparse_bsr and gA.shape == A.shape and gA.values().shape == A.values().shape
    assert gA.crow_indices().dtype == index_dtype and gA.col_indices().dtype == index_dtype
    assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and gA.col_indices().data_ptr() == A.col_indices().data_ptr()
    _check_item(A.detach(), Q.detach(), K.detach(), V.detach(), dO, (O.detach(), gQ, gK, gV, gA.values()), 0.3)
    assert bool((O[bh:2 * bh] == 0).all()) and bool((gQ[bh:2 * bh] == 0).all())          # the empty block row
    assert bool((gK[2 * bw:3 * bw] != 0).any())


def test_batched_cpu_operands_against_the_oracle():
    bh, bw, b, d, H = 2, 4, 3, 4, 2
    items = [_bsr(bh, bw, crow=c, col=j, seed=10 + i) for i, (c, j) in enumerate((([0, 2, 2, 5, 6], [1, 0, 4, 2, 3, 3]),
                                                                                  ([0, 0, 4, 5, 6], [3, 2, 1, 0, 0, 4]),
                                                                                  ([0, 1, 2, 3, 6], [2, 2, 2, 4, 0, 1])))]
    A = torch.sparse_bsr_tensor(torch.stack([a.crow_indices() for a in items]), torch.stack([a.col_indices() for a in items]),
                                torch.stack([a.values() for a in items]), (b,) + tuple(items[0].shape)).requires_grad_(True)
    n, m = items[0].shape
    Q, K, V, dO = (_randn((b, s, H, d), 3 + i).requires_grad_(i < 3) for i, s in enumerate((n, m, m, n)))
    O = sparse_bsr_attention(A, Q, K, V)
    gA, gQ, gK, gV = torch.autograd.grad(O, (A, Q, K, V), dO)
    assert O.shape == Q.shape and gK.shape == K.shape and gA.values().shape == (b, 6, bh, bw)
    for i, a in enumerate(items):
        _check_item(a, Q[i].detach(), K[i].detach(), V[i].detach(), dO[i], (O[i].detach(), gQ[i], gK[i], gV[i], gA.values()[i]), d ** -0.5)


def test_values_as_bias_false_and_minus_inf_inside_a_block():
    bh, bw, d = 2, 4, 6
    A = _bsr(bh, bw)
    n, m = A.shape
    Q, K, V, dO = (_randn((s, d), 3 + i).requires_grad_(i < 3) for i, s in enumerate((n, m, m, n)))
    Ag = A.detach().clone().requires_grad_(True)
    O = sparse_bsr_attention(Ag, Q, K, V, values_as_bias=False)
    gQ, gK, gV = torch.autograd.grad(O, (Q, K, V), dO, retain_graph=True)
    assert torch.autograd.grad(O.sum(), (Ag,), allow_unused=True)[0] is None
    _check_item(A, Q.detach(), K.detach(), V.detach(), dO, (O.detach(), gQ, gK, gV, None), d ** -0.5, use_bias=False)
    val = A.values().clone()
    val[0, 0, 1:] = float("-inf")                                         # -inf beside finite logits: weight 0, gradient 0
    val[3, 1, :] = float("-inf")
    val[4, 1, :] = float("-inf")                                          # row 2·bh + 1: nothing but -inf
    Ai = torch.sparse_bsr_tensor(A.crow_indices(), A.col_indices(), val, A.shape).requires_grad_(True)
    O = sparse_bsr_attention(Ai, Q, K, V)
    gA, gQ = torch.autograd.grad(O, (Ai, Q), dO)
    assert O[2 * bh + 1].isnan().all() and gQ[2 * bh + 1].isnan().all()
    assert O[:2 * bh + 1].isfinite().all() and O[2 * bh + 2:].isfinite().all()
    assert bool((gA.values()[0, 0, 1:] == 0).all())
    rows = [0, 1]
    mask, B = _dense(Ai.detach())
    live = mask & B.isfinite()
    want = ar.dense_oracle(live, B.masked_fill(~live, 0.0), *(ar.heads_view(x.detach(), False) for x in (Q, K, V)),
                           ar.heads_view(dO, False), d ** -0.5)
    assert torch.allclose(O[rows].detach(), want[0][rows, 0], rtol=1e-12, atol=1e-12)


def test_a_repeated_block_counts_twice():
    bh, bw, d = 2, 4, 3
    A = _bsr(bh, bw, crow=[0, 3], col=[1, 0, 1], ncb=2)
    E = torch.sparse_bsr_tensor(torch.tensor([0, 3]), torch.tensor([1, 0, 2]), A.values(), (bh, 3 * bw))
    Q, K, V = _randn((bh, d), 3), _randn((2 * bw, d), 4), _randn((2 * bw, d), 5)
    got = sparse_bsr_attention(A, Q, K, V)
    want = sparse_bsr_attention(E, Q, torch.cat([K, K[bw:]]), torch.cat([V, V[bw:]]))
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-13)


def test_bfloat16_and_float32_operands_on_the_cpu():
    bh, bw, d = 2, 4, 8
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 2.0 ** -6)):
        A = _bsr(bh, bw, dtype=dtype)
        n, m = A.shape
        Q, K, V = (_randn((s, 2, d), 3 + i).to(dtype) for i, s in enumerate((n, m, m)))
        O = sparse_bsr_attention(A, Q, K, V)
        want = sparse_bsr_attention(torch.sparse_bsr_tensor(A.crow_indices(), A.col_indices(), A.values().double(), A.shape),
                                    Q.double(), K.double(), V.double())
        assert O.dtype == dtype and torch.allclose(O.double(), want, rtol=tol, atol=tol)


# ---------------------------------------------------------------------------------------------------------------------------
# what torch allows for the gradient of a BSR operand; the pattern cache


def test_backward_reaches_a_values_parameter():
    bh, bw, d = 2, 4, 3
    A = _bsr(bh, bw, crow=[0, 2, 2, 3], col=[0, 2, 1], ncb=3)            # (torch's canonical pattern: sorted, no repeats)
    values = torch.nn.Parameter(A.values().clone())
    n, m = A.shape
    Q, K, V, dO = (_randn((s, d), 3 + i) for i, s in enumerate((n, m, m, n)))
    (sparse_bsr_attention(torch.sparse_bsr_tensor(A.crow_indices(), A.col_indices(), values, A.shape), Q, K, V) * dO).sum().backward()
    Ag = A.detach().clone().requires_grad_(True)
    (gA,) = torch.autograd.grad(sparse_bsr_attention(Ag, Q, K, V), (Ag,), dO)
    assert values.grad is not None and values.grad.shape == values.shape and torch.equal(values.grad, gA.values())
    assert bool((values.grad != 0).any())


def test_gradcheck_through_a_values_parameter():
    bh, bw, d = 2, 3, 2
    A = _bsr(bh, bw, crow=[0, 2, 2, 3], col=[0, 2, 1], ncb=3)
    crow, col = A.crow_indices(), A.col_indices()
    n, m = A.shape
    values = A.values().clone().requires_grad_(True)
    Q, K, V = (_randn((s, 2, d), 3 + i).requires_grad_(True) for i, s in enumerate((n, m, m)))

    def f(v, q, k, w):
        return sparse_bsr_attention(torch.sparse_bsr_tensor(crow, col, v, A.shape), q, k, w, scale=0.7)

    assert torch.autograd.gradcheck(f, (values, Q, K, V), eps=1e-6, atol=1e-6)


def test_the_pattern_is_cached_on_the_index_tensors():
    _pattern.clear_cache()
    A = _bsr(2, 4)
    n, m = A.shape
    Q, K, V = _randn((n, 3), 3), _randn((m, 3), 4), _randn((m, 3), 5)
    crow, col = A.crow_indices(), A.col_indices()
    sparse_bsr_attention(A, Q, K, V)
    assert _pattern.cache_stats()[0] == 1
    for _ in range(3):
        sparse_bsr_attention(torch.sparse_bsr_tensor(crow, col, torch.randn_like(A.values()), A.shape), Q, K, V)
    assert _pattern.cache_stats()[0] == 1
    tsgu.sparse_bsr_mm(A, _randn((m, 2), 6))                               # the same cache entry as sparse_bsr_mm's
    assert _pattern.cache_stats()[0] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: include/tsgu_hip_bsr_attention.h

FAKE = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _addr(k):
    return FAKE + k * 0x100000


_COMMON = dict(vtype=0, itype=0, n_block_rows=40, n_block_cols=30, nnzb=500, bh=16, bw=16)
_TAIL = dict(heads=2, d=32, scale=0.5)


def _fwd(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), bias=_addr(2), Q=_addr(3), ldq=64, K=_addr(4), ldk=64, V=_addr(5), ldv=64, **_TAIL,
             O=_addr(6), ldo=64, lse=_addr(7), O_acc=None, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_bsr_attention(*a.values())


def _rows(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), bias=_addr(2), Q=_addr(3), ldq=64, K=_addr(4), ldk=64, V=_addr(5), ldv=64,
             dO=_addr(8), lddo=64, O_acc=_addr(6), ldo=64, lse=_addr(7), **_TAIL, dQ=_addr(9), lddq=64, delta=_addr(10), dA=_addr(11),
             device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_bsr_attention_backward_rows(*a.values())


def _cols(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), perm=_addr(12), bias=_addr(2), Q=_addr(3), ldq=64, K=_addr(4), ldk=64, V=_addr(5),
             ldv=64, dO=_addr(8), lddo=64, lse=_addr(7), delta=_addr(10), **_TAIL, dK=_addr(13), lddk=64, dV=_addr(14), lddv=64,
             device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_bsr_attention_backward_cols(*a.values())


# (call, pointers every call needs, pointers only stored blocks need, pointers that may always be null, leading dimensions, walked side)
CALLS = [(_fwd, ("ptr", "Q", "O", "lse"), ("idx", "K", "V"), ("bias", "O_acc"), ("ldq", "ldk", "ldv", "ldo"), "n_block_rows"),
         (_rows, ("ptr", "Q", "dO", "O_acc", "lse", "dQ", "delta"), ("idx", "K", "V"), ("bias", "dA"),
          ("ldq", "ldk", "ldv", "lddo", "ldo", "lddq"), "n_block_rows"),
         (_cols, ("ptr", "K", "V", "dK", "dV"), ("idx", "perm", "Q", "dO", "lse", "delta"), ("bias",),
          ("ldq", "ldk", "ldv", "lddo", "lddk", "lddv"), "n_block_cols")]


@pytest.mark.parametrize("call,always,stored,optional,strides,walked", CALLS, ids=["forward", "rows", "cols"])
def test_launcher_refusals_on_the_host(call, always, stored, optional, strides, walked):
    """The order of the refusals: null pointers, the types, the counts and the geometry, the leading dimensions and alignment, the
    size limits — each pinned by a call that breaks two of them and shows the status of the earlier one."""
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert call(lib) == BAD_ARG
    for vt in (1, 2):
        assert call(lib, vtype=vt) == BAD_ARG
    assert call(lib, itype=1) == BAD_ARG
    for name in optional:
        assert call(lib, **{name: None}) == BAD_ARG and call(lib, **{name: None, walked: 0}) == OK, name
    # 1. null pointers, before the types
    for name in always + stored:
        assert call(lib, **{name: None}) == BAD_ARG, name
        assert call(lib, vtype=7, **{name: None}) == BAD_ARG, name
    for name in always:
        assert call(lib, nnzb=0, vtype=7, **{name: None}) == BAD_ARG, name
    for name in stored:                                     # a pattern without blocks dereferences none of these
        assert call(lib, nnzb=0, vtype=7, **{name: None}) == BAD_DTYPE, name
    # 2. the types, before the counts and the geometry
    for vt in (3, 7, -1):
        assert call(lib, vtype=vt) == BAD_DTYPE and call(lib, vtype=vt, d=7) == BAD_DTYPE
    for it in (2, -1):
        assert call(lib, itype=it) == BAD_DTYPE and call(lib, itype=it, bh=0) == BAD_DTYPE
    # 3. the counts and the geometry, before the leading dimensions and the limits (walked = 0 shows it is no device error)
    for kw in (dict(d=8), dict(d=48), dict(d=256), dict(heads=0), dict(heads=-1), dict(bh=8), dict(bw=24), dict(bh=0), dict(bw=-16),
               dict(n_block_rows=-1), dict(n_block_cols=-1), dict(nnzb=-1)):
        kw = dict(kw)
        kw.setdefault(walked, 0)
        assert call(lib, **kw) == BAD_ARG and call(lib, **{**kw, strides[0]: 1 << 40}) == BAD_ARG, kw
        assert call(lib, **{**kw, strides[0]: 63}) == BAD_ARG
    for d in (16, 32, 64):
        assert call(lib, **{walked: 0, "d": d, "heads": 1}) == OK
    assert call(lib, **{walked: 0, "d": 128, "heads": 3, **{name: 384 for name in strides}}) == OK
    # 4. a leading dimension below heads·d, a base or a row stride that is no multiple of 16 bytes, before the limits
    for name in strides:
        assert call(lib, **{name: 63, walked: 0}) == BAD_ARG and call(lib, **{name: 63, "nnzb": 1 << 40, walked: 0}) == BAD_ARG, name
        assert call(lib, **{name: 66, walked: 0}) == BAD_ARG and call(lib, vtype=1, **{name: 66, walked: 0}) == OK, name
        assert call(lib, **{name: 68, walked: 0}) == OK and call(lib, vtype=2, **{name: 68, walked: 0}) == BAD_ARG, name
    assert call(lib, Q=_addr(3) + 8, **{walked: 0}) == BAD_ARG and call(lib, K=_addr(4) + 4, **{walked: 0}) == BAD_ARG
    # 5. the limits: strides below 2^32; nnzb·bh·bw, n_block_rows·bh and n_block_cols·bw below 2^31
    for name in strides:
        assert call(lib, **{name: 1 << 40, walked: 0}) == TOO_LARGE and call(lib, **{name: (1 << 32) - 4}) == BAD_ARG, name
    assert call(lib, nnzb=1 << 23) == TOO_LARGE and call(lib, nnzb=(1 << 23) - 1) == BAD_ARG
    assert call(lib, n_block_rows=1 << 27) == TOO_LARGE and call(lib, n_block_cols=1 << 27) == TOO_LARGE
    assert call(lib, bh=1 << 40) == TOO_LARGE and call(lib, bw=1 << 40) == TOO_LARGE
    # the refusals do not depend on the device
    assert call(lib, device=0, vtype=7) == BAD_DTYPE and call(lib, device=0, ptr=None) == BAD_ARG
    # nothing to walk is not an error (and touches no device), but only behind every check
    assert call(lib, **{walked: 0}) == OK and call(lib, **{walked: 0, "vtype": 7}) == BAD_DTYPE


def test_the_geometry_query():
    lib = _backend.load_library()
    r, s = ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_bsr_attention_geometry(5, 1, 16, 16, 16, ref(r), ref(s)) == BAD_DTYPE
    assert lib.tsgu_bsr_attention_geometry(0, 1, 24, 16, 16, ref(r), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_attention_geometry(0, 1, 16, 16, 8, ref(r), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_attention_geometry(7, 1, 16, 16, 16, None, ref(s)) == BAD_ARG          # (null pointers first)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        for d in (16, 32, 64, 128):
            seen = set()
            for heads, bh, bw in ((1, 16, 16), (7, 64, 16), (2, 256, 48)):
                rows, stage = _backend.bsr_attention_geometry(dtype, heads, d, bh, bw)
                assert rows in (16, 32, 64, 128, 256) and stage % 16 == 0 and 16 <= stage <= 256
                seen.add((rows, stage))
            assert len(seen) == 1                    # the geometry depends on the value type and the head width only
    assert _backend.bsr_attention_geometry(torch.float64, 1, 128, 16, 16)[1] < _backend.bsr_attention_geometry(torch.float64, 1, 16, 16, 16)[1]
    with pytest.raises(RuntimeError, match="tsgu_bsr_attention_geometry failed"):
        _backend.bsr_attention_geometry(torch.float32, 1, 20, 16, 16)
