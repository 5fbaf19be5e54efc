"""sparse_attention without a GPU: the torch-op path against the dense float64 oracle (tests/_attention_ref.py), index identity,
gradient presence, special values, refusals, exports, the C ABI of include/tsgu_hip_attention.h (exports, ctypes table,
host-side refusals with device = -1) and that nothing is densified.

Tolerances: tests/_attention_ref.py::error_bounds (the first-order bound of the GPU tests, derived there) with 4u in place of u,
u = 2^-24 for float32 and bfloat16 operands (computed in float32), 2^-53 for float64.  The torch-op path makes the kernels'
operations unfused: a product and a sum where they make one fma, P normalised by a division before it is used where they take
exp(t − lse), the scale applied to the finished sums — at most twice the roundings of every term, taken as four.  bfloat16 adds
its one rounding of the result: 2^-8 of the oracle's magnitude.
"""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import _attention_ref as ar
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern
from torchsparsegradutils_amd import sparse_attention               # (ImportError before the operator existed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24}
TINY = {torch.float32: float(np.finfo(np.float32).tiny), torch.float64: float(np.finfo(np.float64).tiny),
        torch.bfloat16: float(np.finfo(np.float32).tiny)}
U_STORE = {torch.float32: 0.0, torch.float64: 0.0, torch.bfloat16: 2.0 ** -8}
N, M, D = 13, 9, 8


def _mask(n, m, density, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand((n, m), generator=g) < density
    mask[n // 2] = False        # an empty row and an empty column
    mask[:, m // 3] = False
    return mask


def _operands(batch, heads, dtype, seed, n=N, m=M, d=D):
    """(B, Q, K, V, dO) ~ N(0, 1) rounded to `dtype`, as float64: what the value type holds is what the oracle gets."""
    g = torch.Generator().manual_seed(seed)
    lead = () if batch is None else (batch,)
    hd = (d,) if heads is None else (heads, d)
    shapes = (lead + (n, m), lead + (n,) + hd, lead + (m,) + hd, lead + (m,) + hd, lead + (n,) + hd)
    return [torch.randn(s, generator=g, dtype=torch.float64).to(dtype).double() for s in shapes]


def _check(got, want, bound, dtype, what):
    err = (got.double() - want).abs()
    lim = bound + U_STORE[dtype] * want.abs()
    assert got.dtype == dtype and got.shape == want.shape, what
    assert bool((err <= lim).all()), (what, float((err / lim.clamp(min=1e-300)).max()))


LAYOUTS = [("coo", torch.int64), ("coo_uncoalesced", torch.int64), ("csr", torch.int32), ("csr", torch.int64), ("csc", torch.int32),
           ("csc", torch.int64)]


@pytest.mark.parametrize("use_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("heads", [None, 1, 3], ids=["H-", "H1", "H3"])
@pytest.mark.parametrize("batch", [None, 3], ids=["2d", "batched"])
@pytest.mark.parametrize("layout,index_dtype", LAYOUTS, ids=[f"{a}-{str(b)[6:]}" for a, b in LAYOUTS])
def test_cpu_path_matches_the_dense_oracle(layout, index_dtype, batch, heads, dtype, use_bias):
    mask = _mask(N, M, 0.4, 3)
    B, Q, K, V, dO = _operands(batch, heads, dtype, 4)
    scale = 0.37
    A = ar.sparse_from_dense(B, mask, layout, index_dtype, dtype).requires_grad_(True)
    q, k, v = (x.to(dtype).requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v, scale=scale, values_as_bias=use_bias)
    assert O.shape == q.shape and O.dtype == dtype and O.layout == torch.strided
    grads = torch.autograd.grad(O, (q, k, v) + ((A,) if use_bias else ()), dO.to(dtype))
    multi = heads is not None
    items = range(batch) if batch is not None else [None]
    for it in items:
        pick = (lambda x: x) if it is None else (lambda x: x[it])
        Bi, Qi, Ki, Vi, Gi = pick(B), ar.heads_view(pick(Q), multi), ar.heads_view(pick(K), multi), ar.heads_view(pick(V), multi), \
            ar.heads_view(pick(dO), multi)
        O64, dQ64, dK64, dV64, dB64, P = ar.dense_oracle(mask, Bi, Qi, Ki, Vi, Gi, scale, use_bias)
        bO, bQ, bK, bV, bA, rho = ar.error_bounds(mask, Bi, Qi, Ki, Vi, Gi, scale, use_bias, 4 * U[dtype], TINY[dtype], P, O64)
        assert rho < 2.0 ** -10
        shape = Qi.shape if multi else (N, D)
        _check(pick(O.detach()), O64.view(shape), bO.view(shape), dtype, "O")
        _check(pick(grads[0]), dQ64.view(shape), bQ.view(shape), dtype, "dQ")
        shape = Ki.shape if multi else (M, D)
        _check(pick(grads[1]), dK64.view(shape), bK.view(shape), dtype, "dK")
        _check(pick(grads[2]), dV64.view(shape), bV.view(shape), dtype, "dV")
    if not use_bias:
        return
    gA = grads[3]
    assert gA.layout == A.layout and gA.shape == A.shape and gA.dtype == dtype
    dB64, bA = [], []
    for it in items:
        pick = (lambda x: x) if it is None else (lambda x: x[it])
        Bi, Qi, Ki, Vi, Gi = pick(B), ar.heads_view(pick(Q), multi), ar.heads_view(pick(K), multi), ar.heads_view(pick(V), multi), \
            ar.heads_view(pick(dO), multi)
        O64, _, _, _, dB, P = ar.dense_oracle(mask, Bi, Qi, Ki, Vi, Gi, scale, True)
        dB64.append(dB)
        bA.append(ar.error_bounds(mask, Bi, Qi, Ki, Vi, Gi, scale, True, 4 * U[dtype], TINY[dtype], P, O64)[4])
    dB64, bA = (torch.stack(x) if batch is not None else x[0] for x in (dB64, bA))
    if layout == "coo_uncoalesced":       # (its gradient arrives through torch's coalesce: compared at the stored positions)
        where = mask.expand(B.shape)
        _check(gA.to_dense()[where], dB64[where], bA[where], dtype, "dA")
    else:
        _check(ar.values_of(gA), ar.stored_order(dB64, gA), ar.stored_order(bA, gA), dtype, "dA")


@pytest.mark.parametrize("layout,index_dtype", LAYOUTS, ids=[f"{a}-{str(b)[6:]}" for a, b in LAYOUTS])
@pytest.mark.parametrize("batch", [None, 2], ids=["2d", "batched"])
def test_the_gradient_of_A_carries_the_inputs_index_tensors(layout, index_dtype, batch):
    mask = _mask(9, 8, 0.5, 13)
    B, Q, K, V, dO = _operands(batch, 2, torch.float32, 14, n=9, m=8)
    A = ar.sparse_from_dense(B, mask, layout, index_dtype, torch.float32)
    if layout == "coo_uncoalesced":
        A = A.coalesce()                 # (the function coalesces such an input itself: its indices are new by necessity)
    A.requires_grad_(True)
    mine = ar.index_tensors(A)
    _pattern.clear_cache()
    q, k, v = (x.float().requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v)
    gA, gq = torch.autograd.grad(O, (A, q), dO.float())
    assert gA.layout == A.layout and gA.shape == A.shape and gq.shape == q.shape
    for a, b in zip(mine, ar.index_tensors(gA)):
        assert a.data_ptr() == b.data_ptr() and a.dtype == b.dtype == index_dtype and a.shape == b.shape


def test_gradient_presence():
    mask = _mask(N, M, 0.4, 3)
    B, Q, K, V, dO = _operands(None, 3, torch.float64, 5)
    A = ar.sparse_from_dense(B, mask, "csr", torch.int32, torch.float64).requires_grad_(True)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v, values_as_bias=False)
    gA, gq, gk, gv = torch.autograd.grad(O, (A, q, k, v), dO, allow_unused=True)
    assert gA is None and gq is not None and gk is not None and gv is not None
    # ... and the values are then ignored altogether
    A2 = ar.sparse_from_dense(B * 3 + 1, mask, "csr", torch.int32, torch.float64)
    assert torch.equal(O.detach(), sparse_attention(A2, Q, K, V, values_as_bias=False))
    # with the bias: a gradient for A only when A asks for one
    O = sparse_attention(A, q, k, v)
    assert torch.autograd.grad(O, A, dO)[0].layout == torch.sparse_csr
    O = sparse_attention(A.detach(), q, k, v)
    assert O.requires_grad and torch.autograd.grad(O, q, dO)[0].shape == q.shape
    # the default scale is d ** -0.5
    assert torch.equal(sparse_attention(A, Q, K, V).detach(), sparse_attention(A, Q, K, V, scale=D ** -0.5).detach())


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_special_values(layout):
    inf, nan = float("inf"), float("nan")
    rows = [[0.5, None, 1.0, -0.5],        # an ordinary row
            [None, None, None, None],      # no stored entry: zeros, zero gradients
            [-inf, -inf, None, -inf],      # nothing but -inf: NaN
            [-inf, 1.0, None, 2.0],        # -inf beside finite: weight 0, gradient 0
            [nan, 1.0, 0.0, None],         # a NaN: NaN
            [inf, 1.0, None, None]]        # +inf: NaN
    mask = torch.tensor([[v is not None for v in r] for r in rows])
    B = torch.tensor([[0.0 if v is None else v for v in r] for r in rows], dtype=torch.float64)
    g = torch.Generator().manual_seed(6)
    Q, K, V, dO = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((6, 2, 8), (4, 2, 8), (4, 2, 8), (6, 2, 8)))
    A = ar.sparse_from_dense(B, mask, layout, torch.int64, torch.float64).requires_grad_(True)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v, scale=0.5)
    gA, gq, gk, gv = torch.autograd.grad(O, (A, q, k, v), dO)
    O = O.detach()
    assert torch.equal(O[1], torch.zeros(2, 8, dtype=torch.float64)) and torch.equal(gq[1], torch.zeros(2, 8, dtype=torch.float64))
    assert O[2].isnan().all() and O[4].isnan().all() and O[5].isnan().all()
    assert O[0].isfinite().all() and O[3].isfinite().all()
    # rows 0 and 3 against the oracle on the finite rows alone (the NaN rows poison the columns they touch in dK, dV only)
    keep = torch.tensor([0, 3])
    O64, dQ64, _, _, dB64, P = ar.dense_oracle(mask[keep], B[keep], Q[keep], K, V, dO[keep], 0.5)
    assert torch.allclose(O[keep], O64, rtol=1e-12, atol=1e-14) and torch.allclose(gq[keep], dQ64, rtol=1e-12, atol=1e-13)
    assert bool((P[:, 1, 0] == 0).all())                       # (the oracle's weight of the -inf entry)
    dA = gA.to_dense()
    assert dA[3, 0] == 0 and torch.allclose(dA[keep][mask[keep]], dB64[mask[keep]], rtol=1e-12, atol=1e-13)
    assert torch.equal(dA[1], torch.zeros(4, dtype=torch.float64))


def test_an_in_place_change_of_the_bias_before_backward_is_refused():
    mask = _mask(N, M, 0.4, 3)
    B, Q, K, V, dO = _operands(None, 3, torch.float64, 5)
    vals = B[mask].clone().requires_grad_(True)
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = mask.sum(1).cumsum(0)
    bias = vals * 1.0
    A = torch.sparse_csr_tensor(crow, mask.nonzero()[:, 1], bias, mask.shape)
    O = sparse_attention(A, Q, K, V)
    with torch.no_grad():
        bias.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        torch.autograd.grad(O, vals, dO)


def test_names_are_exported():
    assert {"sparse_attention", "SparseAttention"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_attention) and tsgu.sparse_attention is sparse_attention


def test_refusals():
    name = "sparse_attention"
    A = torch.eye(4).to_sparse_csr()
    Q = torch.zeros(4, 8)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} supports 2-D or batched 3-D sparse tensors, got ndim=1.")):
        sparse_attention(torch.ones(3).to_sparse(), Q, Q, Q)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} does not support layout torch.strided.")):
        sparse_attention(torch.eye(4), Q, Q, Q)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} does not support layout torch.sparse_bsr.")):
        sparse_attention(torch.eye(4).to_sparse_bsr((2, 2)), Q, Q, Q)
    with pytest.raises(ValueError, match=re.escape(f"{name} requires a sparse tensor with zero dense dimensions.")):
        sparse_attention(torch.ones(3, 3, 2).to_sparse(2), Q, Q, Q)
    with pytest.raises(TypeError, match=re.escape(f"{name}: values must be float32, float64 or bfloat16, got torch.float16")):
        sparse_attention(A.half(), Q.half(), Q.half(), Q.half())
    with pytest.raises(TypeError, match=re.escape(f"{name}: A, Q, K and V must have one dtype, got torch.float32 for A and torch.float64 for K")):
        sparse_attention(A, Q, Q.double(), Q)
    with pytest.raises(TypeError, match=re.escape(f"{name}: V must be a dense tensor")):
        sparse_attention(A, Q, Q, A)
    with pytest.raises(ValueError, match=re.escape(f"{name}: Q must be [n, d] or [n, H, d], got (4,)")):
        sparse_attention(A, torch.zeros(4), Q, Q)
    with pytest.raises(ValueError, match=re.escape(f"{name}: Q must be [b, n, d] or [b, n, H, d] for a batched A, got (4, 8)")):
        sparse_attention(torch.stack([torch.eye(4)] * 2).to_sparse_coo(), Q, Q, Q)
    with pytest.raises(ValueError, match=re.escape(f"{name}: Q, K and V must have the same number of dimensions, got 2, 3 and 2")):
        sparse_attention(A, Q, Q.view(4, 1, 8), Q)
    with pytest.raises(ValueError, match=re.escape(f"{name}: Q must be (4, 8) for A of shape (4, 4), got (5, 8)")):
        sparse_attention(A, torch.zeros(5, 8), Q, Q)
    with pytest.raises(ValueError, match=re.escape(f"{name}: K must be (4, 2, 8) for A of shape (4, 4) and Q of shape (4, 2, 8), got (4, 3, 8)")):
        sparse_attention(A, torch.zeros(4, 2, 8), torch.zeros(4, 3, 8), torch.zeros(4, 3, 8))
    with pytest.raises(ValueError, match=re.escape(f"{name}: V must have K's shape (4, 8)")):
        sparse_attention(A, Q, Q, torch.zeros(4, 16))
    for bad in (float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match=re.escape(f"{name}: scale must be a finite number, got")):
            sparse_attention(A, Q, Q, Q, scale=bad)
    with pytest.raises(RuntimeError, match=re.escape("all operands must be on the same device, got cpu and meta")):
        sparse_attention(A, Q, torch.zeros(4, 8, device="meta"), Q)
    # the CPU path has no geometry limits; what the GPU kernels take is a host-side query of the library
    assert sparse_attention(A, torch.zeros(4, 5), torch.zeros(4, 5), torch.ones(4, 5)).shape == (4, 5)
    from torchsparsegradutils_amd.sparse_attention import LIMITS

    assert LIMITS == "d in {8, 16, 32, 64, 128}, V as wide as Q and K, and H*d <= 1024"


def test_the_geometry_query_knows_the_limits_without_a_gpu():
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        for d in (8, 16, 32, 64, 128):
            assert _backend.attention_supported(dtype, 1, d) and _backend.attention_supported(dtype, 1024 // d, d)
            assert not _backend.attention_supported(dtype, 1024 // d + 1, d)
        for d in (0, 1, 4, 12, 24, 48, 96, 256):
            assert not _backend.attention_supported(dtype, 1, d)
        assert not _backend.attention_supported(dtype, 0, 8) and not _backend.attention_supported(dtype, -1, 8)
    assert not _backend.attention_supported(torch.float16, 1, 8)
    # entry lanes, rows per workgroup, entries per staged slice: bfloat16 walks a row exactly as float32 does
    src = open(os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "attention_impl.h")).read()
    stage = int(re.search(r"kAttnStage\s*=\s*(\d+)", src).group(1))
    for heads, d in ((1, 8), (3, 16), (2, 64), (1, 128), (8, 128), (4, 32)):
        ep, rpb, st = _backend.attention_geometry(torch.float32, heads, d)
        assert st == stage and ep in (1, 2, 4) and 1 <= rpb <= 256 and 256 % rpb == 0
        assert _backend.attention_geometry(torch.bfloat16, heads, d)[0] == ep
    with pytest.raises(RuntimeError, match="tsgu_csr_attention_geometry failed"):
        _backend.attention_geometry(torch.float32, 1, 12)


# ---------------------------------------------------------------------------------------------------------------------------
# nothing is densified


def test_nothing_is_densified(monkeypatch):
    mask = _mask(N, M, 0.4, 3)
    B, Q, K, V, dO = _operands(None, 3, torch.float64, 5)
    A = ar.sparse_from_dense(B, mask, "csr", torch.int32, torch.float64).requires_grad_(True)
    C = ar.sparse_from_dense(B, mask, "csc", torch.int64, torch.float64).requires_grad_(True)
    q, k, v = (x.clone().requires_grad_(True) for x in (Q, K, V))

    def refuse(self, *a, **kw):
        raise AssertionError("to_dense called")

    monkeypatch.setattr(torch.Tensor, "to_dense", refuse)
    for S in (A, C):
        O = sparse_attention(S, q, k, v)
        gA, gq, gk, gv = torch.autograd.grad(O, (S, q, k, v), dO)
        assert gA.layout == S.layout and gq.shape == q.shape and gk.shape == k.shape and gv.shape == v.shape


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: the third header


FAKE = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _addr(k):
    return FAKE + k * 0x100000


def _forward(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), perm=None, bias=_addr(2), Q=_addr(3), ldq=64,
             K=_addr(4), ldk=64, V=_addr(5), ldv=64, heads=2, d=32, scale=0.25, O=_addr(6), ldo=64, lse=_addr(7), device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_attention(*a.values())


def _backward_rows(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), perm=None, bias=_addr(2), Q=_addr(3), ldq=64,
             K=_addr(4), ldk=64, V=_addr(5), ldv=64, dO=_addr(8), lddo=64, lse=_addr(7), heads=2, d=32, scale=0.25, dQ=_addr(9), lddq=64,
             delta=_addr(10), dA=_addr(11), device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_attention_backward_rows(*a.values())


def _backward_cols(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), perm=_addr(12), bias=_addr(2), Q=_addr(3),
             ldq=64, K=_addr(4), ldk=64, V=_addr(5), ldv=64, dO=_addr(8), lddo=64, lse=_addr(7), delta=_addr(10), heads=2, d=32,
             scale=0.25, dK=_addr(9), lddk=64, dV=_addr(13), lddv=64, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_attention_backward_cols(*a.values())


CALLS = [(_forward, ("ptr", "idx", "Q", "K", "V", "O", "lse"), ("ldq", "ldk", "ldv", "ldo"), ("perm", "bias")),
         (_backward_rows, ("ptr", "idx", "Q", "K", "V", "dO", "lse", "dQ", "delta"), ("ldq", "ldk", "ldv", "lddo", "lddq"),
          ("perm", "bias", "dA")),
         (_backward_cols, ("ptr", "idx", "Q", "K", "V", "dO", "lse", "delta", "dK", "dV"), ("ldq", "ldk", "ldv", "lddo", "lddk", "lddv"),
          ("perm", "bias"))]


@pytest.mark.parametrize("call,operands,strides,optional", CALLS, ids=["forward", "backward_rows", "backward_cols"])
def test_launcher_refusals_on_the_host(call, operands, strides, optional):
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert call(lib) == BAD_ARG
    assert call(lib, heads=1, d=64) == BAD_ARG and call(lib, ldq=128) == BAD_ARG           # (other valid forms reach set_device too)
    for name in optional:
        assert call(lib, **{name: None}) == BAD_ARG                                        # (allowed to be NULL: set_device again)
    for vt in (3, -1):
        assert call(lib, vtype=vt) == BAD_DTYPE
    for it in (2, -1):
        assert call(lib, itype=it) == BAD_DTYPE
    for name in ("n_rows", "n_cols", "nnz", "heads", "d"):
        assert call(lib, **{name: -1}) == BAD_ARG, name
    for name in operands:
        assert call(lib, **{name: None}) == BAD_ARG, name
    # rows are touched in 16-byte lanes: base and row stride must be multiples of 16 bytes, the stride at least heads·d
    for name in operands[2:]:
        if name not in ("lse", "delta"):
            assert call(lib, **{name: _addr(3) + 8}) == BAD_ARG, name
    for name in strides:
        assert call(lib, **{name: 63}) == BAD_ARG and call(lib, **{name: 66}) == BAD_ARG and call(lib, **{name: 60}) == BAD_ARG, name
        assert call(lib, **{name: 1 << 40}) == TOO_LARGE, name
    assert call(lib, vtype=2, ldq=68) == BAD_ARG                                           # (bf16: 8 elements per 16 bytes)
    # unsupported geometry
    for heads, d in ((1, 12), (1, 256), (2, 4), (0, 32), (33, 32), (9, 128)):
        assert call(lib, heads=heads, d=d, ldq=4096, ldk=4096, ldv=4096) == BAD_ARG, (heads, d)
    # grid too large, rows beyond 2^31
    assert call(lib, n_rows=1 << 40) == TOO_LARGE and call(lib, n_cols=1 << 40) == TOO_LARGE
    # the refusals do not depend on the device
    assert call(lib, device=0, vtype=7) == BAD_DTYPE and call(lib, device=0, ptr=None) == BAD_ARG
    # nothing to walk is not an error (and touches no device)
    empty = "n_cols" if call is _backward_cols else "n_rows"
    assert call(lib, **{empty: 0}) == OK


def test_the_query_entries_refuse_on_the_host():
    lib = _backend.load_library()
    ep, rpb, st = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_csr_attention_geometry(0, 2, 32, ref(ep), ref(rpb), ref(st)) == OK and ep.value * rpb.value > 0 and st.value > 0
    assert lib.tsgu_csr_attention_geometry(5, 2, 32, ref(ep), ref(rpb), ref(st)) == BAD_DTYPE
    assert lib.tsgu_csr_attention_geometry(0, 2, 12, ref(ep), ref(rpb), ref(st)) == BAD_ARG
    assert lib.tsgu_csr_attention_geometry(0, 2, 32, None, ref(rpb), ref(st)) == BAD_ARG
    assert lib.tsgu_csr_attention_supported(0, 2, 32) == 1 and lib.tsgu_csr_attention_supported(9, 2, 32) == 0
    assert lib.tsgu_csr_attention_supported(0, 2, 12) == 0 and lib.tsgu_csr_attention_supported(1, 9, 128) == 0
