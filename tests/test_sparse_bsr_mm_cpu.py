"""sparse_bsr_mm without a GPU: argument refusals, CPU operands against the numpy float64 oracle, the forms of the gradients torch
allows for a BSR operand, and the C-ABI header of the block-sparse kernels with its host-side refusals."""

import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import _bsr_ref as br
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern, sparse_bsr_mm

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
NRB, NCB, P = 6, 5, 7
LENS = [3, 0, 5, 1, 2, 4]                     # an empty block row; with duplicates=True rows of two or more blocks repeat a column


def _bsr(bh, bw, dtype=torch.float64, index_dtype=torch.int64, seed=0, lens=LENS, ncb=NCB, duplicates=True, canonical=False):
    crow, col = br.random_bsr(len(lens), ncb, lens, seed, duplicates=duplicates, canonical=canonical)
    val = np.random.default_rng(seed + 1).standard_normal((len(col), bh, bw))
    A = torch.sparse_bsr_tensor(torch.from_numpy(crow).to(index_dtype), torch.from_numpy(col).to(index_dtype),
                                torch.from_numpy(val).to(dtype), (len(lens) * bh, ncb * bw))
    return A, crow, col, val


def _dense(shape, seed, dtype=torch.float64):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape)).to(dtype)


def _within(got, want, mag, terms):
    """|err| <= terms · 2^-53 · sum |terms|: the float64 bound of a sum of `terms` products in any order."""
    err = np.abs(got.detach().numpy() - want)
    bound = terms * U64 * mag
    assert (err <= bound).all(), float((err - bound).max())


def test_exports():
    assert {"sparse_bsr_mm", "SparseBSRMatMul"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_bsr_mm) and issubclass(tsgu.SparseBSRMatMul, torch.autograd.Function)
    from torchsparsegradutils_amd.sparse_bsr_mm import __all__ as mod_all

    assert mod_all == ["sparse_bsr_mm", "SparseBSRMatMul"]
    assert callable(_pattern.from_bsr) and callable(_backend.bsr_mm_geometry)
    for name in ("bsr_spmm", "bsr_sddmm", "bsr_spmm_t"):
        assert callable(getattr(_backend, name))
    for what in ("autograd.grad", "values", ".backward()", "AccumulateGrad"):
        assert what in sparse_bsr_mm.__doc__, what


# ---------------------------------------------------------------------------------------------------------------------------
# refusals


def test_refusals():
    A, *_ = _bsr(2, 4, dtype=torch.float32)
    m = A.size(1)
    B = _dense((m, P), 5, torch.float32)
    with pytest.raises(ValueError, match=re.escape("Both A and B should be instances of torch.Tensor")):
        sparse_bsr_mm(A, None)
    with pytest.raises(ValueError, match=re.escape("Both A and B should be at least 2-dimensional tensors")):
        sparse_bsr_mm(A, B[0])
    with pytest.raises(ValueError, match=re.escape("A and B must both be 2D or both be 3D tensors")):
        sparse_bsr_mm(A, B.unsqueeze(0))
    dense = A.to_dense()
    others = (dense, dense.to_sparse_csr(), dense.to_sparse_csc(), dense.to_sparse_coo(), dense.to_sparse_bsc((2, 4)))
    for other in others:
        with pytest.raises(ValueError, match=re.escape("A should be in BSR sparse format")):
            sparse_bsr_mm(other, B)
    hybrid = torch.sparse_bsr_tensor(torch.tensor([0, 1]), torch.tensor([0]), torch.zeros(1, 2, 4, 3), (2, 4, 3))
    assert hybrid.dense_dim() == 1
    with pytest.raises(ValueError, match=re.escape("A must not have dense dimensions, got dense_dim() = 1")):
        sparse_bsr_mm(hybrid, torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match=re.escape("B must be a dense (strided) tensor")):
        sparse_bsr_mm(A, B.to_sparse())
    crow, col, val = A.crow_indices(), A.col_indices(), A.values()
    batched = torch.sparse_bsr_tensor(torch.stack([crow, crow]), torch.stack([col, col]), torch.stack([val, val]), (2,) + tuple(A.shape))
    with pytest.raises(ValueError, match=re.escape("If batched, A and B must have the same batch size")):
        sparse_bsr_mm(batched, torch.zeros(3, m, P))
    with pytest.raises(ValueError, match=re.escape(f"Incompatible inner dimensions: A[..., {m}] vs B[..., {m + 1}]")):
        sparse_bsr_mm(A, torch.zeros(m + 1, P))
    with pytest.raises(RuntimeError, match=re.escape("A and B must be on the same device, got cpu and meta")):
        sparse_bsr_mm(A, torch.zeros(m, P, device="meta"))
    with pytest.raises(RuntimeError, match=re.escape("expected A and B to have the same dtype, got torch.float32 and torch.float64")):
        sparse_bsr_mm(A, B.double())
    half = torch.sparse_bsr_tensor(crow, col, val.half(), A.shape)
    with pytest.raises(RuntimeError, match=re.escape("unsupported value dtype torch.float16")):
        sparse_bsr_mm(half, B.half())
    with pytest.raises(ValueError, match=re.escape("B needs at least one column")):
        sparse_bsr_mm(A, torch.zeros(m, 0))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU operands against the oracle


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("block", [(2, 4), (3, 5), (16, 16), (1, 1)])
def test_cpu_operands_against_the_oracle(block, index_dtype):
    bh, bw = block
    A, crow, col, val = _bsr(bh, bw, index_dtype=index_dtype)
    assert len(col) != len({(i, j) for i, j in zip(br.block_rows(crow), col)})          # a repeated (I, J) is present
    B, G = _dense((NCB * bw, P), 5), _dense((NRB * bh, P), 6)
    Ag, Bg = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)
    C = sparse_bsr_mm(Ag, Bg)
    gA, gB = torch.autograd.grad(C, (Ag, Bg), G)
    Cr, mag, terms = br.forward(crow, col, val, B.numpy(), bh, bw)
    _within(C, Cr, mag, terms[:, None])
    assert C.shape == (NRB * bh, P) and (C[bh:2 * bh] == 0).all()                        # the empty block row
    dV, mag_v, dB, mag_b, terms_b = br.gradients(crow, col, val, B.numpy(), G.numpy(), bh, bw)
    assert gA.layout == torch.sparse_bsr and gA.shape == A.shape and gA.values().shape == (len(col), bh, bw)
    assert gA.crow_indices().dtype == index_dtype and gA.col_indices().dtype == index_dtype
    _within(gA.values(), dV, mag_v, P)
    _within(gB, dB, mag_b, terms_b[:, None])
    assert gB.shape == B.shape
    # the two stored copies of a repeated block get the same gradient, each its own
    e = int(crow[0])
    assert col[e] == col[e + LENS[0] - 1] and torch.equal(gA.values()[e], gA.values()[e + LENS[0] - 1])


@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_batched_cpu_operands_against_the_oracle(index_dtype):
    bh, bw, b = 3, 5, 3
    items = [_bsr(bh, bw, index_dtype=index_dtype, seed=10 + i, lens=L) for i, L in enumerate(([3, 0, 2, 1], [0, 0, 5, 1], [2, 2, 1, 1]))]
    A = torch.sparse_bsr_tensor(torch.stack([a.crow_indices() for a, *_ in items]), torch.stack([a.col_indices() for a, *_ in items]),
                                torch.stack([a.values() for a, *_ in items]), (b, 4 * bh, NCB * bw))
    B, G = _dense((b, NCB * bw, P), 5), _dense((b, 4 * bh, P), 6)
    Ag, Bg = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)
    C = sparse_bsr_mm(Ag, Bg)
    gA, gB = torch.autograd.grad(C, (Ag, Bg), G)
    assert C.shape == (b, 4 * bh, P) and gB.shape == B.shape and gA.layout == torch.sparse_bsr and gA.values().shape == (b, 6, bh, bw)
    assert gA.col_indices().dtype == index_dtype
    for i, (_, crow, col, val) in enumerate(items):
        Cr, mag, terms = br.forward(crow, col, val, B[i].numpy(), bh, bw)
        _within(C[i], Cr, mag, terms[:, None])
        dV, mag_v, dB, mag_b, terms_b = br.gradients(crow, col, val, B[i].numpy(), G[i].numpy(), bh, bw)
        _within(gA.values()[i], dV, mag_v, P)
        _within(gB[i], dB, mag_b, terms_b[:, None])


def test_a_matrix_without_blocks():
    for bh, bw in ((2, 4), (16, 16)):
        A = torch.sparse_bsr_tensor(torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                                    torch.zeros(0, bh, bw, dtype=torch.float64), (3 * bh, 2 * bw)).requires_grad_(True)
        B = _dense((2 * bw, P), 5).requires_grad_(True)
        C = sparse_bsr_mm(A, B)
        assert C.shape == (3 * bh, P) and (C == 0).all()
        gA, gB = torch.autograd.grad(C, (A, B), torch.ones_like(C))
        assert gA.values().shape == (0, bh, bw) and gB.shape == B.shape and (gB == 0).all()


def test_bfloat16_and_float32_accumulate_in_float32():
    bh, bw = 3, 5
    _, crow, col, val = _bsr(bh, bw)
    for dtype in (torch.float32, torch.bfloat16):
        v = torch.from_numpy(val).to(dtype)
        A = torch.sparse_bsr_tensor(torch.from_numpy(crow), torch.from_numpy(col), v, (NRB * bh, NCB * bw))
        B = _dense((NCB * bw, P), 5, dtype)
        C = sparse_bsr_mm(A, B)
        Cr, mag, terms = br.forward(crow, col, v.double().numpy(), B.double().numpy(), bh, bw)
        ulp = np.where(Cr == 0, 0.0, 2.0 ** (np.floor(np.log2(np.abs(Cr) + (Cr == 0))) - 7)) if dtype == torch.bfloat16 else 0.0
        bound = ulp + 2 * terms[:, None] * 2.0 ** -24 * mag
        assert C.dtype == dtype and (np.abs(C.double().numpy() - Cr) <= bound).all()


def test_a_strided_view_of_b_and_one_sided_gradients():
    bh, bw = 2, 4
    A, *_ = _bsr(bh, bw)
    B, G = _dense((NCB * bw, P), 5), _dense((NRB * bh, P), 6)
    want = sparse_bsr_mm(A, B)
    assert not want.requires_grad
    Bt = B.t().contiguous().t()
    wide = _dense((NCB * bw, 2 * P), 5)
    wide[:, ::2] = B
    assert not Bt.is_contiguous() and torch.equal(sparse_bsr_mm(A, Bt), want) and torch.equal(sparse_bsr_mm(A, wide[:, ::2]), want)
    Ag, Bg = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)
    gA, gB = torch.autograd.grad(sparse_bsr_mm(Ag, Bg), (Ag, Bg), G)
    (only_a,) = torch.autograd.grad(sparse_bsr_mm(Ag, B), (Ag,), G)
    (only_b,) = torch.autograd.grad(sparse_bsr_mm(A, Bg), (Bg,), G)
    assert torch.equal(only_a.values(), gA.values()) and torch.equal(only_b, gB)


# ---------------------------------------------------------------------------------------------------------------------------
# what torch allows for the gradient of a BSR operand


def test_gradcheck_through_a_values_parameter():
    bh, bw = 3, 2
    A, *_ = _bsr(bh, bw, lens=[2, 0, 3], ncb=3, canonical=True)      # (torch's own backward of sparse_bsr_tensor sorts and merges the blocks)
    crow, col = A.crow_indices(), A.col_indices()
    values = A.values().clone().requires_grad_(True)
    B = _dense((3 * bw, 4), 5).requires_grad_(True)

    def f(v, b):
        return sparse_bsr_mm(torch.sparse_bsr_tensor(crow, col, v, A.shape), b)

    assert torch.autograd.gradcheck(f, (values, B), eps=1e-6, atol=1e-7)


def test_autograd_grad_with_respect_to_a_bsr_leaf():
    for index_dtype in (torch.int32, torch.int64):
        A, *_ = _bsr(2, 4, index_dtype=index_dtype)
        A.requires_grad_(True)
        B = _dense((NCB * 4, P), 5)
        (gA,) = torch.autograd.grad(sparse_bsr_mm(A, B).sum(), (A,))
        assert gA.layout == torch.sparse_bsr and gA.shape == A.shape and gA.values().shape == A.values().shape
        assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and gA.col_indices().data_ptr() == A.col_indices().data_ptr()
        assert gA.crow_indices().dtype == index_dtype and gA.col_indices().dtype == index_dtype


def test_backward_reaches_a_values_parameter():
    A, crow, col, val = _bsr(2, 4, canonical=True)
    values = torch.nn.Parameter(A.values().clone())
    B, G = _dense((NCB * 4, P), 5), _dense((NRB * 2, P), 6)
    (sparse_bsr_mm(torch.sparse_bsr_tensor(A.crow_indices(), A.col_indices(), values, A.shape), B) * G).sum().backward()
    dV, mag_v, *_ = br.gradients(crow, col, val, B.numpy(), G.numpy(), 2, 4)
    assert values.grad is not None and values.grad.shape == values.shape
    _within(values.grad, dV, mag_v, P)


def test_the_pattern_is_cached_on_the_index_tensors():
    A, *_ = _bsr(2, 4)
    B = _dense((NCB * 4, P), 5)
    crow, col = A.crow_indices(), A.col_indices()
    sparse_bsr_mm(A, B)
    entries, _ = _pattern.cache_stats()
    assert entries == 1
    for _ in range(3):          # fresh BSR tensors on the same index tensors: the training-loop form
        sparse_bsr_mm(torch.sparse_bsr_tensor(crow, col, torch.randn_like(A.values()), A.shape), B)
    assert _pattern.cache_stats()[0] == 1
    # the block size is part of the key: the same index tensors under another block size are another matrix
    sparse_bsr_mm(torch.sparse_bsr_tensor(crow, col, torch.zeros(len(col), 4, 2, dtype=torch.float64), (NRB * 4, NCB * 2)), _dense((NCB * 2, P), 7))
    assert _pattern.cache_stats()[0] == 2


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: include/tsgu_hip_bsr.h

FAKE = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _addr(k):
    return FAKE + k * 0x100000


_COMMON = dict(vtype=0, itype=0, n_block_rows=40, n_block_cols=30, nnzb=500, bh=16, bw=16)


def _spmm(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), val=_addr(2), B=_addr(3), ldb=64, p=64, C=_addr(4), ldc=64, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_bsr_spmm(*a.values())


def _sddmm(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), G=_addr(5), ldg=64, B=_addr(3), ldb=64, p=64, dval=_addr(6), device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_bsr_sddmm(*a.values())


def _spmm_t(lib, **kw):
    a = dict(_COMMON, ptr=_addr(0), idx=_addr(1), perm=_addr(7), val=_addr(2), G=_addr(5), ldg=64, p=64, dB=_addr(8), lddb=64, device=-1,
             stream=None)
    a.update(kw)
    return lib.tsgu_bsr_spmm_t(*a.values())


# (call, pointers every call needs, pointers only stored blocks need, leading dimensions, dense operands, the walked side)
CALLS = [(_spmm, ("ptr", "C"), ("idx", "val", "B"), ("ldb", "ldc"), ("B", "C"), "n_block_rows"),
         (_sddmm, ("ptr",), ("idx", "G", "B", "dval"), ("ldg", "ldb"), ("G", "B"), "n_block_rows"),
         (_spmm_t, ("ptr", "dB"), ("idx", "perm", "val", "G"), ("ldg", "lddb"), ("G", "dB"), "n_block_cols")]


@pytest.mark.parametrize("call,always,stored,strides,dense,walked", CALLS, ids=["spmm", "sddmm", "spmm_t"])
def test_launcher_refusals_on_the_host(call, always, stored, strides, dense, walked):
    """The order of the refusals: null pointers, the types, the counts, the leading dimensions, the size limits — each pinned by a
    call that breaks two of them and shows the status of the earlier one."""
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert call(lib) == BAD_ARG
    for vt in (1, 2):
        assert call(lib, vtype=vt) == BAD_ARG
    assert call(lib, itype=1) == BAD_ARG and call(lib, p=1) == BAD_ARG and call(lib, p=33) == BAD_ARG
    for block in ((1, 1), (3, 5), (72, 136), (16, 64)):
        assert call(lib, bh=block[0], bw=block[1]) == BAD_ARG
    # 1. null pointers, before the types
    for name in always + stored:
        assert call(lib, **{name: None}) == BAD_ARG, name
        assert call(lib, vtype=7, **{name: None}) == BAD_ARG, name
    for name in always:
        assert call(lib, nnzb=0, vtype=7, **{name: None}) == BAD_ARG, name
    for name in stored:                                     # a pattern without blocks dereferences none of these
        assert call(lib, nnzb=0, vtype=7, **{name: None}) == BAD_DTYPE, name
    # 2. the types, before the counts
    for vt in (3, 7, -1):
        assert call(lib, vtype=vt) == BAD_DTYPE and call(lib, vtype=vt, p=0) == BAD_DTYPE
    for it in (2, -1):
        assert call(lib, itype=it) == BAD_DTYPE and call(lib, itype=it, bh=0) == BAD_DTYPE
    # 3. the counts, before the leading dimensions and the limits
    for name in ("p", "bh", "bw"):
        assert call(lib, **{name: 0}) == BAD_ARG and call(lib, **{name: -3}) == BAD_ARG, name
        assert call(lib, **{name: 0, strides[0]: 1 << 40}) == BAD_ARG and call(lib, **{name: 0, "nnzb": 1 << 40}) == BAD_ARG, name
    for name in ("n_block_rows", "n_block_cols", "nnzb"):
        assert call(lib, **{name: -1}) == BAD_ARG and call(lib, **{name: -1, strides[0]: 1 << 40}) == BAD_ARG, name
    # 4. a leading dimension below p and dense pointers that are not whole elements, before the limits
    for name in strides:
        assert call(lib, **{name: 63}) == BAD_ARG and call(lib, **{name: 63, "nnzb": 1 << 40}) == BAD_ARG, name
        assert call(lib, **{name: 63, walked: 0}) == BAD_ARG, name
    for name in dense:
        assert call(lib, **{name: _addr(3) + 2, walked: 0}) == BAD_ARG and call(lib, vtype=2, **{name: _addr(3) + 2, walked: 0}) == OK, name
        assert call(lib, vtype=1, **{name: _addr(3) + 4, walked: 0}) == BAD_ARG and call(lib, **{name: _addr(3) + 4, walked: 0}) == OK, name
    # 5. the limits: strides below 2^32; nnzb·bh·bw, n_block_rows·bh and n_block_cols·bw below 2^31
    for name in strides:
        assert call(lib, **{name: 1 << 40}) == TOO_LARGE and call(lib, **{name: (1 << 32) - 1}) == BAD_ARG, name
    assert call(lib, nnzb=1 << 23) == TOO_LARGE and call(lib, nnzb=(1 << 23) - 1) == BAD_ARG
    assert call(lib, n_block_rows=1 << 27) == TOO_LARGE and call(lib, n_block_rows=(1 << 27) - 1) == BAD_ARG
    assert call(lib, n_block_cols=1 << 27) == TOO_LARGE and call(lib, n_block_cols=(1 << 27) - 1) == BAD_ARG
    assert call(lib, bh=1 << 40) == TOO_LARGE and call(lib, bw=1 << 40) == TOO_LARGE and call(lib, nnzb=1 << 40) == TOO_LARGE
    # the refusals do not depend on the device
    assert call(lib, device=0, vtype=7) == BAD_DTYPE and call(lib, device=0, ptr=None) == BAD_ARG
    # nothing to walk is not an error (and touches no device), but only behind every check
    assert call(lib, **{walked: 0}) == OK and call(lib, **{walked: 0, "vtype": 7}) == BAD_DTYPE
    assert call(lib, **{walked: 0, strides[0]: 1 << 40}) == TOO_LARGE
    if call is _sddmm:
        assert call(lib, nnzb=0, idx=None, G=None, B=None, dval=None) == OK              # (no blocks: nothing to write)
    else:
        assert call(lib, nnzb=0, **{name: None for name in stored}) == BAD_ARG          # (zeros are written: reaches set_device)


def test_the_geometry_query():
    lib = _backend.load_library()
    r, c, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_bsr_mm_geometry(5, 16, 16, 32, ref(r), ref(c), ref(s)) == BAD_DTYPE
    assert lib.tsgu_bsr_mm_geometry(0, 16, 16, 0, ref(r), ref(c), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_mm_geometry(0, 0, 16, 32, ref(r), ref(c), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_mm_geometry(0, 16, -1, 32, ref(r), ref(c), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_mm_geometry(0, 16, 16, 32, None, ref(c), ref(s)) == BAD_ARG
    assert lib.tsgu_bsr_mm_geometry(7, 16, 16, 32, None, ref(c), ref(s)) == BAD_ARG      # (null pointers first)
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        stages = set()
        for p in (1, 17, 4096):
            for bh, bw in ((16, 16), (1, 1), (3, 5), (128, 128), (1000, 7)):
                rows, cols, stage = _backend.bsr_mm_geometry(dtype, bh, bw, p)
                assert rows >= 16 and rows % 16 == 0 and cols >= 16 and cols % 16 == 0 and rows <= 1024 and cols <= 1024
                assert stage >= 4 and stage * dtype.itemsize % 16 == 0 and stage <= 1024
                stages.add(stage)
        assert len(stages) == 1                      # the stage depends on the value type only
    with pytest.raises(RuntimeError, match="tsgu_bsr_mm_geometry failed"):
        _backend.bsr_mm_geometry(torch.float32, 16, 16, 0)
