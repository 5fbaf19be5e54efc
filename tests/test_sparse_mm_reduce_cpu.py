"""sparse_mm_reduce without a GPU: CPU operands against torch.sparse.mm(A, B, reduce), the numpy oracle of the GPU tests against
the same op (bit for bit), argument refusals, and the fourth C-ABI header with its host-side refusals."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import _mm_reduce_ref as mr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_mm, sparse_mm_reduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, M, P = 13, 11, 5
LENS = [3, 0, 11, 1, 4, 0, 2, 5, 1, 3, 0, 6, 2]          # empty first-but-one, middle and (nearly) last rows, a full row
REDUCTIONS = ("amax", "amin", "mean", "sum")


def _csr(dtype, index_dtype, seed=0, ints=False, n=N, m=M, lens=LENS):
    crow, col = mr.random_csr(n, m, lens, seed)
    rng = np.random.default_rng(seed + 1)
    val = mr.small_ints(len(col), seed + 2) if ints else rng.standard_normal(len(col))
    A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(index_dtype), torch.from_numpy(col).to(index_dtype),
                                torch.from_numpy(val).to(dtype), (n, m))
    return A


def _dense(shape, dtype, seed, ints=False):
    x = mr.small_ints(shape, seed) if ints else np.random.default_rng(seed).standard_normal(shape)
    return torch.from_numpy(x).to(dtype)


def _torch_op(A_csr, B, G, reduce):
    """(C, gradient of the values, gradient of B) of torch's own op on 2-D CSR CPU operands."""
    A = A_csr.detach().clone().requires_grad_(True)
    Bg = B.detach().clone().requires_grad_(True)
    C = torch.sparse.mm(A, Bg, reduce)
    gA, gB = torch.autograd.grad(C, (A, Bg), G)
    return C.detach(), gA.values(), gB


def _ours(A, B, G, reduce):
    A = A.detach().clone().requires_grad_(True)
    Bg = B.detach().clone().requires_grad_(True)
    C = sparse_mm_reduce(A, Bg, reduce)
    gA, gB = torch.autograd.grad(C, (A, Bg), G)
    return C.detach(), gA, gB


def test_exports():
    assert {"sparse_mm_reduce", "SparseMMReduce"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_mm_reduce) and issubclass(tsgu.SparseMMReduce, torch.autograd.Function)
    from torchsparsegradutils_amd.sparse_mm_reduce import __all__ as mod_all

    assert mod_all == ["sparse_mm_reduce", "SparseMMReduce"]


# ---------------------------------------------------------------------------------------------------------------------------
# CPU operands: the torch op


@pytest.mark.parametrize("reduce", REDUCTIONS)
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_csr_cpu_operands_are_the_torch_op(dtype, index_dtype, reduce):
    A, B, G = _csr(dtype, index_dtype), _dense((M, P), dtype, 5), _dense((N, P), dtype, 6)
    C, gA, gB = _ours(A, B, G, reduce)
    Cr, gAr, gBr = _torch_op(A, B, G, reduce)
    if reduce in ("amax", "amin"):
        assert torch.equal(C, Cr) and torch.equal(gA.values(), gAr) and torch.equal(gB, gBr)
    else:       # (sum and mean run sparse_mm's products: equal up to the summation order)
        tol = 1e-5 if dtype == torch.float32 else 1e-13
        for x, y in ((C, Cr), (gA.values(), gAr), (gB, gBr)):
            assert float((x - y).abs().max()) <= tol * max(1.0, float(y.abs().max()))
    # the gradient's form: A's layout, on its index tensors, index dtype kept
    assert gA.layout == torch.sparse_csr and gA.shape == A.shape
    assert gA.crow_indices().dtype == index_dtype and gA.col_indices().dtype == index_dtype
    assert torch.equal(gA.crow_indices(), A.crow_indices()) and torch.equal(gA.col_indices(), A.col_indices())
    assert gB.shape == B.shape and C.shape == (N, P)


def test_bfloat16_cpu_operands_are_the_torch_op():
    A, B, G = _csr(torch.bfloat16, torch.int32), _dense((M, P), torch.bfloat16, 5), _dense((N, P), torch.bfloat16, 6)
    for reduce in ("amax", "amin"):
        C, gA, gB = _ours(A, B, G, reduce)
        Cr, gAr, gBr = _torch_op(A, B, G, reduce)
        assert torch.equal(C, Cr) and torch.equal(gA.values(), gAr) and torch.equal(gB, gBr)


def test_sum_is_sparse_mm():
    A, B = _csr(torch.float64, torch.int64), _dense((M, P), torch.float64, 5)
    assert torch.equal(sparse_mm_reduce(A, B, "sum"), sparse_mm(A, B))


def test_mean_is_sparse_mm_divided_by_the_stored_count():
    A, B, G = _csr(torch.float64, torch.int64), _dense((M, P), torch.float64, 5), _dense((N, P), torch.float64, 6)
    cnt = torch.tensor(LENS, dtype=torch.float64).clamp(min=1).unsqueeze(1)
    C, gA, gB = _ours(A, B, G, "mean")
    Am, Bm = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)
    Cm = sparse_mm(Am, Bm)
    gAm, gBm = torch.autograd.grad(Cm, (Am, Bm), G / cnt)
    assert torch.equal(C, Cm.detach() / cnt) and torch.equal(gA.values(), gAm.values()) and torch.equal(gB, gBm)
    assert torch.equal(C[[1, 5, 10]], torch.zeros(3, P, dtype=torch.float64))
    # a second call finds the count cached with the pattern
    assert torch.equal(sparse_mm_reduce(A, B, "mean"), C)


@pytest.mark.parametrize("reduce", ["amax", "amin", "mean"])
def test_coo_coalesced_and_uncoalesced(reduce):
    dtype = torch.float64
    Acsr = _csr(dtype, torch.int64)
    B, G = _dense((M, P), dtype, 5), _dense((N, P), dtype, 6)
    Cr, gAr, gBr = _torch_op(Acsr, B, G, reduce)
    tol = 0.0 if reduce != "mean" else 1e-13
    # coalesced
    Acoo = Acsr.to_sparse_coo().coalesce()
    C, gA, gB = _ours(Acoo, B, G, reduce)
    assert gA.layout == torch.sparse_coo and torch.equal(gA._indices(), Acoo._indices())
    for x, y in ((C, Cr), (gA._values(), gAr), (gB, gBr)):
        assert float((x - y).abs().max()) <= tol
    # un-coalesced: every entry stored as two parts, shuffled
    idx, val = Acoo._indices(), Acoo._values()
    nnz = val.numel()
    perm = torch.randperm(2 * nnz)
    idx2 = torch.cat((idx, idx), 1)[:, perm]
    val2 = torch.cat((val * 0.25, val * 0.75))[perm]
    Au = torch.sparse_coo_tensor(idx2, val2, (N, M))
    assert not Au.is_coalesced()
    C, gA, gB = _ours(Au, B, G, reduce)
    assert gA.layout == torch.sparse_coo and gA.shape == Au.shape
    tol = 1e-13
    assert float((C - Cr).abs().max()) <= tol and float((gB - gBr).abs().max()) <= tol
    # duplicates are one matrix entry (their sum is the candidate): the gradient is that entry's, handed on by coalesce's backward
    gAc = gA.coalesce()
    assert torch.equal(gAc._indices(), Acoo._indices())
    assert float((gAc._values() - gAr).abs().max()) <= tol


@pytest.mark.parametrize("reduce", ["amax", "amin", "mean"])
def test_batched_operands_against_a_loop_over_the_items(reduce):
    dtype = torch.float64
    lens = ([3, 0, 2, 4, 1], [0, 0, 5, 1, 1], [2, 2, 2, 2, 2])
    items = [_csr(dtype, torch.int64, seed=10 + b, n=5, m=6, lens=L) for b, L in enumerate(lens)]
    B, G = _dense((3, 6, P), dtype, 5), _dense((3, 5, P), dtype, 6)
    ref = [_torch_op(items[b], B[b], G[b], reduce) for b in range(3)]
    # batched COO, items of unequal nnz
    Acoo = torch.stack([a.to_sparse_coo() for a in items]).coalesce()
    C, gA, gB = _ours(Acoo, B, G, reduce)
    assert C.shape == (3, 5, P) and gA.layout == torch.sparse_coo and torch.equal(gA._indices(), Acoo._indices())
    tol = 0.0 if reduce != "mean" else 1e-13
    for b in range(3):
        assert float((C[b] - ref[b][0]).abs().max()) <= tol and float((gB[b] - ref[b][2]).abs().max()) <= tol
    assert float((gA._values() - torch.cat([r[1] for r in ref])).abs().max()) <= tol
    # batched CSR (equal nnz per item)
    same = [_csr(dtype, torch.int32, seed=20 + b, n=5, m=6, lens=L) for b, L in enumerate(([3, 0, 2, 4, 1], [0, 4, 5, 0, 1], [2, 2, 2, 2, 2]))]
    Acsr = torch.sparse_csr_tensor(torch.stack([a.crow_indices() for a in same]), torch.stack([a.col_indices() for a in same]),
                                   torch.stack([a.values() for a in same]), (3, 5, 6))
    ref = [_torch_op(same[b], B[b], G[b], reduce) for b in range(3)]
    C, gA, gB = _ours(Acsr, B, G, reduce)
    assert gA.layout == torch.sparse_csr and gA.col_indices().dtype == torch.int32 and gA.values().shape == (3, 10)
    for b in range(3):
        assert float((C[b] - ref[b][0]).abs().max()) <= tol and float((gB[b] - ref[b][2]).abs().max()) <= tol
        assert float((gA.values()[b] - ref[b][1]).abs().max()) <= tol


def test_only_one_operand_requires_a_gradient():
    A, B, G = _csr(torch.float64, torch.int64), _dense((M, P), torch.float64, 5), _dense((N, P), torch.float64, 6)
    _, gAr, gBr = _torch_op(A, B, G, "amax")
    Ag = A.detach().clone().requires_grad_(True)
    (gA,) = torch.autograd.grad(sparse_mm_reduce(Ag, B, "amax"), (Ag,), G)
    assert torch.equal(gA.values(), gAr)
    Bg = B.clone().requires_grad_(True)
    (gB,) = torch.autograd.grad(sparse_mm_reduce(A, Bg, "amax"), (Bg,), G)
    assert torch.equal(gB, gBr)
    assert not sparse_mm_reduce(A, B, "amax").requires_grad
    # a transposed view of B is taken as it is
    Bt = B.t().contiguous().t()
    assert not Bt.is_contiguous() and torch.equal(sparse_mm_reduce(A, Bt, "amin"), sparse_mm_reduce(A, B, "amin"))


def test_refusals():
    A, B = _csr(torch.float32, torch.int64), _dense((M, P), torch.float32, 5)
    with pytest.raises(ValueError, match=re.escape("Both A and B should be instances of torch.Tensor")):
        sparse_mm_reduce(A, None)
    with pytest.raises(ValueError, match=re.escape("reduce must be one of 'sum', 'mean', 'amax' or 'amin', got 'max'")):
        sparse_mm_reduce(A, B, "max")
    with pytest.raises(ValueError, match=re.escape("Both A and B should be at least 2-dimensional tensors")):
        sparse_mm_reduce(A, B[0])
    with pytest.raises(ValueError, match=re.escape("A and B must both be 2D or both be 3D tensors")):
        sparse_mm_reduce(A, B.unsqueeze(0))
    with pytest.raises(ValueError, match=re.escape("A should be in either COO or CSR sparse format")):
        sparse_mm_reduce(A.to_sparse_csc(), B)
    with pytest.raises(ValueError, match=re.escape("A should be in either COO or CSR sparse format")):
        sparse_mm_reduce(A.to_dense(), B)
    with pytest.raises(ValueError, match=re.escape("B must be a dense (strided) tensor")):
        sparse_mm_reduce(A, B.to_sparse())
    batched = torch.stack([A.to_sparse_coo(), A.to_sparse_coo()])
    with pytest.raises(ValueError, match=re.escape("If batched, A and B must have the same batch size")):
        sparse_mm_reduce(batched, torch.zeros(3, M, P))
    with pytest.raises(ValueError, match=re.escape(f"Incompatible inner dimensions: A[..., {M}] vs B[..., {M + 1}]")):
        sparse_mm_reduce(A, torch.zeros(M + 1, P))
    with pytest.raises(RuntimeError, match=re.escape("A and B must be on the same device, got cpu and meta")):
        sparse_mm_reduce(A, torch.zeros(M, P, device="meta"))
    with pytest.raises(RuntimeError, match=re.escape("expected A and B to have the same dtype, got torch.float32 and torch.float64")):
        sparse_mm_reduce(A, B.double())
    with pytest.raises(RuntimeError, match=re.escape("unsupported value dtype torch.float16")):
        sparse_mm_reduce(A.to(torch.float16), B.half())
    with pytest.raises(ValueError, match=re.escape("B needs at least one column")):
        sparse_mm_reduce(A, torch.zeros(M, 0))
    assert sparse_mm_reduce(A, B).equal(sparse_mm_reduce(A, B, "amax"))          # (the default reduction)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy oracle of the GPU tests is the torch op, bit for bit


def _oracle_vs_torch(A, B, G, reduce):
    crow, col = A.crow_indices().numpy(), A.col_indices().numpy()
    C, arg = mr.forward(crow, col, mr.to_acc(A.values()), mr.to_acc(B), reduce)
    Cr, gAr, gBr = _torch_op(A, B, G, reduce)
    assert mr.same_bits(torch.from_numpy(C), Cr), reduce
    return arg, gAr, gBr


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_oracle_agrees_with_torch_forward(dtype, reduce):
    lens = [7, 0, 40, 1, 0, 19, 3]
    A = _csr(dtype, torch.int64, seed=3, n=7, m=40, lens=lens)
    B, G = _dense((40, 9), dtype, 8), _dense((7, 9), dtype, 9)
    arg, _, _ = _oracle_vs_torch(A, B, G, reduce)
    assert (arg[[1, 4]] == -1).all() and (arg[[0, 2, 3, 5, 6]] >= 0).all()


@pytest.mark.parametrize("reduce", ["amax", "amin"])
def test_the_oracle_agrees_with_torch_under_ties(reduce):
    """Small-integer operands: dozens of exact ties, and gradients that are exact in float64 — the winners must be the same."""
    lens = [9, 0, 30, 1, 12, 30, 2, 25, 17]
    A = _csr(torch.float64, torch.int64, seed=4, ints=True, n=9, m=30, lens=lens)
    B, G = _dense((30, 8), torch.float64, 11, ints=True), _dense((9, 8), torch.float64, 12, ints=True)
    arg, gAr, gBr = _oracle_vs_torch(A, B, G, reduce)
    crow, col, val = A.crow_indices().numpy(), A.col_indices().numpy(), A.values().numpy()
    prod = val[:, None] * B.numpy()[col]
    ext = np.max if reduce == "amax" else np.min
    ties = sum(int((prod[crow[i]:crow[i + 1]] == ext(prod[crow[i]:crow[i + 1]], axis=0)).sum()) - 8 for i in range(9) if lens[i])
    assert ties >= 24, ties
    dval, _, dB, _ = mr.gradients(crow, col, val, B.numpy(), G.numpy(), arg)
    assert np.array_equal(dval, gAr.numpy()) and np.array_equal(dB, gBr.numpy())
    # ... and the package's CPU path gives those gradients
    _, gA, gB = _ours(A, B, G, reduce)
    assert np.array_equal(dval, gA.values().numpy()) and np.array_equal(dB, gB.numpy())


@pytest.mark.parametrize("reduce", ["amax", "amin"])
def test_special_values(reduce):
    nan, dtype = float("nan"), torch.float32
    crow = torch.tensor([0, 0, 3, 6, 9, 12, 12, 15, 15])
    col = torch.tensor([0, 1, 2] * 5)
    #        row 1: all negative   row 2: NaN value    row 3: NaN in B   row 4: signed zeros  row 6: plain
    val = torch.tensor([-1.0, -2.0, -3.0, 1.0, nan, 2.0, 1.0, 1.0, 1.0, 0.0, -0.0, 0.0, 3.0, -1.0, 2.0], dtype=dtype)
    A = torch.sparse_csr_tensor(crow, col, val, (8, 4))
    B = torch.tensor([[1.0, 2.0], [3.0, 1.0], [2.0, 5.0], [nan, nan]], dtype=dtype)          # (row 3 of B is never gathered)
    Bn = B.clone()
    Bn[1, 0] = nan
    G = _dense((8, 2), dtype, 3, ints=True)             # (integers: the float64 gradients of the oracle are exact in float32 too)
    for Bx in (B, Bn):
        C, gA, gB = _ours(A, Bx, G, reduce)
        Cr, gAr, gBr = _torch_op(A, Bx, G, reduce)
        assert mr.same_bits(C, Cr) and mr.same_bits(gA.values(), gAr) and mr.same_bits(gB, gBr)
        Co, arg = mr.forward(crow.numpy(), col.numpy(), val.numpy(), Bx.numpy(), reduce)
        assert mr.same_bits(torch.from_numpy(Co), C)
        assert (arg[[0, 5, 7]] == -1).all() and (Co[[0, 5, 7]] == 0).all()             # rows without entries: 0, not -inf
        assert np.isnan(Co[2]).all() and (arg[2] == 4).all()                             # the NaN wins over any number
        if Bx is B:
            assert (arg[4] == 9).all() and not np.signbit(Co[4]).any()                   # +0.0 and -0.0 tie: the first stays
            assert (Co[1] < 0).all() if reduce == "amax" else (Co[1] == [-6.0, -15.0]).all()      # absent entries are not zeros
        else:
            assert np.isnan(Co[[1, 3, 4, 6], 0]).all() and (arg[[1, 3, 4, 6], 0] == [1, 7, 10, 13]).all()
        dval, _, dB, _ = mr.gradients(crow.numpy(), col.numpy(), val.numpy(), Bx.numpy(), G.numpy(), arg)
        assert mr.same_bits(torch.from_numpy(dval).float(), gAr) and mr.same_bits(torch.from_numpy(dB).float(), gBr)


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: the fourth header

FAKE = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _addr(k):
    return FAKE + k * 0x100000


def _forward(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), val=_addr(2), B=_addr(3), ldb=64, p=64, op=0,
             C=_addr(4), ldc=64, arg=_addr(5), ldarg=64, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_spmm_reduce(*a.values())


def _backward_values(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), arg=_addr(5), ldarg=64, G=_addr(6), ldg=64,
             B=_addr(3), ldb=64, p=64, dval=_addr(7), device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_spmm_reduce_backward_values(*a.values())


def _backward_dense(lib, **kw):
    a = dict(vtype=0, itype=0, n_rows=40, n_cols=30, nnz=500, ptr=_addr(0), idx=_addr(1), perm=_addr(8), val=_addr(2), arg=_addr(5),
             ldarg=64, G=_addr(6), ldg=64, p=64, dB=_addr(9), lddb=64, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_spmm_reduce_backward_dense(*a.values())


CALLS = [(_forward, ("ptr", "idx", "val", "B", "C", "arg"), ("ldb", "ldc", "ldarg"), ("B", "C")),
         (_backward_values, ("ptr", "idx", "arg", "G", "B", "dval"), ("ldarg", "ldg", "ldb"), ("G", "B")),
         (_backward_dense, ("ptr", "idx", "perm", "val", "arg", "G", "dB"), ("ldarg", "ldg", "lddb"), ("G", "dB"))]


@pytest.mark.parametrize("call,operands,strides,dense", CALLS, ids=["forward", "backward_values", "backward_dense"])
def test_launcher_refusals_on_the_host(call, operands, strides, dense):
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert call(lib) == BAD_ARG
    for vt in (1, 2):
        assert call(lib, vtype=vt) == BAD_ARG
    assert call(lib, itype=1) == BAD_ARG and call(lib, p=1) == BAD_ARG and call(lib, p=33) == BAD_ARG
    for vt in (3, -1):
        assert call(lib, vtype=vt) == BAD_DTYPE
    for it in (2, -1):
        assert call(lib, itype=it) == BAD_DTYPE
    for name in ("n_rows", "n_cols", "nnz"):
        assert call(lib, **{name: -1}) == BAD_ARG, name
    assert call(lib, p=0) == BAD_ARG and call(lib, p=-3) == BAD_ARG
    for name in operands:
        assert call(lib, **{name: None}) == BAD_ARG, name
    for name in strides:                                   # a leading dimension below p
        assert call(lib, **{name: 63}) == BAD_ARG, name
        assert call(lib, **{name: 1 << 40}) == TOO_LARGE, name
    # alignment: whole elements are required (arg: whole int32), 16 bytes are not — such operands reach set_device
    for name in dense:
        assert call(lib, **{name: _addr(3) + 2}) == BAD_ARG, name
        assert call(lib, **{name: _addr(3) + 4}) == BAD_ARG and call(lib, vtype=1, **{name: _addr(3) + 4}) == BAD_ARG, name
    assert call(lib, arg=_addr(5) + 2) == BAD_ARG
    # positions are int32
    assert call(lib, nnz=1 << 31) == TOO_LARGE and call(lib, nnz=(1 << 31) - 1) == BAD_ARG
    assert call(lib, n_rows=1 << 40) == TOO_LARGE and call(lib, n_cols=1 << 40) == TOO_LARGE
    # the refusals do not depend on the device
    assert call(lib, device=0, vtype=7) == BAD_DTYPE and call(lib, device=0, ptr=None) == BAD_ARG
    # nothing to walk is not an error (and touches no device)
    empty = "n_cols" if call is _backward_dense else "n_rows"
    assert call(lib, **{empty: 0}) == OK
    if call is _forward:
        for op in (2, -1):
            assert call(lib, op=op) == BAD_ARG
        assert call(lib, op=1) == BAD_ARG                                              # (amin reaches set_device)
    if call is _backward_values:
        assert call(lib, nnz=0, idx=None, B=None, dval=None) == OK                      # (no entries: nothing to write)


def test_the_geometry_query():
    lib = _backend.load_library()
    r, s, w = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_csr_spmm_reduce_geometry(5, 32, ref(r), ref(s), ref(w)) == BAD_DTYPE
    assert lib.tsgu_csr_spmm_reduce_geometry(0, 0, ref(r), ref(s), ref(w)) == BAD_ARG
    assert lib.tsgu_csr_spmm_reduce_geometry(0, 32, None, ref(s), ref(w)) == BAD_ARG
    src = open(os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "spmm_impl.h")).read()
    stage = int(re.search(r"kStageCap\s*=\s*(\d+)", src).group(1))
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        for p in (1, 3, 32, 33, 64, 130, 256, 1024, 1025):
            rpb, st, width = _backend.spmm_reduce_geometry(dtype, p)
            assert st == stage and 1 <= rpb <= 256 and 256 % rpb == 0 and width >= 1
            assert width * (-(-p // width)) >= p
    # 16-byte lanes when p allows them: 8 lanes of 4 floats cover 32 columns, 32 rows per workgroup
    assert _backend.spmm_reduce_geometry(torch.float32, 32) == (32, stage, 32)
    assert _backend.spmm_reduce_geometry(torch.float32, 1024) == (4, stage, 256)
    with pytest.raises(RuntimeError, match="tsgu_csr_spmm_reduce_geometry failed"):
        _backend.spmm_reduce_geometry(torch.float32, 0)
