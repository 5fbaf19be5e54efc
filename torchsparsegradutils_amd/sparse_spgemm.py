"""``sparse_spgemm`` — the sparse × sparse product ``C = A·B`` with sparsity-preserving gradients: ``torch.sparse.mm(S1, S2)`` whose
output pattern is computed once per pair of input patterns.  The reference has no counterpart.

What the precision matrix ``L·Lᵀ`` of a sparse factor, a Galerkin product ``R·A·P``, the normal equations ``Aᵀ·A`` and a two-hop
adjacency are built with.  ``C``'s pattern is the STRUCTURAL product — (i, j) is stored when some ``A[i,k]`` and ``B[k,j]`` are both
stored; entries that cancel stay stored, as torch keeps them — with ascending columns in every row.

The pattern depends on the two input patterns only.  The symbolic kernels of ``csrc/spgemm.hip`` compute it on the first call
and the plan is kept in A's pattern core, keyed (weakly) by B's: later calls run the numeric kernel alone and return a tensor
on THE SAME index tensors, so that a following ``sparse_mm(C, X)`` or ``sparse_softmax(C, -1)`` finds C's cached plans, and the
backward recognises a gradient on C's pattern by its pointers.  The first call reads the device twice (the sizes of the row
bins, then ``nnz(C)``); the steady state does not synchronise.

Both gradients are evaluated at the operand's stored positions only and come back as sparse tensors on the operand's own index
tensors: ``gradA[i,k] = Σ_t g[i, col_t]·B[k, col_t]`` over the stored entries of ``B[k,:]``, ``gradB[k,j] = Σ_i A[i,k]·g[i,j]`` over the
cached transpose of ``A``.  Every sum — forward and backward — runs in a fixed order without float atomics: two runs give the
same bits.  CPU operands take the torch-op path of ``_cpu.py``: ``torch.sparse.mm`` itself.
"""

from __future__ import annotations

import weakref
from typing import cast

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt
from .sparse_logsumexp import _Operand
from .sparse_softmax import _restrict

__all__ = ["sparse_spgemm", "SparseSpGEMM"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
_UB_MAX = 1 << 30          # a row's upper bound Σ_k nnz(B[k,:]) the sort buffers are addressed for


class _Plan:
    """C's pattern for one pair of input patterns: ``crow`` / ``col`` in the result's index dtype (``indices`` = [row; col] for a
    COO result, ``col`` being its second row), and the row lists of the numeric kernel's bins."""

    __slots__ = ("layout", "shape", "crow", "col", "indices", "nnz", "bins", "__weakref__")

    def tensor(self, values: torch.Tensor) -> torch.Tensor:
        if self.layout == torch.sparse_csr:
            return torch.sparse_csr_tensor(self.crow, self.col, values, self.shape)
        return torch.sparse_coo_tensor(self.indices, values, self.shape, is_coalesced=True)


def _pow2_ceil(x: torch.Tensor) -> torch.Tensor:
    v = (x - 1).clamp_(min=0)
    for s in (1, 2, 4, 8, 16, 32):
        v = v | (v >> s)
    return v + 1


def _binned(measure: torch.Tensor):
    """(bin of every row — 0: no entry, b + 1: bin b of the kernels —, rows sorted by bin as int32, rows per bin on the device)."""
    limits = torch.tensor((0,) + _be.SPGEMM_BIN_LIMITS, dtype=torch.int64, device=measure.device)
    which = torch.bucketize(measure, limits)
    order = torch.argsort(which, stable=True).to(torch.int32)
    return which, order, torch.bincount(which, minlength=limits.numel() + 1)


def _split(order: torch.Tensor, counts):
    """[(bin, rows)] of the bins that have rows; `counts` on the host, counts[0] = rows without entries."""
    out, at = [], counts[0]
    for b, c in enumerate(counts[1:]):
        if c:
            out.append((b, order[at:at + c]))
        at += c
    return out


def _arrays(g: _pt.RowGather):
    """(crow, col) of a stored-order pattern as contiguous arrays of ONE index dtype (a COO pattern's row pointer is int64)."""
    col = g.col.contiguous()
    crow = g.crow
    if crow.dtype != col.dtype:
        key = "crow_" + str(col.dtype)
        crow = g.core.own.get(key)
        if crow is None:
            crow = g.core.own[key] = g.crow.to(col.dtype)
    return crow.contiguous(), col


def _unique_columns(g: _pt.RowGather) -> bool:
    """Whether no row of the pattern holds a column twice (hand-built CSR can); one sort and one host read per pattern."""
    own = g.core.own
    ok = own.get("spgemm_unique_columns")
    if ok is None:
        if g.nnz < 2:
            ok = True
        else:
            key = g.row_indices().to(torch.int64) * max(g.n_cols, 1) + g.col.to(torch.int64)
            key = torch.sort(key).values
            ok = not bool((key[1:] == key[:-1]).any())
        own["spgemm_unique_columns"] = ok
    return cast(bool, ok)


def _build_plan(a: _pt.RowGather, b: _pt.RowGather, layout) -> _Plan:
    n, k, m = a.n_rows, a.n_cols, b.n_cols
    a_crow, a_col = _arrays(a)
    b_crow, b_col = _arrays(b)
    idt, dev = a_col.dtype, a_col.device
    dims = (n, k, m)
    last = len(_be.SPGEMM_BIN_LIMITS)

    ub = _be.spgemm_row_bound(a_crow, a_col, b_crow, n, k)
    which, order, counts = _binned(ub)
    caps = torch.where(which == last + 1, _pow2_ceil(ub).clamp_(min=_be.SPGEMM_SCRATCH_MIN), torch.zeros_like(ub))
    head = torch.cat((counts, caps.sum().reshape(1), ub.max().reshape(1) if n else ub.new_zeros(1))).tolist()      # host read 1 of 2
    counts_h, scratch_len, ub_max = head[:last + 2], head[last + 2], head[last + 3]
    if ub_max >= _UB_MAX:
        raise RuntimeError(f"sparse_spgemm: a row of the product meets {ub_max} entries of B; at most {_UB_MAX - 1} are supported")
    sym = _split(order, counts_h)
    scratch = sptr = None
    if sym and sym[-1][0] == last:
        rows_g = sym[-1][1]
        sptr = torch.zeros(rows_g.numel() + 1, dtype=torch.int64, device=dev)
        sptr[1:] = torch.cumsum(caps[rows_g.long()], 0)
        scratch = torch.empty(scratch_len, dtype=torch.int32, device=dev)

    cnt = torch.zeros(n, dtype=torch.int64, device=dev)
    for bin_, rows in sym:
        _be.spgemm_symbolic(bin_, rows, dims, a_crow, a_col, b_crow, b_col, scratch=scratch, sptr=sptr, cnt=cnt)
    crow64 = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    crow64[1:] = torch.cumsum(cnt, 0)
    _, norder, ncounts = _binned(cnt)
    tail = torch.cat((crow64[-1:], ncounts)).tolist()                                                         # host read 2 of 2
    nnz = tail[0]
    if nnz > torch.iinfo(idt).max:
        raise RuntimeError(f"sparse_spgemm: the product has {nnz} stored entries, which does not fit A's index dtype {idt}")

    plan = _Plan()
    plan.layout, plan.shape, plan.nnz = layout, (n, m), nnz
    plan.crow = crow64.to(idt)
    if layout == torch.sparse_coo:
        plan.indices = torch.empty((2, nnz), dtype=idt, device=dev)
        plan.col = plan.indices[1]
    else:
        plan.indices = None
        plan.col = torch.empty(nnz, dtype=idt, device=dev)
    for bin_, rows in sym:
        _be.spgemm_symbolic(bin_, rows, dims, a_crow, a_col, b_crow, b_col, scratch=scratch, sptr=sptr, c_crow=plan.crow, c_col=plan.col)
    if plan.indices is not None:
        plan.indices[0] = torch.repeat_interleave(torch.arange(n, dtype=idt, device=dev), cnt, output_size=nnz)
    plan.bins = _split(norder, tail[1:])
    return plan


def _plan_for(aop: _Operand, bop: _Operand) -> _Plan:
    plans = aop.plan.core.own.get("spgemm")
    if plans is None:
        plans = aop.plan.core.own["spgemm"] = weakref.WeakKeyDictionary()      # B's pattern core -> plan: dies with either pattern
    plan = plans.get(bop.plan.core)
    if plan is None:
        plan = plans[bop.plan.core] = _build_plan(aop.plan, bop.plan, aop.A.layout)
    return cast(_Plan, plan)


def _numeric(plan: _Plan, a: _pt.RowGather, a_val: torch.Tensor, b: _pt.RowGather, b_val: torch.Tensor) -> torch.Tensor:
    """C's values on the pattern of `plan` for GPU operands on the patterns the plan was built from: the numeric kernel over the
    plan's row bins, nothing else.  (Also what `SparseAMG.refresh` repeats on the plans it keeps, without a cache look-up.)"""
    a_crow, a_col = _arrays(a)
    b_crow, b_col = _arrays(b)
    vals = torch.empty(plan.nnz, dtype=a_val.dtype, device=a_val.device)
    acc = None
    if plan.bins and plan.bins[-1][0] == len(_be.SPGEMM_BIN_LIMITS):
        acc = vals if vals.dtype != torch.bfloat16 else torch.empty(plan.nnz, dtype=torch.float32, device=vals.device)
    dims = (a.n_rows, a.n_cols, b.n_cols)
    for bin_, rows in plan.bins:
        _be.spgemm_numeric(bin_, rows, dims, a_crow, a_col, a_val, b_crow, b_col, b_val, plan.crow, plan.col, vals, acc=acc)
    return vals


def _cpu_plan(C: torch.Tensor, layout, idt) -> _Plan:
    """The pattern of a coalesced COO product on the CPU, in the result's layout and index dtype."""
    plan = _Plan()
    plan.layout, plan.shape, plan.nnz, plan.bins = layout, tuple(C.shape), C._nnz(), []
    idx = C._indices()
    plan.crow = torch._convert_indices_from_coo_to_csr(idx[0].contiguous(), C.size(0), out_int32=idt == torch.int32)
    plan.indices = idx if layout == torch.sparse_coo else None
    plan.col = idx[1] if layout == torch.sparse_coo else idx[1].to(idt)
    return plan


def _coo(op: _Operand, dtype: torch.dtype) -> torch.Tensor:
    """The operand as a coalesced COO tensor of `dtype` (the torch-op path's form)."""
    g = op.plan
    idx = torch.stack((g.row_indices().to(torch.int64), g.col.to(torch.int64)))
    return torch.sparse_coo_tensor(idx, op.values.to(dtype), (g.n_rows, g.n_cols), is_coalesced=True)


class SparseSpGEMM(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_spgemm` (once differentiable).  ``A`` and ``B`` are CSR or coalesced COO; either
    gradient has its operand's layout, index tensors and index dtype."""

    @staticmethod
    def forward(ctx, A, B):
        aop, bop = _Operand(A), _Operand(B)
        a_val, b_val = aop.values.contiguous(), bop.values.contiguous()
        if not _unique_columns(bop.plan):      # (what the forward's plain adds rely on; known after the pattern's first call)
            raise ValueError("sparse_spgemm: a row of B holds a column index more than once")
        if a_val.is_cuda:
            plan = _plan_for(aop, bop)
            vals = _numeric(plan, aop.plan, a_val, bop.plan, b_val)
        else:
            wide = torch.float32 if a_val.dtype == torch.bfloat16 else a_val.dtype
            C = _cpu.spgemm(_coo(aop, wide), _coo(bop, wide))
            plan = _cpu_plan(C, A.layout, aop.plan.col.dtype)
            vals = C._values().to(a_val.dtype)
        ctx.aop, ctx.bop, ctx.plan = aop, bop, plan
        ctx.save_for_backward(a_val, b_val)
        return plan.tensor(vals)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):  # type: ignore[override]
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return None, None
        a_val, b_val = ctx.saved_tensors
        aop, bop, plan = ctx.aop, ctx.bop, ctx.plan
        cop = _Operand(plan.tensor(torch.empty(plan.nnz, dtype=a_val.dtype, device=a_val.device)))
        g = _restrict(cop, grad).reshape(-1).to(a_val.dtype).contiguous()
        ga = gb = None
        if a_val.is_cuda:
            dims = (aop.n_rows, aop.n_cols, bop.n_cols)
            a_crow, a_col = _arrays(aop.plan)
            b_crow, b_col = _arrays(bop.plan)
            if need_a:
                ga = _be.spgemm_grad_a(dims, aop.plan.row_indices().contiguous(), a_col, b_crow, b_col, b_val, plan.crow, plan.col, g)
            if need_b:
                t = aop.plan.transposed
                gb = _be.spgemm_grad_b(dims, bop.plan.row_indices().contiguous(), b_col, t.crow.contiguous(), t.col.contiguous(),
                                       t.perm.contiguous(), a_val, plan.crow, plan.col, g)
        else:
            wide = torch.float32 if a_val.dtype == torch.bfloat16 else a_val.dtype
            idx = torch.stack((cop.plan.row_indices().to(torch.int64), cop.plan.col.to(torch.int64)))
            G = torch.sparse_coo_tensor(idx, g.to(wide), plan.shape, is_coalesced=True)
            ga, gb = _cpu.spgemm_backward(_coo(aop, wide), _coo(bop, wide), G, need_a, need_b)
            ga = None if ga is None else ga.to(a_val.dtype)
            gb = None if gb is None else gb.to(b_val.dtype)
        return (aop.rebuild(ga) if need_a else None), (bop.rebuild(gb) if need_b else None)


def sparse_spgemm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    r"""Sparse × sparse product :math:`C = A B` with sparsity-preserving gradients, as ``torch.sparse.mm(A, B)`` of two sparse
    operands.

    ``A``: ``[n, k]``, ``B``: ``[k, m]``, each sparse COO or CSR (the layouts may differ), float32, float64 or bfloat16 values of one
    dtype, int32 or int64 indices of one dtype, on one device.  Uncoalesced COO is coalesced first.  A ``B`` with a column index
    twice in one row is refused.  Batched operands are not supported.

    Returns a sparse ``[n, m]`` tensor with A's layout and index dtype whose pattern is the structural product (entries that cancel
    to 0.0 stay stored), columns ascending and unique in every row, a COO result coalesced.  The pattern is computed once per pair
    of input patterns; later calls return a tensor on the same index tensors.  bfloat16 is accumulated in float32 and rounded
    once.  Every entry is summed in A's stored order: two runs give the same bits.

    Differentiable once.  ``dL/dA`` and ``dL/dB`` are evaluated at the operands' stored positions only and come back in the operands'
    layouts, on their own index tensors.  The upstream gradient may be sparse on C's pattern, sparse on another pattern (it is
    masked), or dense (it is gathered).
    """
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise TypeError("Both A and B should be instances of torch.Tensor")
    if A.layout not in {torch.sparse_coo, torch.sparse_csr}:
        raise ValueError("A should be in either COO or CSR sparse format")
    if B.layout not in {torch.sparse_coo, torch.sparse_csr}:
        raise ValueError("B should be in either COO or CSR sparse format")
    if A.dim() != 2 or B.dim() != 2:
        raise ValueError("A and B must both be 2D tensors: batched operands are not supported")
    if (A.layout == torch.sparse_coo and A.dense_dim()) or (B.layout == torch.sparse_coo and B.dense_dim()):
        raise ValueError("A and B must both be 2D tensors: hybrid COO operands are not supported")
    if A.size(1) != B.size(0):
        raise ValueError(f"Incompatible inner dimensions: A[..., {A.size(1)}] vs B[{B.size(0)}, ...]")
    if A.device != B.device:
        raise ValueError(f"A and B must be on the same device, got {A.device} and {B.device}")
    if A.dtype != B.dtype:
        raise ValueError(f"expected A and B to have the same dtype, got {A.dtype} and {B.dtype}")
    if A.dtype not in _DTYPES:
        raise ValueError(f"sparse_spgemm: values must be float32, float64 or bfloat16, got {A.dtype}")
    ia = A.col_indices().dtype if A.layout == torch.sparse_csr else A._indices().dtype
    ib = B.col_indices().dtype if B.layout == torch.sparse_csr else B._indices().dtype
    if ia != ib:
        raise ValueError(f"expected A and B to have the same index dtype, got {ia} and {ib}")
    if A.layout == torch.sparse_coo and not A.is_coalesced():
        A = A.coalesce()
    if B.layout == torch.sparse_coo and not B.is_coalesced():
        B = B.coalesce()
    return cast(torch.Tensor, SparseSpGEMM.apply(A, B))
