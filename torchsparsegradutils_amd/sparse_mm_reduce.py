"""``sparse_mm_reduce`` — the sparse × dense product with the sum over a row's stored entries replaced by a maximum, a minimum or
a mean: ``torch.sparse.mm(A, B, reduce)``, which torch offers for CSR operands on the CPU only.

What a max- / min- / mean-aggregating message-passing layer calls (GraphSAGE-pool, PointNet-style set pooling, GCN's mean
aggregator, morphological filters on a lattice).  The reference has no counterpart.

``amax`` / ``amin`` run the kernels of ``csrc/mm_reduce.hip``: the forward is the row-group gather of ``sparse_mm``'s plan-free
kernel with a compare-and-select per column in place of the sum, and it writes, next to ``C``, the stored position of every
winner (``arg``).  Both gradients flow through the winner only and are gathers too: one pass over the rows for the values, one
over the cached transposed pattern for ``B``.  Saved for the backward: the values, ``B`` and ``arg``, which is ``n·p`` int32 — as
many bytes as a float32 ``C``.

``mean`` is ``sparse_mm(A, B)`` followed by one row scaling, so it runs on whichever kernel family ``sparse_mm`` chooses for the
pattern, and ``sum`` is ``sparse_mm`` itself.  CPU operands take the torch-op path of ``_cpu.py``: torch's own op, which differs
from the kernels in two corners — of two NaN candidates in one row and column it keeps the last (the kernels the first; the
value is NaN either way), and it compares bfloat16 candidates after rounding them (the kernels compare the exact float32
products).
"""

from __future__ import annotations

from typing import cast

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt
from .sparse_matmul import _Operand, sparse_mm

__all__ = ["sparse_mm_reduce", "SparseMMReduce"]

REDUCTIONS = ("sum", "mean", "amax", "amin")
_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class SparseMMReduce(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_mm_reduce` for ``amax`` and ``amin`` (once differentiable).  ``A`` is CSR or coalesced
    COO; the gradient of ``A`` has A's layout, index tensors and index dtype."""

    @staticmethod
    def forward(ctx, A, B, reduce):
        grad_flag = A.requires_grad or B.requires_grad
        A, B = A.detach(), B.detach()
        op = _Operand(A)
        flat = _pt.flat_of(op.plan)
        p = B.size(-1)
        values = op.values.reshape(-1).contiguous()
        Bk = _be.rowmajor(B.reshape(-1, p))
        crow, col = flat.crow.contiguous(), flat.col.contiguous()
        if Bk.is_cuda:
            C, arg = _be.csr_spmm_reduce(crow, col, values, Bk, flat.n_rows, flat.n_cols, reduce)
        else:
            C, arg = _cpu.mm_reduce(crow, col, values, Bk, (flat.n_rows, flat.n_cols), reduce), None
        ctx.op, ctx.reduce, ctx.B_shape = op, reduce, B.shape
        ctx.save_for_backward(values, Bk, arg)
        C = C.view(B.shape[:-2] + (A.size(-2), p))
        C.requires_grad_(grad_flag)
        return C

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):  # type: ignore[override]
        values, Bk, arg = ctx.saved_tensors
        op: _Operand = ctx.op
        flat = _pt.flat_of(op.plan)
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        G = _be.rowmajor(grad.reshape(-1, grad.size(-1)))
        crow, col = flat.crow.contiguous(), flat.col.contiguous()
        gvals = gradB = None
        if G.is_cuda:
            if need_a:
                gvals = _be.csr_spmm_reduce_backward_values(crow, col, arg, G, Bk, flat.n_rows, flat.n_cols)
            if need_b:
                t = flat.transposed
                gradB = _be.csr_spmm_reduce_backward_dense(t.crow, t.col, t.perm, values, arg, G, flat.n_rows, flat.n_cols)
        else:
            gvals, gradB = _cpu.mm_reduce_backward(crow, col, values, Bk, (flat.n_rows, flat.n_cols), ctx.reduce, G, need_a, need_b)
        gradA = op.rebuild(gvals.view(op.values.shape)) if need_a else None
        return gradA, (gradB.view(ctx.B_shape) if need_b else None), None


def _row_count(A: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Stored entries of every row of (coalesced) ``A`` as ``dtype``, shaped to divide ``A·B`` — rows without entries count 1,
    their sum is 0 already.  Cached with the pattern."""
    op = _Operand(A.detach())
    own = op.plan.core.own
    key = "row_count_" + str(dtype)
    cnt = own.get(key)
    if cnt is None:
        crow = op.plan.crow
        cnt = (crow[..., 1:] - crow[..., :-1]).clamp_(min=1).to(dtype)
        cnt = own[key] = cnt.reshape(A.shape[:-1]).unsqueeze(-1)
    return cast(torch.Tensor, cnt)


def sparse_mm_reduce(A: torch.Tensor, B: torch.Tensor, reduce: str = "amax") -> torch.Tensor:
    r"""Sparse–dense product with a reduction over the stored entries of every row of ``A``:
    ``C[i,k] = reduce_e val[e]·B[col[e],k]`` — the semantics of ``torch.sparse.mm(A_csr, B, reduce)`` on the CPU.

    ``A``: sparse COO or CSR, ``(n, m)`` or ``(b, n, m)``, float32, float64 or bfloat16 values, int32 or int64 indices; ``B``: dense
    ``(m, p)`` or ``(b, m, p)`` of A's dtype on A's device (any strided view; copied when its column stride is not 1).  Returns
    dense ``(n, p)`` / ``(b, n, p)``.  An un-coalesced COO ``A`` is coalesced first: duplicates are ONE matrix entry, their sum is
    the candidate, and the gradient reaches every duplicate.

    ``reduce``:

    * ``"amax"`` / ``"amin"``: only stored entries are candidates (an absent entry is not a zero); a row without stored entries
      gives 0 and no gradient.  Of equal candidates the one stored first wins (``+0.0`` and ``-0.0`` are equal); a NaN candidate
      wins over any number, and the first NaN stays.  The product is formed and compared in float32 for float32 and bfloat16
      (rounded once when stored), in float64 for float64.  The gradients flow through the winner only.  The backward keeps the
      winners' positions: ``n·p`` int32 besides the values and ``B``.
    * ``"mean"``: ``sparse_mm(A, B)`` divided by the number of stored entries of each row (rows without entries stay 0; bfloat16
      is divided in float32 and rounded once more); the backward is ``sparse_mm``'s on ``G / count``.
    * ``"sum"``: ``sparse_mm(A, B)``.

    Differentiable once.  ``dL/dA`` comes back in A's layout, on A's own index tensors, with its index dtype.
    """
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise ValueError("Both A and B should be instances of torch.Tensor")
    if reduce not in REDUCTIONS:
        raise ValueError(f"reduce must be one of 'sum', 'mean', 'amax' or 'amin', got {reduce!r}")
    if A.dim() < 2 or B.dim() < 2:
        raise ValueError("Both A and B should be at least 2-dimensional tensors")
    if A.dim() != B.dim() or A.dim() not in (2, 3):
        raise ValueError("A and B must both be 2D or both be 3D tensors")
    if A.layout not in {torch.sparse_coo, torch.sparse_csr}:
        raise ValueError("A should be in either COO or CSR sparse format")
    if B.layout != torch.strided:
        raise ValueError("B must be a dense (strided) tensor")
    if A.dim() == 3 and A.size(0) != B.size(0):
        raise ValueError("If batched, A and B must have the same batch size")
    if A.size(-1) != B.size(-2):
        raise ValueError(f"Incompatible inner dimensions: A[..., {A.size(-1)}] vs B[..., {B.size(-2)}]")
    if A.device != B.device:
        raise RuntimeError(f"A and B must be on the same device, got {A.device} and {B.device}")
    if A.dtype != B.dtype:
        raise RuntimeError(f"expected A and B to have the same dtype, got {A.dtype} and {B.dtype}")
    if A.dtype not in _DTYPES:
        raise RuntimeError(f"torchsparsegradutils_amd: unsupported value dtype {A.dtype}")
    if B.size(-1) < 1:
        raise ValueError("B needs at least one column")

    if reduce == "sum":
        return sparse_mm(A, B)
    if A.layout == torch.sparse_coo and not A.is_coalesced():
        A = A.coalesce()
    if reduce == "mean":
        C = sparse_mm(A, B)
        if C.dtype == torch.bfloat16:
            return (C.float() / _row_count(A, torch.float32)).to(torch.bfloat16)
        return C / _row_count(A, C.dtype)
    return cast(torch.Tensor, SparseMMReduce.apply(A, B, reduce))
