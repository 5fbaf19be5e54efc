"""Softmax and log-softmax over the stored entries of a sparse matrix, along rows or columns.

The normalising form of :func:`sparse_logsumexp` with ``include_zeros=False``: semantics of ``torch.sparse.softmax`` /
``torch.sparse.log_softmax`` (absent entries are −inf, not zero), for COO, CSR and CSC, ``[r, c]`` or batched ``[b, r, c]``.
The reference has no counterpart, and torch offers the operation for COO only.

The groups are those of the log-sum-exp: the rows of a CSR / coalesced-COO matrix are the segments of its own ``crow``, its
columns those of the cached transpose (values read and results written through its ``perm``), a CSC matrix is the same with
the roles exchanged; a batched input runs item by item on its slice of the block-diagonal pattern.  GPU operands run the fused kernels of
``csrc/softmax.hip`` (one read and one write per entry); CPU operands the torch-op path of ``_cpu.py``.

The result is a sparse tensor on the input's own index tensors — nothing is copied or rebuilt, so a following
``sparse_mm(out, X)`` finds the pattern's cached plans.  Autograd is first order only; the gradient is sparse on the same
index tensors: ``y·(g − Σ_group g·y)``, or ``g − exp(y)·Σ_group g`` for the log form.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from .sparse_logsumexp import _check_input, _Operand

__all__ = ["sparse_softmax", "sparse_log_softmax"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


def _crossing(ptr: torch.Tensor, R: int) -> bool:
    """Whether a group of `ptr` crosses a boundary between the kernels' ranges of R entries: only then their merge and fix-up
    launches are needed."""
    p = ptr.to(torch.int64)
    lo, hi = p[:-1], p[1:]
    return bool(((hi > lo) & (torch.div(lo, R, rounding_mode="floor") != torch.div(hi - 1, R, rounding_mode="floor"))).any())


def _segments(op: _Operand, kind: str, dtype: torch.dtype):
    """[(ptr, perm, groups, first entry, end, crossing)] of the 'row' or 'col' direction: one launch each.  A 2-D input is one
    segment — the pattern's own crow, or its cached transpose with the perm into the value array.  A batched input is one per
    item (its slice of the block-diagonal pattern, rebased to start at entry 0), so that an item's result does not depend on
    where it lies in the batch: the same bits as the item run alone.  Cached with the pattern, per range length."""
    h = op.plan if (kind == "row") == op.rows_first else op.plan.transposed
    R = _be.segment_softmax_range(dtype) if h.crow.is_cuda else 0
    own, key = h.core.own, f"softmax_segments{R}"
    seg = own.get(key)
    if seg is None:
        b = op.batch or 1
        if op.batch is None:
            items = [(h.crow, h.perm, h.n_rows, 0, h.nnz)]
        else:
            per = h.n_rows // b
            offs = h.crow[::per].tolist() if per else [0] * (b + 1)
            items = [((h.crow[i * per:(i + 1) * per + 1] - offs[i]).contiguous(),
                      None if h.perm is None else (h.perm[offs[i]:offs[i + 1]] - offs[i]).contiguous(), per, offs[i], offs[i + 1])
                     for i in range(b)]
        seg = own[key] = [it + (bool(R) and _crossing(it[0], R),) for it in items]
    return seg


def _positions(op: _Operand):
    """(row, column) of every stored entry in the block-diagonal numbering of the operand's pattern."""
    g = op.plan
    first, second = g.row_indices().reshape(-1).to(torch.int64), g.col.reshape(-1).to(torch.int64)
    return (first, second) if op.rows_first else (second, first)


def _restrict(op: _Operand, grad: torch.Tensor) -> torch.Tensor:
    """The upstream gradient's values at the stored positions of the output, in stored order, never through a dense copy of a
    sparse gradient."""
    A = op.A
    if grad.layout == A.layout:
        if grad.layout == torch.sparse_coo and not grad.is_coalesced():
            grad = grad.coalesce()
        if grad.layout == torch.sparse_csr:
            mine, theirs, gv = (A.crow_indices(), A.col_indices()), (grad.crow_indices(), grad.col_indices()), grad.values()
        elif grad.layout == torch.sparse_csc:
            mine, theirs, gv = (A.ccol_indices(), A.row_indices()), (grad.ccol_indices(), grad.row_indices()), grad.values()
        else:
            mine, theirs, gv = (A._indices(),), (grad._indices(),), grad._values()
        if all(a.shape == b.shape and a.dtype == b.dtype and
               ((a.data_ptr() == b.data_ptr() and a.stride() == b.stride()) or torch.equal(a, b)) for a, b in zip(mine, theirs)):
            return gv
    b, n, m = op.batch or 1, op.n_rows, op.n_cols
    r, c = _positions(op)
    if grad.layout == torch.strided:     # gathered at the stored positions
        return grad.reshape(b * n, m)[r, c - torch.div(r, n, rounding_mode="floor") * m]
    # a sparse gradient on another pattern: masked by a search of the pattern's positions among its (sorted) ones
    G = (grad if grad.layout == torch.sparse_coo else grad.to_sparse()).coalesce()
    gi, gv = G._indices().to(torch.int64), G._values()
    if gi.size(0) == 3:
        gkey = (gi[0] * n + gi[1]) * (b * m) + gi[0] * m + gi[2]
    else:
        gkey = gi[0] * (b * m) + gi[1]
    key = r * (b * m) + c
    if gkey.numel() == 0:
        return torch.zeros(key.numel(), dtype=gv.dtype, device=gv.device)
    pos = torch.searchsorted(gkey, key).clamp_(max=gkey.numel() - 1)
    return torch.where(gkey[pos] == key, gv[pos], torch.zeros((), dtype=gv.dtype, device=gv.device))


class SparseSoftmax(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_softmax` / :func:`sparse_log_softmax` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, op, kind, log_form, dtype):
        val = op.values.reshape(-1)
        if dtype is not None and dtype != val.dtype:
            val = val.to(dtype)
        y = torch.empty_like(val)
        for ptr, perm, n, lo, hi, crossing in _segments(op, kind, val.dtype):
            if val.is_cuda:
                _be.segment_softmax(ptr, perm, val[lo:hi], n, log_form, crossing, out=y[lo:hi])
            else:
                y[lo:hi] = _cpu.segment_softmax(ptr, perm, val[lo:hi], n, log_form)
        ctx.op, ctx.kind, ctx.log_form, ctx.in_dtype = op, kind, log_form, op.values.dtype
        ctx.save_for_backward(y)
        return op.rebuild(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        (y,) = ctx.saved_tensors
        op: _Operand = ctx.op
        g = _restrict(op, grad).reshape(-1).to(y.dtype).contiguous()
        gin = torch.empty_like(y)
        for ptr, perm, n, lo, hi, crossing in _segments(op, ctx.kind, y.dtype):
            if y.is_cuda:
                _be.segment_softmax_backward(ptr, perm, y[lo:hi], g[lo:hi], n, ctx.log_form, crossing, out=gin[lo:hi])
            else:
                gin[lo:hi] = _cpu.segment_softmax_backward(ptr, perm, y[lo:hi], g[lo:hi], n, ctx.log_form)
        return op.rebuild(gin.to(ctx.in_dtype)), None, None, None, None


def _apply(name: str, input: torch.Tensor, dim: int, dtype: Optional[torch.dtype], log_form: bool) -> torch.Tensor:
    _check_input(input, name)
    if not isinstance(dim, int) or isinstance(dim, bool):
        raise TypeError(f"{name}: dim must be an int, got {type(dim).__name__}")
    if not -input.ndim <= dim < input.ndim:
        raise IndexError(
            f"Dimension out of range (expected to be in range of [{-input.ndim}, {input.ndim - 1}], but got {dim})")
    d = dim % input.ndim
    if input.ndim == 3 and d == 0:
        raise NotImplementedError("Cannot reduce the batch dimension (0) of a batched 3-D sparse tensor.")
    if dtype is not None and dtype not in _DTYPES:
        raise TypeError(f"{name}: dtype must be torch.float32, torch.float64 or torch.bfloat16, got {dtype}")
    if (dtype or input.dtype) not in _DTYPES:
        raise TypeError(f"{name}: values must be float32, float64 or bfloat16, got {input.dtype}")
    op = _Operand(input)
    return SparseSoftmax.apply(op.A, op, "row" if d == input.ndim - 1 else "col", log_form, dtype)


def sparse_softmax(input: torch.Tensor, dim: int, *, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    r"""Softmax over the stored entries of a sparse COO / CSR / CSC tensor along ``dim``, as :func:`torch.sparse.softmax`: the
    entries of every row (``dim=-1``) or column (``dim=-2``) are normalised among themselves, absent entries do not take part,
    and a row or column without entries produces nothing.

    ``input`` is ``[r, c]`` or batched ``[b, r, c]`` (the batch axis cannot be normalised over) with float32, float64 or
    bfloat16 values (bfloat16 is computed in float32 and rounded once) and int32 or int64 indices; ``dtype`` casts the values
    first.  Uncoalesced COO is coalesced first.  The result has the input's layout and shape and carries its index tensors
    themselves.  A group with a NaN, or with nothing but ``-inf``, is NaN; ``-inf`` beside finite values gives 0.
    Differentiable once; the gradient is sparse on the same index tensors.
    """
    return _apply("sparse_softmax", input, dim, dtype, False)


def sparse_log_softmax(input: torch.Tensor, dim: int, *, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    r"""Logarithm of :func:`sparse_softmax` (as :func:`torch.sparse.log_softmax`), computed as ``(v − max) − log Σ exp(v − max)``
    over the stored entries of every row or column; ``-inf`` beside finite values stays ``-inf``.  Same inputs, output and
    gradient conventions as :func:`sparse_softmax`."""
    return _apply("sparse_log_softmax", input, dim, dtype, True)
