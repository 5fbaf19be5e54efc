"""Sparse log-sum-exp along rows, columns or whole matrices (reference ``torchsparsegradutils/sparse_logsumexp.py:246-496``).

Every reduction is a segmented one over a cached row-gather pattern (``_pattern``): the rows of a CSR / coalesced-COO
matrix are the segments of its own ``crow``, its columns those of the cached transpose (with a ``perm`` into the value
array), a CSC matrix is the same with the roles exchanged, and a batched input is one block-diagonal pattern.  A whole
matrix (or batch item) is one segment.  GPU operands run the HIP kernels of ``csrc/logsumexp.hip``; CPU operands the
torch-op path of ``_cpu.py``.

Autograd is first order only: the gradient of the stored values is ``Σ_dir g_dir[group] · exp(v − lse_dir[group])`` over
the reduced directions, returned as a sparse tensor with the input's layout and its own index tensors.
"""

from __future__ import annotations

from typing import Sequence, Union

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt

__all__ = ["sparse_logsumexp", "sparse_bidir_logsumexp"]

_SUPPORTED = {torch.sparse_coo, torch.sparse_csr, torch.sparse_csc}


class _Operand:
    """The input as the kernels see it: its stored-order pattern ``plan`` (groups = rows, or columns for CSC), the value
    array, and how to hand a value-shaped gradient back in the input's layout."""

    __slots__ = ("A", "plan", "values", "rows_first", "batch", "n_rows", "n_cols")

    def __init__(self, A: torch.Tensor):
        if A.layout == torch.sparse_coo and not A.is_coalesced():
            A = A.coalesce()  # duplicates are summed first, as the reference does (differentiable)
        self.A = A
        self.batch = A.size(0) if A.dim() == 3 else None
        self.n_rows, self.n_cols = A.size(-2), A.size(-1)
        d = A.detach()
        if A.layout == torch.sparse_csr:
            g, self.rows_first = _pt.from_csr(d), True
            self.values = d.values()
        elif A.layout == torch.sparse_csc:
            g, self.rows_first = _pt.from_csc(d), False
            self.values = d.values()
        elif self.batch is not None:
            g, self.rows_first = _pt.from_coo_batched(d._indices(), d.shape), True
            self.values = d._values()
        else:
            g, self.rows_first = _pt.from_coo_2d(d._indices(), d.shape, coalesced=True), True
            self.values = d._values()
        self.plan = _pt.flat_of(g) if g.batch is not None else g

    def groups(self, kind: str):
        """(ptr, perm, n_groups, groups per item, axis length) of one reduction: 'row' (one value per row), 'col' (one value
        per column) or 'all' (one value per matrix / batch item)."""
        b = self.batch or 1
        g = self.plan
        if kind == "all":
            own = g.core.own
            items = own.get("lse_items")
            if items is None:
                items = own["lse_items"] = g.crow[:: g.n_rows // b].contiguous() if g.n_rows else \
                    torch.zeros(b + 1, dtype=g.crow.dtype, device=g.crow.device)
            return items, None, b, 1, self.n_rows * self.n_cols
        own_dir = (kind == "row") == self.rows_first
        h = g if own_dir else g.transposed
        per = self.n_rows if kind == "row" else self.n_cols
        axis = self.n_cols if kind == "row" else self.n_rows
        return h.crow, h.perm, b * per, per, axis

    def rebuild(self, grad_values: torch.Tensor) -> torch.Tensor:
        A = self.A
        gv = grad_values.view(self.values.shape)
        if A.layout == torch.sparse_csr:
            return torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), gv, A.shape)
        if A.layout == torch.sparse_csc:
            return torch.sparse_csc_tensor(A.ccol_indices(), A.row_indices(), gv, A.shape)
        return torch.sparse_coo_tensor(A._indices(), gv, A.shape, is_coalesced=True)


def _forward(op: _Operand, kinds, include_zeros: bool, stride: int) -> torch.Tensor:
    """Buffer (len(kinds), items, stride): direction d's groups of item i at [d, i, :per], -inf beyond."""
    b = op.batch or 1
    val = op.values.reshape(-1)
    out = torch.empty((len(kinds), b, stride), dtype=val.dtype, device=val.device)
    ws = None
    for d, kind in enumerate(kinds):
        ptr, perm, n, per, axis = op.groups(kind)
        if val.is_cuda:
            if ws is None:
                ws = torch.empty(_be.segment_logsumexp_workspace_bytes(val.dtype, val.numel()), dtype=torch.uint8,
                                 device=val.device)
            _be.segment_logsumexp(ptr, perm, val, out[d], n, val.numel(), include_zeros, axis, per, stride, ws)
        else:
            out[d].fill_(float("-inf"))
            out[d, :, :per] = _cpu.segment_logsumexp(ptr, perm, val, n, include_zeros, axis).view(b, per)
    return out


class SparseLogSumExp(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_logsumexp` / :func:`sparse_bidir_logsumexp` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, op, kinds, include_zeros, stride):
        out = _forward(op, kinds, include_zeros, stride)
        ctx.op, ctx.kinds = op, kinds
        ctx.save_for_backward(op.values, out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        values, out = ctx.saved_tensors
        op: _Operand = ctx.op
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        prim = sec = None  # (ptr or idx, g, lse, n_groups)
        for d, kind in enumerate(ctx.kinds):
            ptr, _, n, per, _ = op.groups(kind)
            g = grad[d, :, :per].reshape(-1).contiguous().to(values.dtype)
            lse = out[d, :, :per].reshape(-1).contiguous()
            if kind == "all" or (kind == "row") == op.rows_first:
                prim = (ptr if kind == "all" else op.plan.crow, g, lse, n)
            else:
                sec = (op.plan.col, g, lse, n)
        val = values.reshape(-1)
        p_ptr, p_g, p_lse, p_n = prim if prim is not None else (None, None, None, 0)
        s_idx, s_g, s_lse, _ = sec if sec is not None else (None, None, None, 0)
        if val.is_cuda:
            gv = _be.segment_logsumexp_backward(val, p_ptr, p_g, p_lse, s_idx, s_g, s_lse, p_n)
        else:
            gv = _cpu.segment_logsumexp_backward(val, p_ptr, p_g, p_lse, s_idx, s_g, s_lse)
        return op.rebuild(gv), None, None, None, None


def _check_input(input: torch.Tensor, name: str) -> None:
    if input.ndim not in (2, 3):
        raise NotImplementedError(f"{name} supports 2-D or batched 3-D sparse tensors, got ndim={input.ndim}.")
    if input.layout not in _SUPPORTED:
        raise NotImplementedError(f"{name} does not support layout {input.layout}. Supported: {_SUPPORTED}.")
    if input.dense_dim() != 0:
        raise ValueError(f"{name} requires a sparse tensor with zero dense dimensions.")


def sparse_logsumexp(input: torch.Tensor, dim: Union[int, Sequence[int]], keepdim: bool = False,
                     include_zeros: bool = True) -> torch.Tensor:
    r"""Log-sum-exp of a sparse COO / CSR / CSC tensor along ``dim``, as :func:`torch.logsumexp` on ``input.to_dense()``
    when ``include_zeros`` (every absent entry is an ``exp(0)`` term), or over the stored values only when not.

    ``input`` is ``[r, c]`` or batched ``[b, r, c]`` (the batch axis cannot be reduced); ``dim`` an int or a sequence,
    negatives allowed; output shape and ``keepdim`` as :func:`torch.logsumexp`.  Uncoalesced COO is coalesced first
    (duplicates summed); duplicate CSR / CSC indices count as separate terms.  A group without values or zeros gives
    ``-inf``, one with ``+inf`` gives ``+inf``, one with NaN gives NaN.  Differentiable once in the stored values.
    """
    _check_input(input, "sparse_logsumexp")
    dims_list = [dim] if isinstance(dim, int) else list(dim)
    if not dims_list:
        raise RuntimeError("sparse_logsumexp: dim must not be an empty sequence.")
    for d in dims_list:
        if not -input.ndim <= d < input.ndim:
            raise IndexError(
                f"Dimension out of range (expected to be in range of [{-input.ndim}, {input.ndim - 1}], but got {d})")
    normalised = [d % input.ndim for d in dims_list]
    if len(set(normalised)) != len(normalised):
        raise RuntimeError("sparse_logsumexp: dim contains a repeated dimension.")
    dims = sorted(normalised)
    batched = input.ndim == 3
    if batched and 0 in dims:
        raise NotImplementedError("Cannot reduce the batch dimension (0) of a batched 3-D sparse tensor.")
    local = [d - 1 for d in dims] if batched else dims

    op = _Operand(input)
    b, r, c = op.batch or 1, op.n_rows, op.n_cols
    if local == [0, 1]:
        out = SparseLogSumExp.apply(op.A, op, ("all",), include_zeros, 1)
        res = out.view(b) if batched else out.view(())
        if keepdim:
            res = res.view(b, 1, 1) if batched else res.view(1, 1)
        return res
    kind, per = ("row", r) if local == [1] else ("col", c)
    out = SparseLogSumExp.apply(op.A, op, (kind,), include_zeros, per)
    res = out.view(b, per) if batched else out.view(per)
    if keepdim:
        res = res.unsqueeze(dims[0])
    return res


def _nested_supported() -> bool:
    parts = torch.__version__.split("+")[0].split(".")
    try:
        return (int(parts[0]), int(parts[1])) >= (2, 4)
    except (IndexError, ValueError):
        return True


def sparse_bidir_logsumexp(input: torch.Tensor, keepdim: bool = False, include_zeros: bool = True,
                           output_layout: str = "tuple"):
    r"""Column- and row-wise log-sum-exp of a sparse tensor: ``(col_lse, row_lse)`` — the ``dim=0`` and ``dim=1`` reductions
    (batched: ``dim=1`` and ``dim=2``), bit for bit equal to two :func:`sparse_logsumexp` calls.

    ``output_layout="padded"`` returns the one ``(2, G)`` / ``(2, b, G)`` buffer both live in (``G = max(r, c)``, ``-inf``
    padding; ``"tuple"`` returns views into it); ``"nested"`` a nested tensor of the two.  ``keepdim`` needs ``"tuple"``.
    """
    _check_input(input, "sparse_bidir_logsumexp")
    if output_layout not in ("tuple", "padded", "nested"):
        raise ValueError(
            f"sparse_bidir_logsumexp: unknown output_layout {output_layout!r}. Expected one of 'tuple', 'padded', 'nested'.")
    if keepdim and output_layout != "tuple":
        raise ValueError("sparse_bidir_logsumexp: keepdim is only supported with output_layout='tuple'.")
    if output_layout == "nested" and not _nested_supported():
        raise NotImplementedError("PyTorch version is too old for nested tensors")

    op = _Operand(input)
    batched = op.batch is not None
    b, r, c = op.batch or 1, op.n_rows, op.n_cols
    G = max(r, c)
    out = SparseLogSumExp.apply(op.A, op, ("col", "row"), include_zeros, G)
    padded = out if batched else out.view(2, G)
    if batched:
        col_lse, row_lse = padded[0, :, :c], padded[1, :, :r]
    else:
        col_lse, row_lse = padded[0, :c], padded[1, :r]
    if output_layout == "padded":
        return padded
    if output_layout == "nested":
        return torch.nested.as_nested_tensor([col_lse, row_lse])
    if keepdim:
        col_ax, row_ax = (1, 2) if batched else (0, 1)
        col_lse, row_lse = col_lse.unsqueeze(col_ax), row_lse.unsqueeze(row_ax)
    return col_lse, row_lse
