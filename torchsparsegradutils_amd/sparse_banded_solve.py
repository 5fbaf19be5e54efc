"""``sparse_banded_triangular_solve`` — ``sparse_triangular_solve`` for factors whose selected triangle is a BAND of width at
most 8 (bi-, tri- and pentadiagonal factors, AR(p) / 1-D GMRF ``precision_tril``, spline and line smoothers), solved in
logarithmic depth.

The sync-free sweep behind ``sparse_triangular_solve`` costs one cross-wave hop per dependency level and a band has one level per
row.  A band of width w is a linear recurrence of order w: the rows are cut into chunks, every chunk is reduced to the affine map of
the w solutions entering it, the chain of maps is carried by the same reduce / apply over groups of chunks, and every chunk is
substituted again from its true incoming state (csrc/band_impl.h).  Every dependency between workgroups is a kernel boundary, so
the path has no waits, no error word and can be captured in a graph as it stands.

Same signature, validation, operand layouts, ignored entries, batching and autograd contract as ``sparse_triangular_solve``; the
function is opt-in — ``sparse_triangular_solve`` does not dispatch to it — because its bits differ from the sweep's (both are
within the componentwise bound of a substitution).  The chunk maps are products of the recurrence: as accurate as the recurrence is
stable (factors of diagonally dominant and positive definite operators are), and they can overflow where it grows without bound.
"""

from __future__ import annotations

from typing import cast

import torch

from . import _backend as _be
from . import _ops
from . import _pattern as _pt
from .sparse_solve import _TriOperand

MAX_WIDTH = _be.BAND_MAX_WIDTH


def sparse_banded_triangular_solve(
    A: torch.Tensor,
    B: torch.Tensor,
    upper: bool = True,
    unitriangular: bool = False,
    transpose: bool = False,
) -> torch.Tensor:
    r"""Solve :math:`A x = B` (or :math:`A^\top x = B`) for a sparse triangular ``A`` (COO/CSR, ``(m, m)`` or ``(b, m, m)``, float32 /
    float64) whose selected triangle lies within 8 of the diagonal, and dense ``B``, with sparsity-preserving gradients.  A wider band
    and rows whose columns are not strictly ascending raise ``ValueError``."""
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise ValueError("Both A and B should be instances of torch.Tensor")
    if A.dim() < 2 or B.dim() < 2:
        raise ValueError("Both A and B should be at least 2-dimensional tensors")
    if A.dim() != B.dim() or A.dim() not in (2, 3):
        raise ValueError("A and B must both be 2D or both be 3D tensors")
    if A.layout not in {torch.sparse_coo, torch.sparse_csr}:
        raise ValueError("A should be in either COO or CSR sparse format")
    if B.layout != torch.strided:
        raise ValueError("B must be a dense (strided) tensor")
    if A.shape[-2] != A.shape[-1]:
        raise ValueError("A must be square on its last two dimensions")
    if A.size(-2) != B.size(-2):
        raise ValueError(f"Incompatible inner dimensions: A[..., {A.size(-2)}] vs B[..., {B.size(-2)}]")
    if A.dim() == 3 and A.size(0) != B.size(0):
        raise ValueError("If batched, A and B must have the same batch size")

    return cast(torch.Tensor, SparseBandedTriangularSolve.apply(A, B, upper, unitriangular, transpose))


def _solve(plan: _pt.RowGather, values, rhs, upper: bool, unit: bool, transpose: bool, chunk_rows=None, group_chunks=None):
    """X = op(A)^{-1} rhs on the 2-D plan: A's own arrays in all four modes (no transposed pattern, no permutation is built)."""
    if not rhs.is_cuda:     # CPU operands: the legacy ATen call, as sparse_triangular_solve makes it (_cpu.py)
        from . import _cpu

        return _cpu.sptrsm(plan, values, rhs, upper, unit, transpose)
    width = _pt.band_plan(plan, lower=not upper).width
    if width > MAX_WIDTH:
        raise ValueError(f"sparse_banded_triangular_solve: the band is {width} wide and the widest band served is {MAX_WIDTH}: "
                         "use sparse_triangular_solve")
    if plan.perm is not None:
        values = values.index_select(0, plan.perm.to(torch.int64))
    return _be.csr_band_sptrsm(plan.crow, plan.col, values, rhs, plan.n_rows, width, lower=not upper, unit=unit, transpose=transpose,
                               chunk_rows=chunk_rows, group_chunks=group_chunks)


class SparseBandedTriangularSolve(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_banded_triangular_solve`: ``SparseTriangularSolve`` with the banded kernels."""

    @staticmethod
    def forward(ctx, A, B, upper, unitriangular, transpose):
        ctx.batch_size = B.size()[0] if B.dim() == 3 else None
        ctx.A_shape = A.size()
        ctx.B_shape = B.size()
        ctx.upper = upper
        ctx.unitriangular = unitriangular
        ctx.transpose = transpose
        grad_flag = A.requires_grad or B.requires_grad

        A, B = A.detach(), B.detach()
        if A.device != B.device:
            raise RuntimeError(f"A and B must be on the same device, got {A.device} and {B.device}")
        op = _TriOperand(A)
        rhs = B.reshape(-1, B.size(-1)) if ctx.batch_size is not None else B

        x = _solve(op.plan, op.values, rhs, upper, unitriangular, transpose)

        x.requires_grad = grad_flag
        ctx.op = op
        ctx.save_for_backward(op.values, x.detach())
        if ctx.batch_size is not None:
            x = x.view(ctx.batch_size, ctx.A_shape[-2], ctx.B_shape[-1])
        return x

    @staticmethod
    def backward(ctx, grad):  # type: ignore[override]
        if ctx.batch_size is not None:
            grad = grad.reshape(-1, grad.size(-1))
        values, x = ctx.saved_tensors
        op: _TriOperand = ctx.op
        plan = op.plan

        # gradB = op(A)^{-T} grad: the same kernels in the other direction
        gradB = _solve(plan, values, grad, ctx.upper, ctx.unitriangular, not ctx.transpose)

        if ctx.unitriangular is True and plan.has_diagonal:
            raise ValueError("First input should be strictly triangular (i.e. unit diagonals is implicit)")

        # gradA[k] = -<gradB[i,:], x[j,:]>, roles swapped for the transposed solve
        gvals = _ops.sddmm(plan, gradB, x, alpha=-1.0, swap_roles=bool(ctx.transpose))
        if plan.perm is not None:
            out = torch.empty_like(gvals)
            out[plan.perm] = gvals
            gvals = out
        gradA = op.rebuild(gvals)
        if ctx.batch_size is not None:
            gradB = gradB.view(ctx.B_shape)
        return gradA, gradB, None, None, None
