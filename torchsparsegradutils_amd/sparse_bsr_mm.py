"""``sparse_bsr_mm`` — the product of a block-sparse (``torch.sparse_bsr``) matrix with a dense one, on the matrix cores.

BSR is the layout of block-pruned weights, block-sparse attention masks and multi-dof FEM / channel-coupled stencil matrices, and
the one sparse layout that maps onto MFMA: a stored block is a small dense matrix, so a block row's product is a GEMM whose K runs
over the row's blocks.  Stock torch serves it through Triton on the GPU (a path this package does not take), and on the CPU refuses
non-square blocks and bfloat16.  The reference has no counterpart.

The kernels are those of ``csrc/bsr_impl.h`` behind ``include/tsgu_hip_bsr.h``: the forward ``A·B``, the block SDDMM that writes
the gradient of every stored block, and the transposed product ``Aᵀ·G`` over the cached transposed block pattern.  The block
pattern ``(crow, col)`` is a CSR pattern of the ``(n / bh) × (m / bw)`` block matrix and goes through the same pattern cache as
every other operand.  CPU operands take the torch-op path of ``_cpu.py`` (gather, ``torch.bmm``, ``index_add_``).
"""

from __future__ import annotations

from typing import cast

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt

__all__ = ["sparse_bsr_mm", "SparseBSRMatMul"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class SparseBSRMatMul(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_bsr_mm` (once differentiable).  The gradient of ``A`` is a BSR tensor on A's own
    ``crow_indices()`` / ``col_indices()`` tensors with A's index dtype."""

    @staticmethod
    def forward(ctx, A, B):
        grad_flag = A.requires_grad or B.requires_grad
        A, B = A.detach(), B.detach()
        plan = _pt.from_bsr(A)
        flat = _pt.flat_of(plan)
        values = A.values()
        bh, bw = values.shape[-2:]
        p = B.size(-1)
        blocks = values.reshape(-1, bh, bw).contiguous()
        Bk = _be.rowmajor(B.reshape(-1, p))
        if Bk.is_cuda:
            C = _be.bsr_spmm(flat.crow.contiguous(), flat.col.contiguous(), blocks, Bk, flat.n_rows, flat.n_cols)
        else:
            C = _cpu.bsr_mm(flat, blocks, Bk)
        ctx.plan, ctx.A_shape, ctx.B_shape, ctx.values_shape = plan, A.shape, B.shape, values.shape
        ctx.save_for_backward(blocks, Bk)
        C = C.view(B.shape[:-2] + (A.size(-2), p))
        C.requires_grad_(grad_flag)
        return C

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):  # type: ignore[override]
        blocks, Bk = ctx.saved_tensors
        plan: _pt.RowGather = ctx.plan
        flat = _pt.flat_of(plan)
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        G = _be.rowmajor(grad.reshape(-1, grad.size(-1)))
        bh, bw = blocks.shape[-2:]
        dblocks = gradB = None
        if G.is_cuda:
            if need_a:
                dblocks = _be.bsr_sddmm(flat.crow.contiguous(), flat.col.contiguous(), G, Bk, flat.n_rows, flat.n_cols, bh, bw)
            if need_b:
                t = flat.transposed
                gradB = _be.bsr_spmm_t(t.crow, t.col, t.perm, blocks, G, flat.n_rows, flat.n_cols)
        else:
            dblocks, gradB = _cpu.bsr_mm_backward(flat, blocks, Bk, G, need_a, need_b)
        gradA = None
        if need_a:
            gradA = torch.sparse_bsr_tensor(plan.crow, plan.col, dblocks.view(ctx.values_shape), ctx.A_shape)
        return gradA, (gradB.view(ctx.B_shape) if need_b else None)


def sparse_bsr_mm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    r"""Block-sparse × dense product ``C = A·B`` for a ``torch.sparse_bsr`` operand, on the matrix cores.

    ``A``: ``torch.sparse_bsr``, ``(n, m)`` or batched ``(b, n, m)``, any block size ``(bh, bw)`` with ``bh, bw ≥ 1`` (non-square
    blocks, sides that are no multiple of 16 and blocks larger than one LDS stage included; the fast geometry is sides that are
    multiples of 16), float32, float64 or bfloat16 values, int32 or int64 indices, no dense dimensions.  ``B``: dense ``(m, p)`` or
    ``(b, m, p)`` of A's dtype on A's device, ``p ≥ 1`` (any strided view; copied when its column stride is not 1).  Returns dense
    ``(n, p)`` / ``(b, n, p)``.

    Every stored block is a term: the blocks of a block row are summed in stored order, column indices need not be sorted, a
    repeated ``(I, J)`` is two terms and each gets its own gradient, a stored zero block stays stored, and a block row without
    blocks gives zeros.  Accumulation is in float32 for float32 and bfloat16 (bfloat16 products are exact, the result is rounded once
    when stored) and in float64 for float64.  Deterministic: no float atomics, the summation order of an output element depends on
    its own block row (block column, for ``dL/dB``) only.

    Differentiable once.  ``dL/dA`` is a BSR tensor on A's own index tensors, with A's index dtype, whose values are
    ``dV[e] = G[I_e·bh : +bh, :] · B[J_e·bw : +bw, :]ᵀ``; ``dL/dB = Aᵀ·G``.  Each is computed only when it is asked for.

    What torch itself allows for gradients of a BSR operand:

    * ``torch.autograd.grad(loss, A)`` with respect to a BSR leaf works.
    * A ``values`` parameter wrapped by ``torch.sparse_bsr_tensor(crow, col, values, size)`` inside the graph works, with
      ``.backward()`` too: the training-loop form.  The pattern cache hits on the unchanged ``crow`` / ``col`` tensors.  (The
      backward of ``torch.sparse_bsr_tensor`` itself hands the gradient's blocks on sorted by column and merged, so this form
      needs torch's canonical pattern: sorted columns, no repeated ``(I, J)``.)
    * ``loss.backward()`` into a BSR leaf itself does not work ("Sparse BSR tensors do not have is_contiguous"): that is torch's
      ``AccumulateGrad``, and this function cannot change it.

    BSC operands are not served.
    """
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise ValueError("Both A and B should be instances of torch.Tensor")
    if A.dim() < 2 or B.dim() < 2:
        raise ValueError("Both A and B should be at least 2-dimensional tensors")
    if A.dim() != B.dim() or A.dim() not in (2, 3):
        raise ValueError("A and B must both be 2D or both be 3D tensors")
    if A.layout != torch.sparse_bsr:
        raise ValueError("A should be in BSR sparse format")
    if A.dense_dim() != 0:
        raise ValueError(f"A must not have dense dimensions, got dense_dim() = {A.dense_dim()}")
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
    return cast(torch.Tensor, SparseBSRMatMul.apply(A, B))
