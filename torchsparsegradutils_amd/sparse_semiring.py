"""``sparse_semiring_mm`` — the sparse × dense product in the semirings log-domain code is written in::

    log       C[i, c] = log Σ_j exp(A[i, j] + B[j, c])      j over the stored entries of row i
    max_plus  C[i, c] = max_j (A[i, j] + B[j, c])
    min_plus  C[i, c] = min_j (A[i, j] + B[j, c])

The forward (``log``) and Viterbi (``max_plus``) recursions of an HMM or CRF with a sparse transition matrix, belief propagation on
a sparse factor graph, a Bellman–Ford relaxation (``min_plus``), a Sinkhorn half step for ``p`` marginals at once.  ``genbmm`` serves
the dense and banded side; the reference has no counterpart.

The kernels of ``csrc/semiring.hip`` keep the candidate ``A[i, j] + B[j, c]`` in a register from its gather to its use: the forward
is the row-group gather of ``sparse_mm``'s plan-free kernel with a one-``exp`` running (max, sum) — or (best, arg) — per column in
place of the sum, and both gradients are gathers too, one pass over the rows for the values and one over the cached transposed
pattern for ``B``.  There is never an ``nnz × p`` tensor.  Saved for the backward: the values, ``B`` and ``C`` in the accumulator
type (``log``) or the winners' positions ``arg`` (tropical) — for bfloat16 operands the forward writes a float32 copy of ``C`` in
the same pass when a gradient is needed, since a bfloat16 ``C`` in the exponent would put ``2⁻⁸·|C|`` into every weight.

CPU operands take the torch-op path of ``_cpu.py`` (a gather, ``scatter_reduce``, ``index_add``), which does keep the temporary.
"""

from __future__ import annotations

from typing import cast

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt
from .sparse_matmul import _Operand

__all__ = ["sparse_semiring_mm", "SparseSemiringMM"]

SEMIRINGS = ("log", "max_plus", "min_plus")
_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class SparseSemiringMM(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_semiring_mm` (once differentiable).  ``A`` is CSR or coalesced COO; the gradient of ``A``
    has A's layout, index tensors and index dtype."""

    @staticmethod
    def forward(ctx, A, B, semiring):
        grad_flag = A.requires_grad or B.requires_grad
        A, B = A.detach(), B.detach()
        op = _Operand(A)
        flat = _pt.flat_of(op.plan)
        p = B.size(-1)
        values = op.values.reshape(-1).contiguous()
        Bk = _be.rowmajor(B.reshape(-1, p))
        crow, col = flat.crow.contiguous(), flat.col.contiguous()
        if Bk.is_cuda:
            C, C_acc, arg = _be.csr_semiring_mm(crow, col, values, Bk, flat.n_rows, flat.n_cols, semiring, want_acc=grad_flag)
        else:
            (C, arg), C_acc = _cpu.semiring_mm(crow, col, values, Bk, (flat.n_rows, flat.n_cols), semiring), None
        ctx.op, ctx.semiring, ctx.B_shape = op, semiring, B.shape
        ctx.save_for_backward(values, Bk, C_acc if semiring == "log" else arg)
        C = C.view(B.shape[:-2] + (A.size(-2), p))
        C.requires_grad_(grad_flag)
        return C

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):  # type: ignore[override]
        values, Bk, kept = ctx.saved_tensors
        op: _Operand = ctx.op
        flat = _pt.flat_of(op.plan)
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        G = _be.rowmajor(grad.reshape(-1, grad.size(-1)))
        crow, col = flat.crow.contiguous(), flat.col.contiguous()
        gvals = gradB = None
        if G.is_cuda:
            C_acc, arg = (kept, None) if ctx.semiring == "log" else (None, kept)
            if need_a:
                gvals = _be.csr_semiring_mm_bwd_values(crow, col, values, Bk, C_acc, arg, G, flat.n_rows, flat.n_cols, ctx.semiring)
            if need_b:
                t = flat.transposed
                gradB = _be.csr_semiring_mm_bwd_dense(t.crow, t.col, t.perm, values, Bk, C_acc, arg, G, flat.n_rows, flat.n_cols,
                                                      ctx.semiring)
        else:
            gvals, gradB = _cpu.semiring_mm_backward(crow, col, values, Bk, (flat.n_rows, flat.n_cols), ctx.semiring, G, need_a, need_b)
        gradA = op.rebuild(gvals.view(op.values.shape)) if need_a else None
        return gradA, (gradB.view(ctx.B_shape) if need_b else None), None


def sparse_semiring_mm(A: torch.Tensor, B: torch.Tensor, semiring: str = "log") -> torch.Tensor:
    r"""Sparse–dense product in the ``"log"``, ``"max_plus"`` or ``"min_plus"`` semiring: ``C[i,c] = ⊕_e (val[e] + B[col[e],c])`` over
    the stored entries ``e`` of row ``i`` of ``A``, with ``⊕`` a log-sum-exp, a maximum or a minimum.

    ``A``: sparse COO or CSR, ``(n, m)`` or ``(b, n, m)``, float32, float64 or bfloat16 values, int32 or int64 indices; ``B``: dense
    ``(m, p)`` or ``(b, m, p)`` of A's dtype on A's device.  Returns dense ``(n, p)`` / ``(b, n, p)``.  An un-coalesced COO ``A`` is
    coalesced first.

    Only stored entries are candidates: an absent entry is the semiring's zero, and a row without entries gives ``-inf`` (``+inf``
    for ``min_plus``).  The candidate is one addition in float32 for float32 and bfloat16 operands (the result rounded once), in
    float64 for float64.

    * ``"log"``: a candidate of ``-inf`` is an absent entry, also when it is the only one in its row; its gradient weight is 0.  A
      ``+inf`` candidate gives ``+inf``, a NaN gives NaN.
    * ``"max_plus"`` / ``"min_plus"``: of equal candidates the one stored first wins (``+0.0 == -0.0``); a NaN candidate wins over
      any number, and the first NaN stays.  The gradients flow through the winner only.

    Differentiable once in both operands.  ``dL/dA`` comes back in A's layout, on A's own index tensors, with its index dtype.
    """
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise TypeError("Both A and B should be instances of torch.Tensor")
    if semiring not in SEMIRINGS:
        raise ValueError(f"semiring must be one of 'log', 'max_plus' or 'min_plus', got {semiring!r}")
    if A.layout not in {torch.sparse_coo, torch.sparse_csr}:
        raise TypeError(f"A should be in either COO or CSR sparse format, got {A.layout}")
    if B.layout != torch.strided:
        raise TypeError(f"B must be a dense (strided) tensor, got {B.layout}")
    if A.dtype != B.dtype:
        raise TypeError(f"expected A and B to have the same dtype, got {A.dtype} and {B.dtype}")
    if A.dtype not in _DTYPES:
        raise TypeError(f"values must be float32, float64 or bfloat16, got {A.dtype}")
    if A.dim() != B.dim() or A.dim() not in (2, 3):
        raise ValueError("A and B must both be 2D or both be 3D tensors")
    if A.dim() == 3 and A.size(0) != B.size(0):
        raise ValueError("If batched, A and B must have the same batch size")
    if A.size(-1) != B.size(-2):
        raise ValueError(f"Incompatible inner dimensions: A[..., {A.size(-1)}] vs B[..., {B.size(-2)}]")
    if B.size(-1) < 1:
        raise ValueError("B needs at least one column")
    if A.device != B.device:
        raise RuntimeError(f"A and B must be on the same device, got {A.device} and {B.device}")
    if A.layout == torch.sparse_coo and not A.is_coalesced():
        A = A.coalesce()
    return cast(torch.Tensor, SparseSemiringMM.apply(A, B, semiring))
