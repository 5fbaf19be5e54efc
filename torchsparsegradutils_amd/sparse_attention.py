"""Attention over a sparse pattern: ``softmax_row(scale·QKᵀ restricted to the pattern + bias) · V`` as one operation.

What a graph-transformer or GAT layer calls: the logits ``scale·<Q[i,h], K[j,h]> + A[i,j]`` exist at the stored positions of ``A``
only (an absent entry is −inf, as in :func:`sparse_softmax`), every row is normalised among its stored entries per head, and the
probabilities weight the rows of ``V``.  The reference has no counterpart.

The composition ``csr_sddmm → + bias → sparse_softmax → sparse_mm`` writes and re-reads the ``nnz`` logits three times, once more
per head, and saves the ``nnz·H`` probabilities for the backward.  Here GPU operands run the fused kernels of
``csrc/attention.hip``: the logits never leave registers, the forward saves one log-sum-exp per (row, head), and the backward
recomputes the probabilities from it in a pass over the rows (``dQ``, ``dA``) and one over the cached transpose (``dK``, ``dV``).
CPU operands run the torch-op path of ``_cpu.py``.

The pattern is the one of :func:`sparse_logsumexp` (``_Operand``): the rows of a CSR / coalesced-COO matrix are the segments of
its own ``crow``; a CSC matrix is walked by rows through its cached transpose (values through its ``perm``); a batched input is
one block-diagonal pattern over ``Q/K/V`` flattened to ``[b·n, H·d]``.  Autograd is first order only; ``dA`` is sparse on ``A``'s
own index tensors.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from .sparse_logsumexp import _check_input, _Operand

__all__ = ["sparse_attention", "SparseAttention"]

_NAME = "sparse_attention"
_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
LIMITS = "d in {8, 16, 32, 64, 128}, V as wide as Q and K, and H*d <= 1024"


def _walks(op: _Operand):
    """((ptr, idx, perm) by rows, the same by columns) of the operand's (block-diagonal) pattern."""
    g, t = op.plan, op.plan.transposed
    own, other = (g.crow, g.col, g.perm), (t.crow, t.col, t.perm)
    return (own, other) if op.rows_first else (other, own)


class SparseAttention(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_attention` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, Q, K, V, op, heads, scale, use_bias):
        b, n, m = op.batch or 1, op.n_rows, op.n_cols
        d = Q.size(-1)
        Q2, K2, V2 = Q.reshape(b * n, heads * d), K.reshape(b * m, heads * d), V.reshape(b * m, heads * d)
        bias = op.values.reshape(-1).contiguous() if use_bias else None
        rows, _ = _walks(op)
        if Q.is_cuda:
            O, keep = _be.csr_attention(rows, bias, Q2, K2, V2, heads, d, scale)       # keep: lse [b·n, H]
        else:
            O, keep = _cpu.attention(*rows, bias, Q2, K2, V2, heads, scale)            # keep: the probabilities [nnz, H]
        ctx.op, ctx.heads, ctx.scale, ctx.use_bias, ctx.shape_k = op, heads, scale, use_bias, K.shape
        ctx.save_for_backward(Q2, K2, V2, keep, bias)      # (the bias too: autograd then sees an in-place change of A's values)
        return O.view(Q.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        Q2, K2, V2, keep, bias = ctx.saved_tensors
        op: _Operand = ctx.op
        heads, scale = ctx.heads, ctx.scale
        want_dA = ctx.needs_input_grad[0] and ctx.use_bias
        rows, cols = _walks(op)
        dO2 = dO.reshape(Q2.shape)
        if dO2.is_cuda:
            dQ, dK, dV, dA = _be.csr_attention_backward(rows, cols, bias, Q2, K2, V2, dO2, keep, heads, Q2.size(1) // heads, scale,
                                                        want_dA)
        else:
            dQ, dK, dV, dA = _cpu.attention_backward(*rows, Q2, K2, V2, dO2, keep, heads, scale, want_dA)
        gA = op.rebuild(dA.to(op.values.dtype)) if want_dA else None
        return gA, dQ.view(dO.shape), dK.view(ctx.shape_k), dV.view(ctx.shape_k), None, None, None, None


def _fail(kind, what: str):
    raise kind(f"{_NAME}: {what}")


def sparse_attention(A: torch.Tensor, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, *, scale: Optional[float] = None,
                     values_as_bias: bool = True) -> torch.Tensor:
    r"""Attention over the stored positions of a sparse COO / CSR / CSC tensor ``A``:
    ``O[i,h,:] = Σ_j P[i,j,h]·V[j,h,:]`` with ``P[i,·,h]`` the softmax over row ``i``'s stored ``j`` of
    ``scale·<Q[i,h], K[j,h]> + A[i,j]``.

    ``A`` is ``[n, m]`` or batched ``[b, n, m]`` with float32, float64 or bfloat16 values and int32 or int64 indices (uncoalesced
    COO is coalesced first).  Only stored positions take part; their values are added to the logits of every head, or ignored
    with ``values_as_bias=False`` (``A`` then gets no gradient).  ``Q`` is ``[n, d]`` or ``[n, H, d]``, ``K`` and ``V`` are
    ``[m, d]`` or ``[m, H, d]``, each with a leading ``b`` when ``A`` is batched, all of ``A``'s dtype and device.  ``scale``
    defaults to ``d ** -0.5``.  On the GPU ``d`` is 8, 16, 32, 64 or 128 and ``H·d <= 1024``.

    The result has ``Q``'s shape.  A row without stored entries gives zeros and zero gradients; a row whose logits hold a NaN or
    ``+inf``, or nothing but ``-inf``, is NaN for that head; ``-inf`` beside finite logits has weight 0 and gradient 0.  bfloat16
    is computed in float32 and rounded once (the result and every gradient).  Differentiable once: the gradients of ``Q``, ``K``
    and ``V`` are dense, the gradient of ``A`` is sparse on ``A``'s own index tensors (``dA[i,j] = Σ_h dS[i,j,h]``).
    """
    _check_input(A, _NAME)
    if A.dtype not in _DTYPES:
        _fail(TypeError, f"values must be float32, float64 or bfloat16, got {A.dtype}")
    batched = A.dim() == 3
    for name, t in (("Q", Q), ("K", K), ("V", V)):
        if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
            _fail(TypeError, f"{name} must be a dense tensor")
        if t.dtype != A.dtype:
            _fail(TypeError, f"A, Q, K and V must have one dtype, got {A.dtype} for A and {t.dtype} for {name}")
    lead = 1 if batched else 0
    if Q.dim() - lead not in (2, 3):
        form = "[b, n, d] or [b, n, H, d] for a batched A" if batched else "[n, d] or [n, H, d]"
        _fail(ValueError, f"Q must be {form}, got {tuple(Q.shape)}")
    if K.dim() != Q.dim() or V.dim() != Q.dim():
        _fail(ValueError, f"Q, K and V must have the same number of dimensions, got {Q.dim()}, {K.dim()} and {V.dim()}")
    multi = Q.dim() - lead == 3
    heads, d = (Q.size(-2) if multi else 1), Q.size(-1)
    want_q = tuple(A.shape[:-1]) + ((heads, d) if multi else (d,))
    want_k = tuple(A.shape[:-2]) + (A.size(-1),) + ((heads, d) if multi else (d,))
    if tuple(Q.shape) != want_q:
        _fail(ValueError, f"Q must be {want_q} for A of shape {tuple(A.shape)}, got {tuple(Q.shape)}")
    if tuple(K.shape) != want_k:
        _fail(ValueError, f"K must be {want_k} for A of shape {tuple(A.shape)} and Q of shape {tuple(Q.shape)}, got {tuple(K.shape)}")
    if tuple(V.shape) != tuple(K.shape):
        _fail(ValueError, f"V must have K's shape {tuple(K.shape)} ({LIMITS}), got {tuple(V.shape)}")
    if heads < 1 or d < 1:
        _fail(ValueError, f"Q needs at least one head and one column, got {tuple(Q.shape)}")
    _be.operand_device(A, Q, K, V)
    if scale is None:
        scale = d ** -0.5
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        _fail(ValueError, f"scale must be a finite number, got {scale!r}")
    if A.is_cuda and not _be.attention_supported(A.dtype, heads, d):
        _fail(ValueError, f"the gfx950 kernels take {LIMITS}, got d={d} and H={heads} (H*d={heads * d})")
    op = _Operand(A)
    return SparseAttention.apply(op.A, Q, K, V, op, heads, float(scale), bool(values_as_bias))
