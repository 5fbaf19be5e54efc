"""``sparse_bsr_attention`` — attention under a block-sparse (``torch.sparse_bsr``) mask, on the matrix cores.

Block masks are how long sequences are attended to: sliding windows, BigBird, block-causal and block-pruned patterns.  A stored
block is a dense ``bh × bw`` tile of logits, so ``Q_tile·K_blockᵀ`` and ``P·V_block`` are small GEMMs and ``K`` / ``V`` are read as
contiguous slabs — the case of :func:`sparse_attention` that maps onto MFMA, which that function's gather kernel never touches.  The
reference has no counterpart.

GPU operands run the flash-style kernels of ``csrc/bsr_attention_impl.h`` behind ``include/tsgu_hip_bsr_attention.h``: the forward
walks a block row's stored blocks stage by stage with an online softmax and keeps one log-sum-exp per (row, head); the backward
recomputes the probabilities from it in a pass over the block rows (``dQ``, ``dA``) and one over the cached transposed block
pattern (``dK``, ``dV``).  Logits and probabilities never reach global memory.  CPU operands take the torch-op path of ``_cpu.py``
over the element pattern the blocks cover.  The block pattern goes through the pattern cache of :func:`sparse_bsr_mm`
(``_pattern.from_bsr``); a batched operand is one block-diagonal pattern (``_pattern.flat_of``).
"""

from __future__ import annotations

import math
from typing import Optional, cast

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import _pattern as _pt

__all__ = ["sparse_bsr_attention", "SparseBSRAttention"]

_NAME = "sparse_bsr_attention"
_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
LIMITS = _be.BSR_ATTENTION_LIMITS


class SparseBSRAttention(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_bsr_attention` (once differentiable).  The gradient of ``A`` is a BSR tensor on A's own
    ``crow_indices()`` / ``col_indices()`` tensors with A's index dtype."""

    @staticmethod
    def forward(ctx, A, Q, K, V, heads, scale, use_bias):
        A = A.detach()
        plan = _pt.from_bsr(A)
        flat = _pt.flat_of(plan)
        values = A.values()
        bh, bw = values.shape[-2:]
        d = Q.size(-1)
        Q2, K2, V2 = Q.reshape(-1, heads * d), K.reshape(-1, heads * d), V.reshape(-1, heads * d)
        bias = values.reshape(-1, bh, bw).contiguous() if use_bias else None
        if Q2.is_cuda:
            O, lse, Oacc = _be.bsr_attention(flat.crow.contiguous(), flat.col.contiguous(), bias, bh, bw, Q2, K2, V2, heads, d, scale,
                                             want_acc=any(ctx.needs_input_grad[:4]))
            keep, ctx.walk = lse, None                      # keep: lse [b·n, H]; Oacc: O before its rounding (bfloat16), for δ
        else:
            O, ctx.walk, keep = _cpu.bsr_attention(flat, bias, bh, bw, Q2, K2, V2, heads, scale)     # keep: the probabilities
            Oacc = O
        ctx.plan, ctx.heads, ctx.scale, ctx.use_bias = plan, heads, scale, use_bias
        ctx.A_shape, ctx.values_shape, ctx.values_dtype, ctx.shape_k = A.shape, values.shape, values.dtype, K.shape
        ctx.save_for_backward(Q2, K2, V2, Oacc, keep, bias)    # (the bias too: autograd then sees an in-place change of A's values)
        return O.view(Q.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):  # type: ignore[override]
        Q2, K2, V2, O, keep, bias = ctx.saved_tensors
        plan: _pt.RowGather = ctx.plan
        flat = _pt.flat_of(plan)
        heads, scale = ctx.heads, ctx.scale
        bh, bw = ctx.values_shape[-2:]
        want_dA = ctx.needs_input_grad[0] and ctx.use_bias
        dO2 = dO.reshape(Q2.shape)
        if dO2.is_cuda:
            t = flat.transposed
            dQ, dK, dV, dA = _be.bsr_attention_backward(flat.crow.contiguous(), flat.col.contiguous(), (t.crow, t.col, t.perm), bias,
                                                        bh, bw, Q2, K2, V2, dO2, O, keep, heads, Q2.size(1) // heads, scale, want_dA)
        else:
            dQ, dK, dV, dA = _cpu.bsr_attention_backward(ctx.walk, bh, bw, Q2, K2, V2, dO2, keep, heads, scale, want_dA)
        gA = None
        if want_dA:
            gA = torch.sparse_bsr_tensor(plan.crow, plan.col, dA.to(ctx.values_dtype).view(ctx.values_shape), ctx.A_shape)
        return gA, dQ.view(dO.shape), dK.view(ctx.shape_k), dV.view(ctx.shape_k), None, None, None


def _fail(kind, what: str):
    raise kind(f"{_NAME}: {what}")


def sparse_bsr_attention(A: torch.Tensor, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, *, scale: Optional[float] = None,
                         values_as_bias: bool = True) -> torch.Tensor:
    r"""Attention under the block mask of a ``torch.sparse_bsr`` tensor ``A``: ``O[i,h,:] = Σ_j P[i,j,h]·V[j,h,:]`` with ``P[i,·,h]``
    the softmax, over the elements ``j`` that row ``i``'s stored blocks cover, of ``scale·<Q[i,h], K[j,h]> + A[i,j]``.

    ``A`` is ``(n, m)`` or batched ``(b, n, m)`` with float32, float64 or bfloat16 values, int32 or int64 indices and no dense
    dimensions.  Its stored values are added to the logits of every head — a ``-inf`` inside a stored block masks that element,
    which is how a causal diagonal block is written — or ignored with ``values_as_bias=False`` (``A`` then gets no gradient).
    ``Q`` is ``[n, d]`` or ``[n, H, d]``, ``K`` and ``V`` are ``[m, d]`` or ``[m, H, d]``, each with a leading ``b`` when ``A`` is
    batched, all of ``A``'s dtype and device.  ``scale`` defaults to ``d ** -0.5``.  On the GPU the block sides are multiples of 16,
    ``d`` is 16, 32, 64 or 128 and ``H ≥ 1``; anything else is a ``ValueError``, never another path.  Operands whose rows are not
    16-byte aligned are copied.

    The result has ``Q``'s shape.  Numerically this is :func:`sparse_attention`: a row whose block row is empty gives zeros and zero
    gradients; ``-inf`` beside finite logits has weight 0 and gradient 0; a row of only ``-inf``, or one holding NaN or ``+inf``,
    is NaN for that head.  The storage is that of :func:`sparse_bsr_mm`: block columns need not be sorted, a stored zero block stays
    stored, and a repeated ``(I, J)`` is two sets of entries — the same keys appear twice in the row's softmax and each block gets
    its own ``dA``.

    float32 and float64 multiply and accumulate in their own type.  bfloat16 runs all five products on the bf16 MFMA with float32
    accumulation: the probabilities enter ``P·V`` and ``Pᵀ·dO`` as bfloat16 (two terms, the rounded value and its rounded remainder:
    one rounding alone is 2^-8 at worst, which a row or column of one narrow block cannot average out) and ``dS`` is rounded to
    bfloat16 for ``dS·K`` and ``dSᵀ·Q`` — unlike :func:`sparse_attention`, whose bfloat16 is the float32 path rounded once.  The
    log-sum-exp, ``δ`` and ``dA`` stay float32 (a forward that a backward may follow also keeps ``O`` before its rounding, in
    float32, for ``δ = <dO, O>``) and results are rounded once when stored.  (CPU operands: float32 throughout, rounded once.)  Deterministic: no float atomics, every
    sum in an order that depends on the element's own block row (block column) only.

    Differentiable once: the gradients of ``Q``, ``K`` and ``V`` are dense; ``dA[e] = Σ_h dS[e,h]`` is a BSR tensor on A's own index
    tensors with A's index dtype.  What torch itself allows for gradients of a BSR operand:

    * ``torch.autograd.grad(loss, A)`` with respect to a BSR leaf works.
    * A ``values`` parameter wrapped by ``torch.sparse_bsr_tensor(crow, col, values, size)`` inside the graph works, with
      ``.backward()`` too: the training-loop form.  The pattern cache hits on the unchanged ``crow`` / ``col`` tensors.  (The
      backward of ``torch.sparse_bsr_tensor`` itself hands the gradient's blocks on sorted by column and merged, so this form
      needs torch's canonical pattern: sorted columns, no repeated ``(I, J)``.)
    * ``loss.backward()`` into a BSR leaf itself does not work ("Sparse BSR tensors do not have is_contiguous"): that is torch's
      ``AccumulateGrad``, and this function cannot change it.
    """
    if not isinstance(A, torch.Tensor) or A.layout != torch.sparse_bsr:
        _fail(TypeError, "A must be a torch.sparse_bsr tensor")
    if A.dim() not in (2, 3):
        _fail(NotImplementedError, f"A must be 2-D or batched 3-D, got ndim={A.dim()}")
    if A.dense_dim() != 0:
        _fail(ValueError, f"A must not have dense dimensions, got dense_dim() = {A.dense_dim()}")
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
        _fail(ValueError, f"V must have K's shape {tuple(K.shape)}, got {tuple(V.shape)}")
    if heads < 1 or d < 1:
        _fail(ValueError, f"Q needs at least one head and one column, got {tuple(Q.shape)}")
    _be.operand_device(A, Q, K, V)
    if scale is None:
        scale = d ** -0.5
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        _fail(ValueError, f"scale must be a finite number, got {scale!r}")
    bh, bw = A.values().shape[-2:]
    if A.is_cuda and not _be.bsr_attention_supported(A.dtype, heads, d, bh, bw):
        _fail(ValueError, f"the gfx950 kernels take {LIMITS}, got blocks of {bh} x {bw}, d={d} and H={heads}")
    return cast(torch.Tensor, SparseBSRAttention.apply(A, Q, K, V, heads, float(scale), bool(values_as_bias)))
