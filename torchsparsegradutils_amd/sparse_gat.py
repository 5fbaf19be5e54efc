"""Graph attention layers (GAT, GATv2) over a sparse pattern as one operation each.

The logit of :func:`sparse_attention` is a dot product; the GAT logits have a LeakyReLU inside them, which no choice of ``Q`` and
``K`` reproduces::

    GAT    e[i,j,h] = lrelu(s_dst[i,h] + s_src[j,h])                      + A[i,j]      O[i,h,:] = Σ_j P[i,j,h]·V[j,h,:]
    GATv2  e[i,j,h] = Σ_k att[h,k]·lrelu(X_dst[i,h,k] + X_src[j,h,k])     + A[i,j]      O[i,h,:] = Σ_j P[i,j,h]·X_src[j,h,:]

with ``P[i,·,h]`` the softmax over row ``i``'s stored ``j``.  The composition builds an ``nnz × H`` (GATv2: ``nnz × H × d``) tensor
with torch ops, keeps it for the backward and calls ``sparse_softmax`` and ``sparse_mm`` once per head.  Here GPU operands run the
kernels of ``csrc/gat.hip``: the GAT forward computes every weight once per (entry, head) through LDS and aggregates with a plain
gather-FMA loop; the GATv2 forward scores and aggregates the one gathered ``X_src[j]`` from registers; both save one log-sum-exp
per (row, head), and the backward recomputes the probabilities in a pass over the rows and one over the cached transpose.  ``datt``
is summed from per-workgroup shares in a fixed order: no atomics, the same bits on every call.  CPU operands run the torch-op path
of ``_cpu.py``.

The pattern contract is :func:`sparse_attention`'s (``_check_input`` / ``_Operand``).  Autograd is first order only; ``dA`` is sparse
on ``A``'s own index tensors.
"""

from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from .sparse_attention import LIMITS, _walks
from .sparse_logsumexp import _check_input, _Operand

__all__ = ["sparse_gat_attention", "sparse_gatv2_attention", "SparseGATAttention", "SparseGATv2Attention"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


def _forward(ctx, kind, op, s_dst, s_src, X_dst, X_src, att, heads, slope, use_bias):
    """The forward both classes share: operands flattened to [rows, heads(·d)], `keep` = lse (GPU) or the probabilities (CPU)."""
    b, n, m = op.batch or 1, op.n_rows, op.n_cols
    d = X_src.size(-1)
    flat = (lambda t, rows, w: None if t is None else t.reshape(b * rows, w))
    sd, ss = flat(s_dst, n, heads), flat(s_src, m, heads)
    xd, xs = flat(X_dst, n, heads * d), flat(X_src, m, heads * d)
    a = None if att is None else att.reshape(heads * d).contiguous()
    if sd is not None:
        sd, ss = sd.contiguous(), ss.contiguous()
    bias = op.values.reshape(-1).contiguous() if use_bias else None
    rows, _ = _walks(op)
    if X_src.is_cuda:
        O, keep = _be.csr_gat_forward(kind, rows, bias, sd, ss, xd, xs, a, heads, d, slope)
    else:
        O, keep = _cpu.gat_attention(kind, *rows, bias, sd, ss, xd, xs, a, heads, slope)
    ctx.op, ctx.kind, ctx.heads, ctx.d, ctx.slope, ctx.use_bias = op, kind, heads, d, slope, use_bias
    ctx.save_for_backward(sd, ss, xd, xs, a, keep, bias)
    return O


def _backward(ctx, dO):
    sd, ss, xd, xs, a, keep, bias = ctx.saved_tensors
    op: _Operand = ctx.op
    want_dA = ctx.needs_input_grad[0] and ctx.use_bias
    rows, cols = _walks(op)
    dO2 = dO.reshape(-1, ctx.heads * ctx.d)
    if dO2.is_cuda:
        d_dst, d_src, ds_src, datt, dA = _be.csr_gat_backward(ctx.kind, rows, cols, bias, sd, ss, xd, xs, a, dO2, keep, ctx.heads,
                                                              ctx.d, ctx.slope, want_dA)
    else:
        d_dst, d_src, ds_src, datt, dA = _cpu.gat_attention_backward(ctx.kind, *rows, bias, sd, ss, xd, xs, a, dO2, keep, ctx.heads,
                                                                     ctx.slope, want_dA)
    gA = op.rebuild(dA.to(op.values.dtype)) if want_dA else None
    return gA, d_dst, d_src, ds_src, datt


class SparseGATAttention(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_gat_attention` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, s_dst, s_src, V, op, heads, slope, use_bias):
        ctx.shapes = (s_dst.shape, s_src.shape, V.shape)
        return _forward(ctx, "gat", op, s_dst, s_src, None, V, None, heads, slope, use_bias).view(s_dst.shape + V.shape[-1:])

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        gA, ds_dst, dV, ds_src, _ = _backward(ctx, dO)
        sh = ctx.shapes
        return gA, ds_dst.view(sh[0]), ds_src.view(sh[1]), dV.view(sh[2]), None, None, None, None


class SparseGATv2Attention(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_gatv2_attention` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, X_dst, X_src, att, op, heads, slope, use_bias):
        ctx.shapes = (X_dst.shape, X_src.shape, att.shape)
        return _forward(ctx, "gatv2", op, None, None, X_dst, X_src, att, heads, slope, use_bias).view(X_dst.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dO):
        gA, dX_dst, dX_src, _, datt = _backward(ctx, dO)
        sh = ctx.shapes
        return gA, dX_dst.view(sh[0]), dX_src.view(sh[1]), datt.view(sh[2]), None, None, None, None


def _checked(name: str, A, operands, shapes, negative_slope, heads: int, d: int) -> _Operand:
    """The validation both functions share.  operands: ((name, tensor), …); shapes: the shape every one of them must have."""

    def fail(kind, what: str):
        raise kind(f"{name}: {what}")

    _check_input(A, name)
    if A.dtype not in _DTYPES:
        fail(TypeError, f"values must be float32, float64 or bfloat16, got {A.dtype}")
    names = ", ".join(nm for nm, _ in operands)
    for nm, t in operands:
        if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
            fail(TypeError, f"{nm} must be a dense tensor")
        if t.dtype != A.dtype:
            fail(TypeError, f"A, {names} must have one dtype, got {A.dtype} for A and {t.dtype} for {nm}")
    for (nm, t), want in zip(operands, shapes):
        if tuple(t.shape) != tuple(want):
            fail(ValueError, f"{nm} must be {tuple(want)} for A of shape {tuple(A.shape)} and {operands[0][0]} of shape "
                             f"{tuple(operands[0][1].shape)}, got {tuple(t.shape)}")
    if heads < 1 or d < 1:
        fail(ValueError, f"the operands need at least one head and one column, got H={heads} and d={d}")
    _be.operand_device(A, *(t for _, t in operands))
    if isinstance(negative_slope, bool) or not isinstance(negative_slope, (int, float)) or not math.isfinite(negative_slope):
        fail(ValueError, f"negative_slope must be a finite number, got {negative_slope!r}")
    if A.is_cuda and not _be.gat_supported(A.dtype, heads, d):
        fail(ValueError, f"the gfx950 kernels take {LIMITS}, got d={d} and H={heads} (H*d={heads * d})")
    return _Operand(A)


def _fail(name: str, kind, what: str):
    raise kind(f"{name}: {what}")


def sparse_gat_attention(A: torch.Tensor, s_dst: torch.Tensor, s_src: torch.Tensor, V: torch.Tensor, *, negative_slope: float = 0.2,
                         values_as_bias: bool = True) -> torch.Tensor:
    r"""A GAT layer's attention over the stored positions of a sparse COO / CSR / CSC tensor ``A``:
    ``O[i,h,:] = Σ_j P[i,j,h]·V[j,h,:]`` with ``P[i,·,h]`` the softmax over row ``i``'s stored ``j`` of
    ``leaky_relu(s_dst[i,h] + s_src[j,h]) + A[i,j]``.

    ``A`` is ``[n, m]`` or batched ``[b, n, m]`` with float32, float64 or bfloat16 values and int32 or int64 indices (uncoalesced
    COO is coalesced first).  Only stored positions take part; their values are added to the logits of every head, or ignored
    with ``values_as_bias=False`` (``A`` then gets no gradient).  ``s_dst`` is ``[n, H]``, ``s_src`` ``[m, H]`` and ``V``
    ``[m, H, d]`` — or ``[n]``, ``[m]``, ``[m, d]`` for one head — each with a leading ``b`` when ``A`` is batched, all of ``A``'s
    dtype and device.  On the GPU ``d`` is 8, 16, 32, 64 or 128 and ``H·d <= 1024``.

    The result is ``[n, H, d]`` (``[n, d]``).  Special values, bfloat16 and the gradients follow :func:`sparse_attention`: empty
    rows give zeros, ``-inf`` beside finite logits has weight 0, a row with a NaN, ``+inf`` or only ``-inf`` is NaN for that head;
    bfloat16 is computed in float32 and rounded once; once differentiable, ``dA[i,j] = Σ_h dS[i,j,h]`` on ``A``'s own index tensors.
    The LeakyReLU's derivative at exactly 0 is ``negative_slope``.
    """
    name = "sparse_gat_attention"
    if not isinstance(V, torch.Tensor) or not isinstance(s_dst, torch.Tensor):
        _fail(name, TypeError, "s_dst, s_src and V must be dense tensors")
    lead = 1 if (isinstance(A, torch.Tensor) and A.dim() == 3) else 0
    if s_dst.dim() - lead not in (1, 2):
        form = "[b, n] or [b, n, H] for a batched A" if lead else "[n] or [n, H]"
        _fail(name, ValueError, f"s_dst must be {form}, got {tuple(s_dst.shape)}")
    multi = s_dst.dim() - lead == 2
    heads, d = (s_dst.size(-1) if multi else 1), (V.size(-1) if V.dim() else 0)
    hs = (heads,) if multi else ()
    front = tuple(A.shape[:-2]) if isinstance(A, torch.Tensor) else ()
    n, m = (A.size(-2), A.size(-1)) if isinstance(A, torch.Tensor) and A.dim() >= 2 else (0, 0)
    op = _checked(name, A, (("s_dst", s_dst), ("s_src", s_src), ("V", V)),
                  (front + (n,) + hs, front + (m,) + hs, front + (m,) + hs + (d,)), negative_slope, heads, d)
    return SparseGATAttention.apply(op.A, s_dst, s_src, V, op, heads, float(negative_slope), bool(values_as_bias))


def sparse_gatv2_attention(A: torch.Tensor, X_dst: torch.Tensor, X_src: torch.Tensor, att: torch.Tensor, *,
                           negative_slope: float = 0.2, values_as_bias: bool = True) -> torch.Tensor:
    r"""A GATv2 layer's attention over the stored positions of ``A``: ``O[i,h,:] = Σ_j P[i,j,h]·X_src[j,h,:]`` with ``P[i,·,h]``
    the softmax over row ``i``'s stored ``j`` of ``Σ_k att[h,k]·leaky_relu(X_dst[i,h,k] + X_src[j,h,k]) + A[i,j]``.

    ``X_dst`` is ``[n, H, d]``, ``X_src`` ``[m, H, d]`` and ``att`` ``[H, d]`` — or ``[n, d]``, ``[m, d]``, ``[d]`` for one head;
    ``X_dst`` and ``X_src`` carry a leading ``b`` when ``A`` is batched, ``att`` is shared by the batch items.  Everything else is
    as for :func:`sparse_gat_attention`; the gradients of ``X_dst``, ``X_src`` and ``att`` are dense, and ``datt`` is summed in a
    fixed order (two calls give the same bits).
    """
    name = "sparse_gatv2_attention"
    if not isinstance(X_dst, torch.Tensor):
        _fail(name, TypeError, "X_dst must be a dense tensor")
    lead = 1 if (isinstance(A, torch.Tensor) and A.dim() == 3) else 0
    if X_dst.dim() - lead not in (2, 3):
        form = "[b, n, d] or [b, n, H, d] for a batched A" if lead else "[n, d] or [n, H, d]"
        _fail(name, ValueError, f"X_dst must be {form}, got {tuple(X_dst.shape)}")
    multi = X_dst.dim() - lead == 3
    heads, d = (X_dst.size(-2) if multi else 1), X_dst.size(-1)
    hd = (heads, d) if multi else (d,)
    front = tuple(A.shape[:-2]) if isinstance(A, torch.Tensor) else ()
    n, m = (A.size(-2), A.size(-1)) if isinstance(A, torch.Tensor) and A.dim() >= 2 else (0, 0)
    op = _checked(name, A, (("X_dst", X_dst), ("X_src", X_src), ("att", att)), (front + (n,) + hd, front + (m,) + hd, hd),
                  negative_slope, heads, d)
    return SparseGATv2Attention.apply(op.A, X_dst, X_src, att, op, heads, float(negative_slope), bool(values_as_bias))
