"""``sparse_topk_mm`` — the ``k`` largest entries of ``scale·Q·Kᵀ + key_bias`` per row as a sparse CSR matrix with gradients: the
op that derives a pattern from the data (kNN graphs, top-k attention, retrieval) for the ops here that take one.  The reference has
no counterpart.

``torch.topk(Q @ K.T, k)`` writes the ``n × m`` scores, sends a dense ``n × m`` cotangent back and promises no order among ties.  Here
GPU operands run one launch of ``csrc/topk.hip``: a workgroup owns a tile of query rows, streams the keys through LDS, forms the
scores on the matrix cores and feeds them to a running per-row selection — no score reaches global memory.  The order is total
(NaN above ``+inf``, then the lower column), so the selected set is a function of the scores alone.  The row pointer follows from
``(n, m, k, causal, exclude_self)`` in closed form: nothing is read back from the device and the call can be captured in a graph.
CPU operands run the torch-op path of ``_cpu.py``.

The selection is piecewise constant; with ``G`` the cotangent on the result's own pattern, ``dQ = scale·G·K``, ``dK = scale·Gᵀ·Q`` and
``d key_bias = Gᵀ·1`` are the package's sparse products (``_ops.spmm`` / ``_ops.spmm_t``) on the result's index tensors.  Autograd is first
order only: a second differentiation raises.
"""

from __future__ import annotations

import math
from typing import Optional, cast

import torch

from . import _backend as _be
from . import _cpu
from . import _ops
from .sparse_logsumexp import _Operand
from .sparse_softmax import _restrict

__all__ = ["sparse_topk_mm", "SparseTopkMM"]

_NAME = "sparse_topk_mm"
_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


def _fail(kind, what: str):
    raise kind(f"{_NAME}: {what}")


def row_counts(n: int, m: int, k: int, causal: bool, exclude_self: bool, device=None) -> torch.Tensor:
    """Entries per row, int64 ``[n]``: ``min(k, allowed columns of row i)``; all ``j < m``, with `causal` ``j <= i + (m − n)``, with
    `exclude_self` ``j != i``."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    lim = (i + (m - n + 1)).clamp_(0, m) if causal else torch.full_like(i, m)
    if exclude_self:
        lim = lim - (i < lim).to(torch.int64)
    return lim.clamp_(max=k)


def nnz_of(n: int, m: int, k: int, causal: bool, exclude_self: bool) -> int:
    """``row_counts(...).sum()`` in integer arithmetic.  Without `causal` the min(n, m) rows that have a column of their own lose it
    to `exclude_self`, every other row may take all m.  With `causal` row i may take max(0, i + c) columns, c = m − n + 1, one fewer
    with `exclude_self` when n <= m (for n > m the diagonal is beyond the causal limit): a ramp clamped to [0, k]."""
    if not causal:
        own = min(n, m) if exclude_self else 0
        return own * min(k, max(m - 1, 0)) + (n - own) * min(k, m)
    c = m - n + 1 - (1 if exclude_self and n <= m else 0)

    def ramp(x: int) -> int:          # Σ_{t=0..x} min(t, k)
        return 0 if x < 0 else (x * (x + 1) // 2 if x <= k else k * (k + 1) // 2 + (x - k) * k)

    return ramp(c + n - 1) - ramp(max(c, 0) - 1) if n > 0 else 0


def _row_pointer(n: int, m: int, k: int, causal: bool, exclude_self: bool, index_dtype, device):
    """(crow on `device`, nnz): the closed form, as torch ops on the device for the pointer and in integers for the count."""
    crow = torch.zeros(n + 1, dtype=torch.int64, device=device)
    torch.cumsum(row_counts(n, m, k, causal, exclude_self, device), 0, out=crow[1:])
    return crow.to(index_dtype), nnz_of(n, m, k, causal, exclude_self)


class SparseTopkMM(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_topk_mm` (once differentiable)."""

    @staticmethod
    def forward(ctx, Q, K, key_bias, k, scale, causal, exclude_self, index_dtype):
        batched = Q.dim() == 3
        Q3, K3 = (Q, K) if batched else (Q.unsqueeze(0), K.unsqueeze(0))
        bias2 = None if key_bias is None else (key_bias if batched else key_bias.unsqueeze(0))
        b, n, _ = Q3.shape
        m = K3.size(1)
        crow, nnz = _row_pointer(n, m, k, causal, exclude_self, index_dtype, Q.device)
        if index_dtype == torch.int32 and nnz >= 2 ** 31:
            _fail(ValueError, f"the result has {nnz} stored entries per matrix, which needs index_dtype=torch.int64")
        if Q.is_cuda:
            col = torch.empty((b, nnz), dtype=index_dtype, device=Q.device)
            val = torch.empty((b, nnz), dtype=Q.dtype, device=Q.device)
            flags = (_be.TOPK_CAUSAL if causal else 0) | (_be.TOPK_EXCLUDE_SELF if exclude_self else 0)
            _be.topk_mm(Q3.contiguous(), K3.contiguous(), None if bias2 is None else bias2.contiguous(), k, scale, flags, m - n, crow, col,
                        val)
        else:
            col, val = _cpu.topk_mm(Q3, K3, bias2, k, scale, causal, exclude_self, row_counts(n, m, k, causal, exclude_self), index_dtype)
        if batched:
            out = torch.sparse_csr_tensor(crow.expand(b, -1).contiguous(), col, val, (b, n, m))
        else:
            out = torch.sparse_csr_tensor(crow, col[0], val[0], (n, m))
        ctx.scale, ctx.has_bias = scale, key_bias is not None
        ctx.pattern = (out.crow_indices(), out.col_indices(), tuple(out.shape))
        ctx.save_for_backward(Q, K)
        return out

    @staticmethod
    def backward(ctx, grad):  # type: ignore[override]
        with torch.no_grad():
            grads = SparseTopkMM._grads(ctx, grad)
        if not torch.is_grad_enabled():
            return grads
        # create_graph=True.  `once_differentiable` arms its error only when a cotangent requires a gradient, and the cotangent of a
        # sparse result arrives without one (torch builds it from `values()` outside the graph): a second differentiation would come
        # back detached, silently.  The same delayed error, armed always.
        fail = torch._C._functions.DelayedError(
            b"trying to differentiate twice a function that was marked with @once_differentiable", len(grads))
        return fail(*[None if g is None else g.detach().requires_grad_(True) for g in grads])

    @staticmethod
    def _grads(ctx, grad):
        need_q, need_k, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        if not (need_q or need_k or need_b):
            return (None,) * 8
        Q, K = ctx.saved_tensors
        crow, col, shape = ctx.pattern
        op = _Operand(torch.sparse_csr_tensor(crow, col, torch.empty(col.shape, dtype=Q.dtype, device=Q.device), shape))
        # bfloat16 is rounded ONCE: scale·G would be a second rounding in bfloat16, so with a scale the products run on the float32
        # kernels (the operands are converted exactly) and the result is rounded.  (torch's CPU sparse product has no bfloat16 at all.)
        wide = torch.float32 if Q.dtype == torch.bfloat16 and (ctx.scale != 1.0 or not Q.is_cuda) else Q.dtype
        g = _restrict(op, grad).reshape(-1).to(wide).contiguous()
        d = Q.size(-1)
        Q2, K2 = Q.reshape(-1, d).to(wide), K.reshape(-1, d).to(wide)      # the rows of the block-diagonal pattern of a batched result
        gs = g if ctx.scale == 1.0 else g * ctx.scale
        dQ = _ops.spmm(op.plan, gs, K2).reshape(Q.shape).to(Q.dtype) if need_q else None
        dK = _ops.spmm_t(op.plan, gs, Q2).reshape(K.shape).to(K.dtype) if need_k else None
        db = None
        if need_b:
            ones = torch.ones((Q2.size(0), 1), dtype=wide, device=Q.device)
            db = _ops.spmm_t(op.plan, g, ones).reshape(K.shape[:-1]).to(K.dtype)
        return dQ, dK, db, None, None, None, None, None


def sparse_topk_mm(Q: torch.Tensor, K: torch.Tensor, k: int, *, scale: float = 1.0, key_bias: Optional[torch.Tensor] = None,
                   causal: bool = False, exclude_self: bool = False, index_dtype: torch.dtype = torch.int32) -> torch.Tensor:
    r"""The ``k`` largest scores ``s[i, j] = scale·<Q[i], K[j]> + key_bias[j]`` of every row as a sparse CSR matrix.

    ``Q`` is ``[n, d]`` or ``[b, n, d]``, ``K`` is ``[m, d]`` or ``[b, m, d]``, dense, of one dtype (float32, float64 or bfloat16) and one
    device, ``d >= 1``; ``key_bias`` is ``[m]`` or ``[b, m]`` of the same dtype.  The scores are accumulated in float32 (float64 for
    float64 operands) and compared before any rounding to bfloat16.  For one pattern per head fold the heads into the batch
    (``[b·H, n, d]``); :func:`sparse_attention` shares one pattern across its heads.

    Row ``i`` may take every ``j < m``; with ``causal`` only ``j <= i + (m − n)`` (bottom-right aligned, as
    ``scaled_dot_product_attention``; a row without an allowed column is empty); with ``exclude_self`` not ``j = i``.  It stores
    exactly ``min(k, allowed)`` entries, the largest scores among its allowed columns: NaN ranks above ``+inf`` as in ``torch.topk``,
    and among equal scores the lower column wins, so the set is a function of the scores alone.  The columns of a row are stored
    ascending, the value is the score in the operands' dtype (bfloat16 rounded once).

    Returns a ``torch.sparse_csr_tensor`` of shape ``[n, m]`` or ``[b, n, m]`` (the same nnz in every batch item) with ``index_dtype``
    (int32 or int64) indices.  Its row pointer is computed in closed form: the call does not synchronise with the device.  On the
    GPU ``k`` is at most the kernels' cap (128).

    Differentiable once in ``Q``, ``K`` and ``key_bias``: the selection is piecewise constant, and with ``G`` the upstream gradient on
    the result's pattern ``dQ = scale·G·K``, ``dK = scale·Gᵀ·Q``, ``d key_bias = Gᵀ·1``.

    An L2 kNN graph: ranking by ``−‖q − k‖²`` is ranking by ``<q, k> − ½‖k‖²``, so
    ``sparse_topk_mm(X, X, k, key_bias=-0.5 * (X * X).sum(-1), exclude_self=True)``.
    """
    for name, t in (("Q", Q), ("K", K)) + ((("key_bias", key_bias),) if key_bias is not None else ()):
        if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
            _fail(TypeError, f"{name} must be a dense tensor")
    if Q.dtype not in _DTYPES:
        _fail(TypeError, f"Q and K must be float32, float64 or bfloat16, got {Q.dtype}")
    if K.dtype != Q.dtype or (key_bias is not None and key_bias.dtype != Q.dtype):
        other = K.dtype if K.dtype != Q.dtype else cast(torch.Tensor, key_bias).dtype
        _fail(TypeError, f"Q, K and key_bias must have one dtype, got {Q.dtype} and {other}")
    if Q.dim() not in (2, 3):
        _fail(ValueError, f"Q must be [n, d] or [b, n, d], got {tuple(Q.shape)}")
    if K.dim() != Q.dim() or K.size(-1) != Q.size(-1) or K.shape[:-2] != Q.shape[:-2]:
        _fail(ValueError, f"K must be {'[b, m, d]' if Q.dim() == 3 else '[m, d]'} with Q's d"
                          f"{' and b' if Q.dim() == 3 else ''}, got {tuple(K.shape)} for Q of shape {tuple(Q.shape)}")
    if Q.size(-1) < 1:
        _fail(ValueError, f"Q and K need at least one column, got {tuple(Q.shape)}")
    if key_bias is not None and tuple(key_bias.shape) != tuple(K.shape[:-1]):
        _fail(ValueError, f"key_bias must be {tuple(K.shape[:-1])} for K of shape {tuple(K.shape)}, got {tuple(key_bias.shape)}")
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        _fail(ValueError, f"k must be an integer of at least 1, got {k!r}")
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        _fail(ValueError, f"scale must be a finite number, got {scale!r}")
    if index_dtype not in (torch.int32, torch.int64):
        _fail(ValueError, f"index_dtype must be torch.int32 or torch.int64, got {index_dtype}")
    _be.operand_device(Q, K, key_bias)
    if Q.is_cuda:
        cap = _be.topk_geometry(Q.dtype)[0]
        if k > cap:
            _fail(ValueError, f"the gfx950 kernels select at most k = {cap} entries per row, got k = {k}")
    return cast(torch.Tensor, SparseTopkMM.apply(Q, K, key_bias, k, float(scale), bool(causal), bool(exclude_self), index_dtype))
