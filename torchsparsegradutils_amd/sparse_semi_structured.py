"""2:4 semi-structured operands — ``SemiStructured``, ``sparse_semi_structured_prune``, ``sparse_semi_structured_mm`` and
``sparse_semi_structured_linear`` — with gradients on the kept entries: the layout of 2:4 sparse training (prune, multiply, gradient
on the kept values, re-prune).  The reference has no counterpart; ``torch.sparse.to_sparse_semi_structured`` has no ROCm backend and
no gradient for the kept values.

A 2:4 matrix keeps two of every four consecutive entries of a row.  ``SemiStructured`` stores the kept entries, ``values`` of shape
``(m, k/2)`` in column order, and ``meta``, an int32 tensor of shape ``(m, 4·ceil(k/128))`` with one nibble ``p0 | p1 << 2``
(``0 <= p0 < p1 <= 3``, the kept positions) per group of four.  Group ``g`` of a row (dense columns ``4g .. 4g+3``) lives, with
``stage = g // 32``, ``s = (g % 32) // 8``, ``q = (g % 8) // 2``, ``h = g % 2``, in bits ``[8s + 4h, 8s + 4h + 4)`` of word ``4·stage + q``:
word ``q`` of a stage is the position register of lane quarter ``q`` of ``v_smfmac_f32_16x16x32_bf16`` and byte ``s`` what the ``s``-th
instruction of a 128-column stage selects (``csrc/tsgu_hip_semi.h``).  Groups past ``k`` hold ``0x4``.  Read the pattern through
:meth:`SemiStructured.indices`, not through the packed words.

GPU operands run the kernels of ``csrc/semi_impl.h``: products on a dense LDS image of ``A`` with zeros at the dropped positions
(float32, float64 and, by default, bfloat16: ``TSGU_SEMI_SMFMAC=0``) or, for bfloat16 with ``TSGU_SEMI_SMFMAC=1``, on the sparse
matrix instruction, which as measured is the slower of the two in this tile layer; ``Aᵀ·G`` and the gradient of the kept values on dense tiles.  CPU operands run the torch-op path of ``_cpu.py``.  Sums are
accumulated in float32 (float64 for float64) and rounded once.

Dropped positions are not stored.  What a non-finite entry of the dense operand that faces a dropped position does is unspecified:
the expanding kernels multiply it by zero, the sparse instruction never reads it.
"""

from __future__ import annotations

import functools
import os
from typing import Optional, Tuple, cast

import torch

from . import _backend as _be
from . import _cpu

__all__ = ["SemiStructured", "sparse_semi_structured_prune", "sparse_semi_structured_mm", "sparse_semi_structured_linear"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)

# bfloat16 products on the sparse matrix instruction (1) or on the expanded image (0, the default: the faster of the two as measured,
# DESIGN.md §6): read at import, like the other switches
USE_SMFMAC = os.environ.get("TSGU_SEMI_SMFMAC", "0") == "1"


def _fail(name: str, what: str):
    raise ValueError(f"{name}: {what}")


def _once(backward):
    """`once_differentiable` that is armed always: torch's arms its error only when a cotangent requires a gradient, so a second
    differentiation through a cotangent that does not (``out.sum()``) would come back detached, silently (see sparse_topk.py)."""

    @functools.wraps(backward)
    def armed(ctx, *grads):
        with torch.no_grad():
            outs = backward(ctx, *grads)
        if not torch.is_grad_enabled():
            return outs
        outs = outs if isinstance(outs, tuple) else (outs,)
        fail = torch._C._functions.DelayedError(
            b"trying to differentiate twice a function that was marked with @once_differentiable", len(outs))
        return fail(*[None if g is None else g.detach().requires_grad_(True) for g in outs])

    return armed


# ---- the packed positions, in torch ops on either device (not a hot path: tests, the CPU path, to_dense's backward) ------------------

def _slots(k: int, device):
    """(word, shift) of every group of a row with k columns."""
    g = torch.arange(k // 4, dtype=torch.int64, device=device)
    gi = g % 32
    return 4 * (g // 32) + (gi % 8) // 2, 8 * (gi // 8) + 4 * (gi % 2)


def _unpack(meta: torch.Tensor, k: int) -> torch.Tensor:
    """Positions (m, k / 4, 2) int64 of the packed words."""
    word, shift = _slots(k, meta.device)
    nib = (meta.to(torch.int64).index_select(1, word) >> shift) & 15
    return torch.stack((nib & 3, nib >> 2), dim=-1)


def _pack(pos: torch.Tensor, k: int) -> torch.Tensor:
    """The packed int32 words (m, 4·ceil(k / 128)) of positions (m, k / 4, 2)."""
    m = pos.size(0)
    words = _be.semi_meta_words(k)
    nib = torch.full((m, 8 * words), 4, dtype=torch.int64, device=pos.device)         # the groups past k: (0, 1)
    nib[:, :k // 4] = pos[..., 0] | (pos[..., 1] << 2)
    word, shift = _slots(32 * words, pos.device)
    out = torch.zeros((m, words), dtype=torch.int64, device=pos.device)
    out.index_add_(1, word, nib << shift)
    return torch.where(out >= 2 ** 31, out - 2 ** 32, out).to(torch.int32)


class SemiStructured:
    """An ``(m, k)`` matrix, ``k % 4 == 0``, with two kept entries per aligned group of four along a row.

    ``values`` is ``(m, k/2)`` (float32, float64 or bfloat16; it may require a gradient), ``meta`` the packed positions described in
    the module's docstring.  Build one with :func:`sparse_semi_structured_prune` or :meth:`from_dense`."""

    def __init__(self, values: torch.Tensor, meta: torch.Tensor, shape: Tuple[int, int]):
        name = "SemiStructured"
        if not isinstance(values, torch.Tensor) or not isinstance(meta, torch.Tensor) or values.layout != torch.strided:
            _fail(name, "values and meta must be dense tensors")
        if len(shape) != 2:
            _fail(name, f"the shape must be (m, k), got {tuple(shape)}")
        m, k = int(shape[0]), int(shape[1])
        if k % 4:
            _fail(name, f"k must be a multiple of 4, got k = {k}")
        if values.dtype not in _DTYPES:
            _fail(name, f"values must be float32, float64 or bfloat16, got {values.dtype}")
        if tuple(values.shape) != (m, k // 2):
            _fail(name, f"values must be {(m, k // 2)} for shape {(m, k)}, got {tuple(values.shape)}")
        if meta.dtype != torch.int32 or tuple(meta.shape) != (m, _be.semi_meta_words(k)) or not meta.is_contiguous():
            _fail(name, f"meta must be a contiguous int32 tensor of shape {(m, _be.semi_meta_words(k))}, got {meta.dtype} {tuple(meta.shape)}")
        if meta.device != values.device:
            _fail(name, f"values and meta must be on one device, got {values.device} and {meta.device}")
        self.values, self.meta, self._shape = values, meta, (m, k)

    @property
    def shape(self) -> Tuple[int, int]:
        return self._shape

    @property
    def dtype(self) -> torch.dtype:
        return self.values.dtype

    @property
    def device(self) -> torch.device:
        return self.values.device

    def indices(self) -> torch.Tensor:
        """The ``(m, k/2)`` int64 columns of the kept entries, ascending along a row."""
        return _indices(self.meta, self._shape)

    def with_values(self, values: torch.Tensor) -> "SemiStructured":
        """The same pattern with other values (same shape and device; the positions are shared, not copied)."""
        return SemiStructured(values, self.meta, self._shape)

    def to_dense(self) -> torch.Tensor:
        """The dense ``(m, k)`` matrix: the kept values at their positions, ``+0`` elsewhere.  Differentiable in ``values``."""
        return cast(torch.Tensor, _Expand.apply(self.values, self.meta, self._shape))

    @staticmethod
    def from_dense(W: torch.Tensor) -> "SemiStructured":
        """:func:`sparse_semi_structured_prune` for a matrix that is 2:4 already: raises ``ValueError`` when a non-zero entry would be
        dropped.  The check reads one flag back from the device."""
        A = sparse_semi_structured_prune(W)
        with torch.no_grad():
            kept = A.values.detach().ne(0).sum()                      # NaN counts as non-zero on both sides
            if bool(W.detach().ne(0).sum() != kept):
                _fail("SemiStructured.from_dense", "the matrix is not 2:4 sparse: a group of four has more than two non-zero entries")
        return A

    def __repr__(self) -> str:
        return f"SemiStructured(shape={self._shape}, dtype={self.dtype}, device={self.device})"


def _indices(meta: torch.Tensor, shape) -> torch.Tensor:
    m, k = shape
    base = 4 * torch.arange(k // 4, dtype=torch.int64, device=meta.device)
    return (_unpack(meta, k) + base[None, :, None]).reshape(m, k // 2)


def _expand(values: torch.Tensor, meta: torch.Tensor, shape) -> torch.Tensor:
    m, k = shape
    if values.is_cuda and m and k:
        return _be.semi_expand(values, meta, k)
    return torch.zeros((m, k), dtype=values.dtype, device=values.device).scatter_(1, _indices(meta, shape), values)


class _Expand(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, meta, shape):
        ctx.meta, ctx.shape = meta, shape
        return _expand(values, meta, shape)

    @staticmethod
    @_once
    def backward(ctx, grad):  # type: ignore[override]
        return grad.gather(1, _indices(ctx.meta, ctx.shape)), None, None


class _Prune(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W):
        m, k = W.shape
        if not W.is_cuda:
            values, pos = _cpu.semi_prune(W)
            meta = _pack(pos, k)
        elif m and k:
            values, meta = _be.semi_prune(W)
        else:
            values = W.new_empty((m, k // 2))
            meta = torch.empty((m, _be.semi_meta_words(k)), dtype=torch.int32, device=W.device)
        ctx.meta, ctx.shape = meta, (m, k)
        ctx.mark_non_differentiable(meta)
        return values, meta

    @staticmethod
    @_once
    def backward(ctx, grad_values, _grad_meta):  # type: ignore[override]
        return _expand(grad_values, ctx.meta, ctx.shape)


def sparse_semi_structured_prune(W: torch.Tensor) -> SemiStructured:
    """The 2:4 operand of the dense ``(m, k)`` matrix ``W`` (float32, float64 or bfloat16, ``k % 4 == 0``).

    Per aligned group of four along a row it keeps the two entries that rank first by (``|w|`` descending, column ascending); NaN ranks
    above ``inf`` (as in :func:`sparse_topk_mm`) and ``-0`` equals ``+0``.  A matrix that is 2:4 already keeps all its non-zeros; a
    group with fewer than two non-zeros is filled with stored zeros.  The kept values are copies, bit for bit.

    Differentiable once in ``W``: the gradient of ``W`` is the gradient of the kept values at the kept positions and zero elsewhere.
    One launch on the GPU; nothing is read back from the device."""
    name = "sparse_semi_structured_prune"
    if not isinstance(W, torch.Tensor) or W.layout != torch.strided:
        _fail(name, "W must be a dense tensor")
    if W.dim() != 2:
        _fail(name, f"W must be a 2-D matrix (m, k), got {tuple(W.shape)}")
    if W.dtype not in _DTYPES:
        _fail(name, f"W must be float32, float64 or bfloat16, got {W.dtype}")
    if W.size(1) % 4:
        _fail(name, f"k must be a multiple of 4, got k = {W.size(1)}")
    values, meta = _Prune.apply(W)
    return SemiStructured(values, meta, (W.size(0), W.size(1)))


class _SemiMM(torch.autograd.Function):
    """Autograd kernel behind the two products (once differentiable).  `linear`: Y·Aᵀ (+ bias) for Y (p, k), else A·Y for Y (k, p)."""

    @staticmethod
    def forward(ctx, values, Y, bias, meta, shape, linear):
        m, k = shape
        p = Y.size(0) if linear else Y.size(1)
        if values.is_cuda and m and k and p:
            out = _be.semi_mm(values, meta, k, Y, None if bias is None else bias.contiguous(), linear, USE_SMFMAC)
        elif values.is_cuda:
            out = values.new_zeros((p, m) if linear else (m, p))
            if bias is not None:
                out = out + bias
        else:
            out = _cpu.semi_mm(values, _indices(meta, shape), k, Y, bias, linear)
        ctx.meta, ctx.shape, ctx.linear, ctx.has_bias = meta, shape, linear, bias is not None
        ctx.save_for_backward(values, Y)
        return out

    @staticmethod
    @_once
    def backward(ctx, G):  # type: ignore[override]
        values, Y = ctx.saved_tensors
        meta, linear = ctx.meta, ctx.linear
        m, k = ctx.shape
        need_v, need_y, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dv = dy = db = None
        p = Y.size(0) if linear else Y.size(1)
        if need_b:
            db = G.sum(0)
        if values.is_cuda and m and k and p:
            if need_v:
                dv = _be.semi_sddmm(meta, m, k, G, Y, linear)
            if need_y:
                dy = _be.semi_mm_t(values, meta, k, G, linear)
        elif values.is_cuda:
            dv = torch.zeros_like(values) if need_v else None
            dy = torch.zeros_like(Y) if need_y else None
        else:
            dv, dy = _cpu.semi_mm_backward(values, _indices(meta, ctx.shape), k, Y, G, linear, need_v, need_y)
        return dv, dy, db, None, None, None


def _check_pair(name: str, A, other: torch.Tensor, what: str) -> None:
    if not isinstance(A, SemiStructured):
        _fail(name, f"A must be a SemiStructured matrix, got {type(A).__name__}")
    if not isinstance(other, torch.Tensor) or other.layout != torch.strided:
        _fail(name, f"{what} must be a dense tensor")
    if not other.dtype.is_floating_point or other.dtype not in _DTYPES:
        _fail(name, f"{what} must be float32, float64 or bfloat16, got {other.dtype}")
    if other.dtype != A.dtype:
        _fail(name, f"A and {what} must have one dtype, got {A.dtype} and {other.dtype}")
    if other.device != A.device:
        _fail(name, f"A and {what} must be on one device, got {A.device} and {other.device}")


def sparse_semi_structured_mm(A: SemiStructured, B: torch.Tensor) -> torch.Tensor:
    """``A·B`` for a 2:4 ``A`` of shape ``(m, k)`` and a dense ``B`` of shape ``(k, p)`` of the same dtype and device.

    Accumulated in float32 (float64 for float64), rounded once.  Differentiable once in ``A.values`` and ``B``: the gradient of the
    kept values is ``G·Bᵀ`` at the kept positions, shape ``(m, k/2)``; the gradient of ``B`` is ``Aᵀ·G``.  A non-finite entry of ``B`` that
    faces a dropped position of ``A`` has an unspecified effect (multiplied by zero on the expanding kernels, never read by the sparse
    instruction)."""
    name = "sparse_semi_structured_mm"
    _check_pair(name, A, B, "B")
    if B.dim() != 2 or B.size(0) != A.shape[1]:
        _fail(name, f"B must be (k, p) with k = {A.shape[1]}, got {tuple(B.shape)}")
    return cast(torch.Tensor, _SemiMM.apply(A.values, B, None, A.meta, A.shape, False))


def sparse_semi_structured_linear(X: torch.Tensor, A: SemiStructured, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``X·Aᵀ (+ bias)`` for ``X`` of shape ``(..., k)`` and a 2:4 weight ``A`` of shape ``(out, k)``: the pruned-weight layer.  Leading
    dimensions of ``X`` are flattened for the product; ``bias`` is ``(out,)`` and is added before the one rounding.

    Differentiable once in ``X``, ``A.values`` and ``bias``; see :func:`sparse_semi_structured_mm` for the rules."""
    name = "sparse_semi_structured_linear"
    _check_pair(name, A, X, "X")
    out_features, k = A.shape
    if X.dim() < 1 or X.size(-1) != k:
        _fail(name, f"X must be (..., k) with k = {k}, got {tuple(X.shape)}")
    if bias is not None:
        _check_pair(name, A, bias, "bias")
        if tuple(bias.shape) != (out_features,):
            _fail(name, f"bias must be ({out_features},), got {tuple(bias.shape)}")
    out = _SemiMM.apply(A.values, X.reshape(-1, k), bias, A.meta, A.shape, True)
    return cast(torch.Tensor, out).reshape(*X.shape[:-1], out_features)
