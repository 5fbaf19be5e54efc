"""Segmented and gathered dense products: ``segment_mm`` / ``gather_mm`` (reference ``torchsparsegradutils/indexed_matmul.py``).

Both are one operation: the rows of ``a`` are grouped into segments, and segment r is multiplied by ``b[r]``.  A plan holds the
grouping (``_Plan``): for ``segment_mm`` the segments are the consecutive row ranges of ``seglen_a``; for ``gather_mm`` a
stable sort of ``idx_b`` (``perm``) brings the rows of one relation together.  Plans are built with torch ops on the index
tensor's device, on the current stream and with no host read-back, and cached per index tensor (storage, view, version),
so a layer that reuses one index tensor builds its plan once.  GPU operands run the MFMA kernels of
``csrc/indexed_mm_impl.h``; CPU operands the torch-op path of ``_cpu.py``.

Deviations from the reference, each where it raises or returns garbage: the output has ``a``'s dtype (fp64 and bf16
``gather_mm`` compute instead of raising), ``N = 0`` gives an empty ``(0, D2)`` result, and a ``gather_mm`` row whose index
lies outside ``[0, R)`` is written as zeros, has a zero gradient and adds nothing to ``grad_b``; it is reported through the
package's error word (raised at once, or by ``poll_errors()`` under ``TSGU_SPTRSM_CHECK=lazy``), once per index tensor.
"""

from __future__ import annotations

import threading
import weakref
from collections import OrderedDict
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from .sparse_logsumexp import _nested_supported

__all__ = ["segment_mm", "gather_mm", "SegmentMM", "GatherMM"]

_VALUE_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
TILE_ROWS = _be.SEGMENT_MM_TILE_ROWS
_ERR_BAD_ARG = -2


class _Plan:
    """Row grouping of one index tensor for n rows and n_seg matrices (see include/tsgu_hip.h, tsgu_segment_mm):
    ``offsets`` / ``tile_ptr`` [n_seg + 3], ``perm`` [n] or None (identity), all of one integer dtype on the operands' device;
    ``bad`` the int32 error word (rows of an index outside [0, n_seg), or negative lengths)."""

    __slots__ = ("offsets", "tile_ptr", "perm", "n", "n_seg", "max_tiles", "bad", "_chunks", "_host", "__weakref__")

    def __init__(self, offsets, tile_ptr, perm, n: int, n_seg: int, bad):
        self.offsets, self.tile_ptr, self.perm = offsets, tile_ptr, perm
        self.n, self.n_seg, self.bad = n, n_seg, bad
        self.max_tiles = -(-n // TILE_ROWS) + min(n_seg, n) + 2
        self._chunks = {}
        self._host = None

    def bounds(self):
        """Host list of the n_seg + 1 real segment boundaries (CPU plans: no device read-back)."""
        if self._host is None:
            self._host = self.offsets[1:self.n_seg + 2].tolist()
        return self._host

    def perm64(self):
        return None if self.perm is None else self.perm.to(torch.int64)

    def chunks(self, chunk: int):
        """(chunk_ptr, part_ptr) [n_seg + 1] of tsgu_segment_mm_grad_b for chunks of `chunk` rows (device ops, cached)."""
        got = self._chunks.get(chunk)
        if got is None:
            off = self.offsets.to(torch.int64)
            nch = (off[2:self.n_seg + 2] - off[1:self.n_seg + 1] + (chunk - 1)) // chunk
            zero = torch.zeros(1, dtype=torch.int64, device=off.device)
            chunk_ptr = torch.cat([zero, torch.cumsum(nch, 0)]).to(self.offsets.dtype)
            part_ptr = torch.cat([zero, torch.cumsum(torch.where(nch > 1, nch, 0), 0)]).to(self.offsets.dtype)
            got = self._chunks[chunk] = (chunk_ptr, part_ptr)
        return got


def _plan_from_bounds(bounds: torch.Tensor, perm, n: int, n_seg: int, bad, dev: torch.device) -> _Plan:
    """bounds: int64 [n_seg + 1], the first position of each real segment and the end of the last one."""
    itype = torch.int32 if n + 2 * TILE_ROWS < 2 ** 31 else torch.int64
    edge = torch.tensor([0, n], dtype=torch.int64, device=bounds.device)
    ext = torch.cat([edge[:1], bounds, edge[1:]])
    tiles = (ext[1:] - ext[:-1] + (TILE_ROWS - 1)) // TILE_ROWS
    tile_ptr = torch.cat([edge[:1], torch.cumsum(tiles, 0)])
    offsets, tile_ptr = ext.to(itype), tile_ptr.to(itype)
    if offsets.device != dev:   # seglen on the host (the usual convention): one copy of each word array
        offsets, tile_ptr = offsets.to(dev, non_blocking=True), tile_ptr.to(dev, non_blocking=True)
    if perm is not None:
        perm = perm.to(itype)
    return _Plan(offsets, tile_ptr, perm, n, n_seg, bad)


def gather_plan(idx: torch.Tensor, n_seg: int) -> _Plan:
    """Stable sort of idx (int32 / int64), relation boundaries by searchsorted; out-of-range rows sort to both ends."""
    n = idx.numel()
    sorted_idx, perm = torch.sort(idx, stable=True)
    bounds = torch.searchsorted(sorted_idx, torch.arange(n_seg + 1, dtype=idx.dtype, device=idx.device))
    bad = (bounds[0] + (n - bounds[n_seg])).to(torch.int32)
    return _plan_from_bounds(bounds, perm, n, n_seg, bad, idx.device)


def segment_plan(seglen: torch.Tensor, n: int, dev: torch.device) -> _Plan:
    """torch.tensor_split's rule: boundaries 0, cumsum(seglen[:-1]) clamped to n, n (the last length is never read)."""
    n_seg = seglen.numel()
    sl = seglen.to(torch.int64)
    bad = (sl < 0).sum().to(torch.int32)
    cs = torch.cumsum(sl.clamp(min=0)[:-1], 0).clamp(max=n)
    edge = torch.tensor([0, n], dtype=torch.int64, device=sl.device)
    bounds = torch.cat([edge[:1], cs, edge[1:]]) if n_seg > 0 else edge[:1]
    return _plan_from_bounds(bounds, None, n, n_seg, bad, dev)


# key -> _Plan, keyed like _pattern keys index tensors; evicted when the index storage dies or by LRU
_PLANS: "OrderedDict[tuple, _Plan]" = OrderedDict()
_PLANS_LOCK = threading.RLock()
_PLANS_MAX = 16
STATS = {"built": 0}


def _key(kind: str, t: torch.Tensor, n: int, n_seg: int, dev: torch.device) -> tuple:
    return (kind, n, n_seg, dev, t.untyped_storage()._cdata, t.storage_offset(), t.shape, t.stride(), t.dtype, t._version,
            t.device)


def _evict(key) -> None:
    with _PLANS_LOCK:
        _PLANS.pop(key, None)


def _cached_plan(kind: str, idx: torch.Tensor, n: int, n_seg: int, dev: torch.device, build) -> _Plan:
    key = _key(kind, idx, n, n_seg, dev)
    with _PLANS_LOCK:
        plan = _PLANS.get(key)
        if plan is not None:
            _PLANS.move_to_end(key)
            return plan
    plan = build()
    STATS["built"] += 1
    what = ("gather_mm (idx_b holds indices outside [0, R))" if kind == "gather"
            else "segment_mm (seglen_a holds negative lengths)")
    _be._defer_error_check(plan.bad, plan.bad.device, what, status=_ERR_BAD_ARG)   # (sync mode: a bad plan is not cached)
    with _PLANS_LOCK:
        _PLANS[key] = plan
        weakref.finalize(idx.untyped_storage(), _evict, key)
        while len(_PLANS) > _PLANS_MAX:
            _PLANS.popitem(last=False)
    return plan


def clear_plans() -> None:
    with _PLANS_LOCK:
        _PLANS.clear()


# ---- the products -------------------------------------------------------------------------------------------------------

def _rowmajor(t: torch.Tensor) -> torch.Tensor:
    return t if (t.stride(-1) == 1 or t.size(-1) <= 1) and (t.size(0) <= 1 or t.stride(0) >= t.size(1)) else t.contiguous()


def _b_view(b: torch.Tensor) -> torch.Tensor:
    return b if b.stride(2) == 1 or b.stride(1) == 1 else b.contiguous()


def _product(plan: _Plan, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """out[perm[i]] = a[perm[i]] @ b[r] for i in segment r, zeros for rows of no segment; b may be a transposed view."""
    n, d2 = a.size(0), b.size(2)
    if not a.is_cuda:
        return _cpu.segment_mm(plan.bounds(), plan.perm64(), a, b)
    out = torch.empty((n, d2), dtype=a.dtype, device=a.device)
    if n == 0 or d2 == 0:
        return out
    return _be.segment_mm(plan, _rowmajor(a), _b_view(b), out)


def _grad_b(plan: _Plan, a: torch.Tensor, g: torch.Tensor, b_shape) -> torch.Tensor:
    if not a.is_cuda:
        return _cpu.segment_mm_grad_b(plan.bounds(), plan.perm64(), a, g, plan.n_seg)
    gb = torch.empty(b_shape, dtype=a.dtype, device=a.device)
    if gb.numel() == 0:
        return gb
    if a.size(0) == 0:
        return gb.zero_()
    return _be.segment_mm_grad_b(plan, _rowmajor(a), _rowmajor(g), gb)


class _IndexedMatMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, plan):
        ctx.plan = plan
        ctx.save_for_backward(a, b)
        return _product(plan, a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        a, b = ctx.saved_tensors
        plan: _Plan = ctx.plan
        grad_a = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_a = _product(plan, grad, b.transpose(1, 2))      # (b read through its strides: no transposed copy)
        if ctx.needs_input_grad[1]:
            grad_b = _grad_b(plan, a, grad, b.shape)
        return grad_a, grad_b, None


class SegmentMM(_IndexedMatMul):
    """Autograd kernel behind :func:`segment_mm` (once differentiable in ``a`` and ``b``)."""


class GatherMM(_IndexedMatMul):
    """Autograd kernel behind :func:`gather_mm` (once differentiable in ``a`` and ``b``)."""


# ---- validation and the public functions --------------------------------------------------------------------------------

def _check_values(a: torch.Tensor, b: torch.Tensor) -> None:
    if a.dtype != b.dtype:
        raise TypeError(f"a and b must have the same dtype, got {a.dtype} and {b.dtype}")
    if a.dtype not in _VALUE_DTYPES:
        raise TypeError(f"unsupported value dtype {a.dtype}: expected float32, float64 or bfloat16")
    if a.device != b.device:
        raise RuntimeError(f"all operands must be on the same device, got {a.device} and {b.device}")


def _index(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor, got {t.dtype}")
    return t if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64)


def segment_mm(a: torch.Tensor, b: torch.Tensor, seglen_a: torch.Tensor) -> torch.Tensor:
    r"""Segmented matrix product: ``a[s_r:s_{r+1}] @ b[r]`` for each segment r, concatenated in row order.

    ``a`` (N, D1), ``b`` (R, D1, D2), ``seglen_a`` (R,) integer lengths, on ``a``'s device or on the CPU.  The boundaries
    follow the reference's ``tensor_split``: ``0, cumsum(seglen_a[:-1])`` clamped to N, then N, so the last length is never
    read and rows beyond the first R - 1 segments belong to the last one.  Returns (N, D2) in ``a``'s dtype (fp32, fp64 or
    bf16; bf16 accumulates in fp32).  Differentiable once in ``a`` and ``b``.
    """
    if not _nested_supported():
        raise NotImplementedError("PyTorch version is too old for nested tensors")
    if not a.dim() == 2 or not b.dim() == 3 or not seglen_a.dim() == 1:
        raise ValueError("Input tensors have unexpected dimensions")
    N, _ = a.shape
    R, D1, D2 = b.shape
    if not a.shape[1] == D1 or not seglen_a.shape[0] == R:
        raise ValueError("Incompatible size for inputs")
    _check_values(a, b)
    if seglen_a.device != a.device and seglen_a.device.type != "cpu":
        raise RuntimeError(f"all operands must be on the same device, got {a.device} and {seglen_a.device}")
    seglen = _index(seglen_a, "seglen_a")
    if seglen.device.type == "cpu" and bool((seglen < 0).any()):
        raise ValueError("seglen_a must not hold negative lengths")
    plan = _cached_plan("segment", seglen_a, N, R, a.device, lambda: segment_plan(seglen, N, a.device))
    return SegmentMM.apply(a, b, plan)


def gather_mm(a: torch.Tensor, b: torch.Tensor, idx_b: torch.Tensor) -> torch.Tensor:
    r"""Per-row indexed matrix product: ``out[i] = a[i] @ b[idx_b[i]]``.

    ``a`` (N, D1), ``b`` (R, D1, D2), ``idx_b`` (N,) integer indices, all on one device.  Returns (N, D2) in ``a``'s dtype
    (fp32, fp64 or bf16; bf16 accumulates in fp32).  A row whose index lies outside ``[0, R)`` is zero, has a zero gradient
    and is reported as an error (once per index tensor).  Differentiable once in ``a`` and ``b``.
    """
    if not _nested_supported():
        raise NotImplementedError("PyTorch version is too old for nested tensors")
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or not isinstance(idx_b, torch.Tensor):
        raise ValueError("Inputs should be instances of torch.Tensor")
    if not a.dim() == 2 or not b.dim() == 3 or not idx_b.dim() == 1:
        raise ValueError("Input tensors have unexpected dimensions")
    N = idx_b.shape[0]
    R, D1, D2 = b.shape
    if not a.shape[0] == N or not a.shape[1] == D1:
        raise ValueError("Incompatible size for inputs")
    _check_values(a, b)
    if idx_b.device != a.device:
        raise RuntimeError(f"all operands must be on the same device, got {a.device} and {idx_b.device}")
    idx = _index(idx_b, "idx_b")
    plan = _cached_plan("gather", idx_b, N, R, a.device, lambda: gather_plan(idx, R))
    return GatherMM.apply(a, b, plan)
