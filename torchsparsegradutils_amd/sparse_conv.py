"""Sparse convolution over a set of voxels: ``neighbor_mm`` with ``voxel_neighbors`` / ``kernel_offsets`` (no reference counterpart).

``out[i] = bias + Σ_k x[nbr[i, k]] @ w[k]``: every output row gathers at most one input row per stencil slot ``k`` and multiplies
it by that slot's matrix, shared by all rows — submanifold (``n_out = n_in``), strided (``n_out < n_in``) and transposed
(``n_out > n_in``) convolutions, and any fixed-fan-in layer with one weight per slot.  GPU operands run the implicit-GEMM MFMA
kernels of ``csrc/conv_impl.h``: the output tile stays in accumulators over all slots, nothing gathered or scattered reaches
global memory, and no pass uses atomics.  CPU operands take the torch-op path of ``_cpu.py``.

The plan of a neighbour table (``_Plan``) is built with torch ops on the table's device with no host read-back and cached per
table (storage, view, version) beside the plans of ``indexed_matmul``.  It holds the inverse table the gradient of ``x`` is
computed through, ``grad_x = neighbor_mm(grad, wᵀ, inv)``, which exists when no column of ``nbr`` sends two rows to one input.
No convolution does; such a table is refused through the package's error word (raised at once, or by ``poll_errors()`` under
``TSGU_SPTRSM_CHECK=lazy``), and so is an entry ``>= n_in``, which the kernels treat as absent.
"""

from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from . import indexed_matmul as _imm

__all__ = ["neighbor_mm", "voxel_neighbors", "kernel_offsets", "NeighborMM"]

_VALUE_DTYPES = (torch.float32, torch.float64, torch.bfloat16)
_ERR_BAD_ARG = -2


class _Plan:
    """``nbr`` (n_out, K) contiguous, ``inv`` (n_in, K) with ``inv[nbr[i, k], k] = i`` and -1 elsewhere, ``bad`` the int32 error
    word: entries >= n_in plus entries whose (input, column) another row holds as well."""

    __slots__ = ("nbr", "inv", "bad", "__weakref__")

    def __init__(self, nbr, inv, bad):
        self.nbr, self.inv, self.bad = nbr, inv, bad


def neighbor_plan(nbr: torch.Tensor, n_in: int) -> _Plan:
    n_out, K = nbr.shape
    dev = nbr.device
    nbr = nbr.contiguous()
    j = nbr.to(torch.int64)
    ok = (j >= 0) & (j < n_in)
    row = torch.arange(n_out, device=dev)[:, None].expand(n_out, K)
    slot = torch.where(ok, j * K + torch.arange(K, device=dev), n_in * K)      # absent entries share one spare slot
    inv = torch.full((n_in * K + 1,), -1, dtype=torch.int64, device=dev)
    inv.scatter_(0, slot.reshape(-1), row.reshape(-1))
    twice = ok & (inv[slot] != row)                                            # another row won this (input, column)
    bad = ((j >= n_in).sum() + twice.sum()).to(torch.int32)
    itype = nbr.dtype if n_out < 2 ** 31 else torch.int64
    return _Plan(nbr, inv[:-1].view(n_in, K).to(itype).contiguous(), bad)


def _product(x: torch.Tensor, w: torch.Tensor, table: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """bias + Σ_k x[table[:, k]] @ w[k]; w may be a transposed view."""
    if not x.is_cuda:
        return _cpu.neighbor_mm(x, w, table, bias)
    n_out, K = table.shape
    out = torch.empty((n_out, w.size(2)), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    if K == 0 or x.size(0) == 0 or x.size(1) == 0:      # bias-only: no launch
        return out.zero_() if bias is None else out.copy_(bias)
    return _be.neighbor_mm(table, _imm._rowmajor(x), _imm._b_view(w), None if bias is None else bias.contiguous(), out)


def _grad_w(plan: _Plan, x: torch.Tensor, g: torch.Tensor, shape) -> torch.Tensor:
    if not x.is_cuda:
        return _cpu.neighbor_mm_grad_w(x, g, plan.nbr)
    gw = torch.empty(shape, dtype=x.dtype, device=x.device)
    if gw.numel() == 0:
        return gw
    if x.size(0) == 0 or g.size(0) == 0:
        return gw.zero_()
    return _be.neighbor_mm_grad_w(plan.nbr, _imm._rowmajor(x), _imm._rowmajor(g), gw)


class NeighborMM(torch.autograd.Function):
    """Autograd kernel behind :func:`neighbor_mm` (once differentiable in ``x``, ``w`` and ``bias``)."""

    @staticmethod
    def forward(ctx, x, w, bias, plan):
        ctx.plan = plan
        ctx.save_for_backward(x, w)
        return _product(x, w, plan.nbr, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        plan: _Plan = ctx.plan
        grad_x = grad_w = grad_bias = None
        if ctx.needs_input_grad[0]:
            grad_x = _product(grad, w.transpose(1, 2), plan.inv, None)        # (w read through its strides: no transposed copy)
        if ctx.needs_input_grad[1]:
            grad_w = _grad_w(plan, x, grad, w.shape)
        if ctx.needs_input_grad[2]:
            grad_bias = grad.sum(0)
        return grad_x, grad_w, grad_bias, None


def neighbor_mm(x: torch.Tensor, w: torch.Tensor, nbr: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    r"""Sparse convolution as a gathered product: ``out[i] = bias + Σ_k x[nbr[i, k]] @ w[k]``.

    ``x`` (n_in, D1), ``w`` (K, D1, D2), ``nbr`` (n_out, K) int32 / int64 indices into the rows of ``x``, ``bias`` (D2,) or None,
    all on one device.  A negative entry of ``nbr`` is an absent neighbour; a row without neighbours gives ``bias`` (or zeros).
    An entry ``>= n_in`` is treated as absent and reported as an error, and so is a column of ``nbr`` that names one input twice
    (once per table).  Returns (n_out, D2) in ``x``'s dtype (fp32, fp64 or bf16; bf16 accumulates in fp32 and is rounded once).
    Differentiable once in ``x``, ``w`` and ``bias``.  :func:`voxel_neighbors` builds ``nbr`` from voxel coordinates.
    """
    if not isinstance(x, torch.Tensor) or not isinstance(w, torch.Tensor) or not isinstance(nbr, torch.Tensor):
        raise ValueError("Inputs should be instances of torch.Tensor")
    if not x.dim() == 2 or not w.dim() == 3 or not nbr.dim() == 2 or (bias is not None and not bias.dim() == 1):
        raise ValueError("Input tensors have unexpected dimensions")
    n_in, _ = x.shape
    K, D1, D2 = w.shape
    if not x.shape[1] == D1 or not nbr.shape[1] == K or (bias is not None and not bias.shape[0] == D2):
        raise ValueError("Incompatible size for inputs")
    for name, t in (("w", w), ("bias", bias)):
        if t is not None and t.dtype != x.dtype:
            raise TypeError(f"x and {name} must have the same dtype, got {x.dtype} and {t.dtype}")
    if x.dtype not in _VALUE_DTYPES:
        raise TypeError(f"unsupported value dtype {x.dtype}: expected float32, float64 or bfloat16")
    for t in (w, nbr, bias):
        if t is not None and t.device != x.device:
            raise RuntimeError(f"all operands must be on the same device, got {x.device} and {t.device}")
    idx = _imm._index(nbr, "nbr")
    plan = _imm._cached_plan("neighbor", nbr, n_in, K, x.device, lambda: neighbor_plan(idx, n_in),
                             what="neighbor_mm (nbr holds entries >= n_in, or a column that names one input twice)")
    return NeighborMM.apply(x, w, bias, plan)


# ---- neighbour tables of voxel sets --------------------------------------------------------------------------------------

def kernel_offsets(kernel_size, dilation=1, batch: bool = True) -> torch.Tensor:
    """The (K, D) int64 offsets of a box stencil in row-major order (the last axis fastest): per axis ``-(k // 2) … (k - 1) // 2``
    for an odd size ``k``, ``0 … k - 1`` for an even one, times the dilation.  An int ``kernel_size`` means three axes; ``batch``
    puts a zero column in front, for coordinates of the form (batch, …)."""
    sizes = (kernel_size,) * 3 if isinstance(kernel_size, int) else tuple(kernel_size)
    dil = (dilation,) * len(sizes) if isinstance(dilation, int) else tuple(dilation)
    if len(dil) != len(sizes) or any(int(k) < 1 for k in sizes) or not 1 <= len(sizes) + bool(batch) <= 4:
        raise ValueError(f"kernel_offsets: kernel_size {kernel_size} and dilation {dilation} do not describe a box of one to four axes")
    axes = [torch.arange(k) * d - (k // 2 * d if k % 2 else 0) for k, d in zip(map(int, sizes), map(int, dil))]
    if batch:
        axes.insert(0, torch.zeros(1, dtype=torch.int64))
    return torch.cartesian_prod(*axes).reshape(-1, len(axes))


def voxel_neighbors(coords: torch.Tensor, offsets: torch.Tensor, out_coords: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nbr[i, k]`` = the row ``j`` with ``coords[j] == out_coords[i] + offsets[k]``, -1 where there is none.

    ``coords`` (n, D) integers with D <= 4, ``offsets`` (K, D), ``out_coords`` (n_out, D) in the input's coordinate system (default:
    ``coords``).  Torch ops on ``coords``' device — linearised keys, one sort, one ``searchsorted``, one comparison — with no host
    synchronisation; duplicate rows of ``coords`` are reported through the package's error word.  Returns int32 for int32
    coordinates, else int64."""
    out_coords = coords if out_coords is None else out_coords
    if coords.dim() != 2 or offsets.dim() != 2 or out_coords.dim() != 2:
        raise ValueError("Input tensors have unexpected dimensions")
    n, D = coords.shape
    if not 1 <= D <= 4 or offsets.shape[1] != D or out_coords.shape[1] != D:
        raise ValueError("Incompatible size for inputs")
    dev = coords.device
    c, q = _imm._index(coords, "coords").to(torch.int64), _imm._index(out_coords, "out_coords").to(torch.int64)
    off = _imm._index(offsets, "offsets").to(device=dev, dtype=torch.int64)
    if q.device != dev:
        raise RuntimeError(f"all operands must be on the same device, got {dev} and {q.device}")
    otype = torch.int32 if coords.dtype == torch.int32 else torch.int64
    if n == 0:
        return torch.full((q.size(0), off.size(0)), -1, dtype=otype, device=dev)
    lo, hi = c.amin(0), c.amax(0)
    ext = hi - lo + 1
    stride = torch.cat([ext[1:], ext.new_ones(1)]).flip(0).cumprod(0).flip(0)  # row-major strides of the bounding box
    keys, perm = torch.sort(((c - lo) * stride).sum(1))
    word = (keys[1:] == keys[:-1]).sum().to(torch.int32)
    _be._defer_error_check(word, dev, "voxel_neighbors (coords holds duplicate rows)", status=_ERR_BAD_ARG)
    inside = torch.ones((q.size(0), off.size(0)), dtype=torch.bool, device=dev)
    for d in range(D):
        qd = q[:, d, None] + off[None, :, d]
        inside &= (qd >= lo[d]) & (qd <= hi[d])
    qkey = ((q - lo) * stride).sum(1)[:, None] + (off * stride).sum(1)[None, :]
    pos = torch.searchsorted(keys, qkey).clamp(max=n - 1)
    hit = inside & (keys[pos] == qkey)
    return torch.where(hit, perm[pos], -1).to(otype)
