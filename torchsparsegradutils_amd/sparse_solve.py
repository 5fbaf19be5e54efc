"""``sparse_triangular_solve`` / ``sparse_generic_solve`` — drop-in for reference
``torchsparsegradutils/sparse_solve.py`` (same signatures, validation order, messages and
autograd contract), computing on the gfx950 kernels:

* forward / adjoint triangular solves: K4 sync-free CSR sweep (``tsgu_csr_sptrsm``), replacing
  ``torch.triangular_solve`` behind reference ``_compat.py:42-48``; the transposed solve walks the
  cached transposed pattern instead of asking a library for ``op(A) = Aᵀ``.
* gradient w.r.t. the sparse operand: K3 fused SDDMM with ``alpha = -1`` (reference
  ``sparse_solve.py:216-235`` and ``:487-504``), no row-index expansion, no nnz×p gathers.
* batched inputs are solved as ONE block-diagonal sweep whose index arrays are produced by two
  vectorised adds (reference ``:173-175`` loops over the batch in Python).
"""

from __future__ import annotations

import os
import warnings
from typing import Callable, Optional, cast

import torch

from . import _backend as _be
from . import _ops
from . import _pattern as _pt
from .utils.utils import convert_coo_to_csr  # noqa: F401  (re-export parity with the reference module)


def sparse_triangular_solve(
    A: torch.Tensor,
    B: torch.Tensor,
    upper: bool = True,
    unitriangular: bool = False,
    transpose: bool = False,
) -> torch.Tensor:
    r"""Solve :math:`A x = B` (or :math:`A^\top x = B`) for sparse triangular ``A`` (COO/CSR,
    ``(m, m)`` or ``(b, m, m)``) and dense ``B`` with sparsity-preserving gradients.
    Mirrors reference ``sparse_solve.py:10-148`` (note the default ``upper=True``)."""
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

    return cast(torch.Tensor, SparseTriangularSolve.apply(A, B, upper, unitriangular, transpose))


class _TriOperand:
    """A triangular operand flattened to one 2-D row-gather plan (block diagonal if batched)."""

    __slots__ = ("plan", "values", "csr", "shape", "batch", "item_crow", "item_col", "coo_indices")

    def __init__(self, A: torch.Tensor):
        self.shape = A.shape
        self.batch = A.size(0) if A.dim() == 3 else None
        self.csr = A.layout == torch.sparse_csr
        if self.csr:
            crow, col = A.crow_indices(), A.col_indices()
            self.values = A.values().reshape(-1)
            self.item_crow, self.item_col = crow, col
            self.coo_indices = None
            if self.batch is None:
                self.plan = _pt.from_csr(A)
            else:
                self.plan = _pt.flat_block_diag(crow, col, A.size(-2), A.size(-1))
            return
        # COO → CSR ordering = coalesced (row-major sorted) order; reference convert_coo_to_csr
        # (sparse_solve.py:177-179 → utils/utils.py:349-410)
        A = A if A.is_coalesced() else A.coalesce()
        idx = A.indices()
        self.values = A.values()
        self.coo_indices = idx
        self.item_crow = self.item_col = None
        if self.batch is None:
            self.plan = _pt.from_coo_2d(idx, A.shape, coalesced=True)
        else:
            self.plan = _pt.from_coo_batched(idx, A.shape)

    def rebuild(self, grad_values: torch.Tensor) -> torch.Tensor:
        """Gradient in the caller's layout (reference sparse_solve.py:237-250)."""
        if self.csr:
            if self.batch is None:
                return torch.sparse_csr_tensor(self.plan.crow, self.plan.col, grad_values, self.shape)
            return torch.sparse_csr_tensor(
                self.item_crow, self.item_col, grad_values.view(self.batch, -1), self.shape
            )
        return torch.sparse_coo_tensor(self.coo_indices, grad_values, self.shape)


def _solve(plan: _pt.RowGather, values, rhs, upper: bool, unit: bool, transpose: bool, combined: bool = False):
    """X = op(A)^{-1} rhs on the 2-D plan (reference _compat.py:42-48 semantics).  `combined`: the value array holds BOTH triangles
    (the L \\ U array of sparse_ilu0): the sync-free sweep ignores the entries on the other side of the diagonal; the line sweep,
    whose tables are derived from the whole pattern, is not asked."""
    if not rhs.is_cuda:     # CPU operands: the legacy ATen call itself, as the reference makes it (_cpu.py)
        from . import _cpu

        return _cpu.sptrsm(plan, values, rhs, upper, unit, transpose)
    lower = upper if transpose else not upper        # (transposed: rows of Aᵀ; the selected triangle flips side)
    tables = None if combined else _lattice_tables(plan, values, rhs, lower, transpose)
    if tables is not None:
        # a stencil factor on a lattice: the line sweep (csrc/sptrsm_lattice.hip) — the same bits, no wall-clock trial, and the
        # transposed solve walks A's own arrays (no transposed pattern is built for it)
        return _be.csr_sptrsm_lattice(tables, values, rhs, plan.n_rows, lower=lower, unit=unit, workgroups=TRSM_LATTICE_WORKGROUPS)
    pt = plan.transposed if transpose else plan

    def run(wg_per_cu):
        return _be.csr_sptrsm(pt.crow, pt.col, values, rhs, pt.n_rows, lower=lower, unit=unit, perm=pt.perm, wg_per_cu=wg_per_cu)

    return run(_sweep_width(pt, lower, unit, rhs, run))


# Line sweep for factors whose pattern is a stencil on a row-major lattice (what PairwiseEncoder emits; truncated 7- / 27-point
# factors): one wave per z-line instead of one ticket and one pointer chase per row.  The solution is the same bits either way.
# OFF by default (TSGU_ENABLE_TRSM_LATTICE=1 switches it on; the master switch TSGU_ENABLE_LATTICE=0 switches it off too): on the
# flagship factor (64³ lattice, 8 columns) it measured 1.02-1.06x the sync-free sweep, not the 2x that was the bar for making it the
# default; on lattices with long z-lines (15 x 17 x 1024) it is 4.9x faster (EXPERIMENTS.md §13).
# TSGU_TRSM_LATTICE_CFG = persistent workgroups of the sweep (experiments; 0 = the kernel's rule).
ENABLE_TRSM_LATTICE = os.environ.get("TSGU_ENABLE_TRSM_LATTICE", "0") == "1"
TRSM_LATTICE_WORKGROUPS = int(os.environ.get("TSGU_TRSM_LATTICE_CFG", "0") or 0)
TRSM_LATTICE_DTYPES = (torch.float32, torch.float64)
TRSM_LATTICE_MAX_COLUMNS = 64


def _lattice_tables(plan: _pt.RowGather, values, rhs, lower: bool, transpose: bool):
    """Tables of the line sweep for this solve, or None: the switch, the operands the kernel takes (fp32 / fp64, one column tile),
    then the pattern (`_ops._lattice_plan`: GPU operands, square, stored order, nnz >= PACK_MIN_NNZ, never first seen inside a stream
    capture; `_lattice.trsm_tables`: the used entries reach back along the sweep without wrapping)."""
    if not ENABLE_TRSM_LATTICE or values.dtype not in TRSM_LATTICE_DTYPES or rhs.dtype != values.dtype:
        return None
    if rhs.dim() != 2 or not 1 <= rhs.size(-1) <= TRSM_LATTICE_MAX_COLUMNS or values.numel() != plan.nnz:
        return None
    lp = _ops._lattice_plan(plan, transposed=transpose)
    if lp is None:
        return None
    if lp._trsm is None and torch.cuda.is_current_stream_capturing():
        return None          # (the tables are derived with one device reduction and a host read)
    return _ops._lt.trsm_tables(lp, lower)


# Persistent workgroups per CU of the sync-free sweep: a measured choice per (pattern, triangle, width), made at the pattern's
# third solve.  Deep dependency chains (C3: 2 673 levels) are fastest with ONE workgroup per CU — every extra polling wave lengthens
# the hop; shallow patterns (the reference's published shape, benchmarks/sparse_triangular_solve_rand.py: one random off-diagonal
# entry per row) are bound by the rows in flight and want all eight.  The solution does not depend on it (every row sums its own
# entries in a fixed order), so the choice is speed only; TSGU_SPTRSM_TUNE=0 keeps one workgroup per CU.  The trial is a ONE-OFF host
# synchronisation inside that third forward solve (12 extra solves, each awaited); it is skipped under
# torch.use_deterministic_algorithms (nothing is chosen by a wall clock there — as for the lattice configurations, _ops._lattice_cfg)
# and inside a stream capture.
SWEEP_TUNE = os.environ.get("TSGU_SPTRSM_TUNE", "1") != "0"
SWEEP_TUNE_AFTER = 2
SWEEP_WIDTHS = (1, 2, 4, 8)


def _sweep_width(pt: _pt.RowGather, lower: bool, unit: bool, rhs: torch.Tensor, run) -> int:
    if not SWEEP_TUNE or pt.n_rows < 4096 or torch.are_deterministic_algorithms_enabled():
        return 1
    memo = pt.core.own.get("sweep_width")
    if memo is None:
        memo = pt.core.own["sweep_width"] = {}
    key = (bool(lower), bool(unit), rhs.dtype, rhs.size(-1))
    got = memo.get(key)
    if isinstance(got, int) and got > 0:
        return got
    seen = memo[key] = (got or 0) - 1          # (negative: solves seen so far)
    if -seen <= SWEEP_TUNE_AFTER or torch.cuda.is_current_stream_capturing():
        return 1
    if _pt.plans_in_flight():
        # a plan build is running on the worker's side stream (device sorts): trial timings taken beside it picked 2 or 4 workgroups
        # per CU where 8 is twice as fast (the published shape's backward: 0.27 ms or 0.44 ms from run to run) — try again next solve
        return 1
    best, best_ms = 1, None
    for w in SWEEP_WIDTHS:
        run(w)
        ts = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(w)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        if best_ms is None or min(ts) < 0.95 * best_ms:      # (a wider sweep has to win by 5 %: ties keep the fewer polling waves)
            best, best_ms = w, min(ts)
    memo[key] = best
    return best


class SparseTriangularSolve(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_triangular_solve` (reference ``sparse_solve.py:151-252``)."""

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
        ctx.csr = op.csr
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

        # gradB = op(A)^{-T} grad   (reference :202-204)
        gradB = _solve(plan, values, grad, ctx.upper, ctx.unitriangular, not ctx.transpose)

        if ctx.unitriangular is True and plan.has_diagonal:  # reference :230-231
            raise ValueError("First input should be strictly triangular (i.e. unit diagonals is implicit)")

        # gradA[k] = -<gradB[i,:], x[j,:]>, roles swapped for the transposed solve (reference :223-235)
        gvals = _ops.sddmm(plan, gradB, x, alpha=-1.0, swap_roles=bool(ctx.transpose))
        if plan.perm is not None:  # cannot happen for coalesced inputs; kept for safety
            out = torch.empty_like(gvals)
            out[plan.perm] = gvals
            gvals = out
        gradA = op.rebuild(gvals)
        if ctx.batch_size is not None:
            gradB = gradB.view(ctx.B_shape)
        return gradA, gradB, None, None, None


def sparse_generic_solve(
    A: torch.Tensor,
    B: torch.Tensor,
    solve: Optional[Callable[..., torch.Tensor]] = None,
    transpose_solve: Optional[Callable[..., torch.Tensor]] = None,
    **kwargs,
) -> torch.Tensor:
    r"""Solve :math:`A x = B` with an iterative ``solve(A, B, **kwargs)`` and sparsity-preserving
    gradients via the implicit function theorem.  ``A``: sparse COO/CSR ``(n, n)``; ``B``: dense
    ``(n,)`` or ``(n, k)``.  Defaults: both solvers ``None`` → ``minres``; one ``None`` → mirrored.
    Mirrors reference ``sparse_solve.py:255-424``.  For a nonsymmetric ``A`` the backward needs a solve with :math:`A^T`:
    pass the pair ``solve=gmres, transpose_solve=gmres_t`` (``utils/gmres.py``); ``solve=gmres`` alone is mirrored to the
    same solver, which is right only for symmetric ``A``."""
    if not isinstance(A, torch.Tensor) or not isinstance(B, torch.Tensor):
        raise ValueError("Both A and B should be instances of torch.Tensor")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise TypeError(f"Unsupported sparse layout: {A.layout}. Only COO and CSR are supported.")
    if A.dim() != 2:
        raise ValueError("A must be a 2D tensor")
    if A.shape[0] != A.shape[1]:
        raise ValueError("A must be square")
    if B.dim() not in (1, 2):
        raise ValueError("B must be a 1D or 2D tensor")
    if B.shape[0] != A.shape[0]:
        raise ValueError(f"Incompatible dimensions: A has shape {tuple(A.shape)}, B has shape {tuple(B.shape)}")
    if B.layout != torch.strided:
        raise TypeError("B must be a dense (strided) tensor")
    if A.dtype != B.dtype:
        warnings.warn(
            f"A and B have different dtypes: A={A.dtype}, B={B.dtype}. This may affect solver behavior.",
            UserWarning,
            stacklevel=2,
        )

    if solve is None and transpose_solve is None:
        from .utils import minres

        solve = minres
        transpose_solve = minres
    elif solve is None:
        solve = transpose_solve
    elif transpose_solve is None:
        transpose_solve = solve

    X = cast(torch.Tensor, SparseGenericSolve.apply(A, B, solve, transpose_solve, kwargs))

    if B.dim() == 1 and X.dim() == 2 and X.shape[1] == 1:
        X = X.squeeze(-1)
    elif B.dim() == 2 and X.dim() == 1:
        X = X.unsqueeze(-1)
    return X


class _MaskedOuter(torch.autograd.Function):
    """vals[k] = alpha·<G[row k,:], X[col k,:]> on a fixed pattern, differentiable in G and X so
    that ``SparseGenericSolve.backward`` supports ``create_graph=True`` (reference tests
    ``test_sparse_solve.py:391-484``; the reference gets this from differentiable index_select/mul/sum)."""

    @staticmethod
    def forward(ctx, G, X, plan, alpha):
        ctx.plan, ctx.alpha = plan, alpha
        ctx.save_for_backward(G, X)
        return _ops.sddmm(plan, G.detach(), X.detach(), alpha=alpha)

    @staticmethod
    def backward(ctx, gout):  # type: ignore[override]
        G, X = ctx.saved_tensors
        plan = ctx.plan
        w = (gout * ctx.alpha).contiguous()
        dG = dX = None
        if ctx.needs_input_grad[0]:  # dG[i,:] = Σ_k∈row i w[k]·X[col k,:]
            dG = _ops.spmm(plan, w, X.detach())
        if ctx.needs_input_grad[1]:  # dX[j,:] = Σ_k: col k = j  w[k]·G[row k,:]
            dX = _ops.spmm_t(plan, w, G.detach())
        return dG, dX, None, None


class SparseGenericSolve(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_generic_solve` (reference ``sparse_solve.py:427-519``)."""

    @staticmethod
    def forward(ctx, A, B, solve, transpose_solve, kwargs):
        grad_flag = A.requires_grad or B.requires_grad
        ctx.solve = solve
        ctx.transpose_solve = transpose_solve
        ctx.kwargs = kwargs

        x = solve(A.detach(), B.detach(), **kwargs)
        if x.dtype != A.dtype:
            x = x.to(dtype=A.dtype)
        x.requires_grad = grad_flag
        ctx.save_for_backward(A, x)
        return x

    @staticmethod
    def backward(ctx, grad):  # type: ignore[override]
        A, x = ctx.saved_tensors
        is_vector = x.ndim == 1
        if is_vector:
            x = x.unsqueeze(-1)
            grad = grad.unsqueeze(-1)

        # gradB = A^{-T} grad through the (swapped) user solvers; stays differentiable (reference :465-471)
        gradB = sparse_generic_solve(A, grad, solve=ctx.transpose_solve, transpose_solve=ctx.solve, **ctx.kwargs)
        if gradB.dtype != A.dtype:
            gradB = gradB.to(dtype=A.dtype)

        if A.layout == torch.sparse_coo:
            Ac = A.coalesce()
            idx = Ac.indices()
            plan = _pt.from_coo_2d(idx, A.shape, coalesced=True)
        else:
            idx = None
            plan = _pt.from_csr(A)

        # gradA[k] = -<gradB[i,:], x[j,:]>   (reference :487-504)
        gvals = _MaskedOuter.apply(gradB, x, plan, -1.0)
        if gvals.dtype != A.dtype:
            gvals = gvals.to(dtype=A.dtype)
        if idx is not None:
            gradA = torch.sparse_coo_tensor(idx, gvals, A.shape)
        else:
            gradA = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), gvals, A.shape)

        if is_vector:
            gradB = gradB.squeeze(-1)
        return gradA, gradB, None, None, None
