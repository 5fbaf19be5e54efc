"""``sparse_fsai`` — the factorised sparse approximate inverse preconditioner (FSAI; Kolotilina and Yeremin, 1993).

For a symmetric positive definite ``A`` and a lower-triangular pattern ``S``, FSAI computes the sparse lower-triangular ``G`` on
``S`` that minimises ``‖I − G·L‖_F`` over that pattern (``L`` the exact Cholesky factor, which is never formed) and scales it so
that ``diag(G·A·Gᵀ) = 1``.  Then ``G·A·Gᵀ ≈ I`` and ``M⁻¹ = Gᵀ·G`` is symmetric positive definite: the preconditioner is APPLIED
WITH TWO SPARSE PRODUCTS — no triangular solve, no dependency chain, no host synchronisation — which is what the incomplete
factorisations of ``sparse_factor`` cannot offer next to a 0.1 ms Krylov step.  The reference package has no counterpart.

Row ``i`` of ``G`` needs one small dense SPD solve with ``A[J, J]``, ``J`` the columns ``S`` stores in row ``i``: the rows are
independent, and the build is one launch of ``csrc/fsai_impl.h`` (C ABI in ``include/tsgu_hip_fsai.h``) in which a group of 8, 16,
32 or 64 lanes owns a row.  Everything about the pattern (the check, the lower triangle, the row order by size, the transposed
pattern of ``Gᵀ``) is a plan cached with it (``_pattern.fsai_plan``).

No gradient flows through ``G``: the function runs under ``no_grad`` on the detached operand, for the reasons given in
``sparse_factor``'s docstring — a preconditioner changes how fast a Krylov loop reaches the solution, not the solution.

CPU operands are served by a plain row-by-row loop (``_cpu.csr_fsai``: the same semantics, reference speed only).
"""

from __future__ import annotations

import torch

from . import _backend as _be
from . import _pattern as _pt
from .sparse_factor import _Factor, _operand
from .sparse_matmul import sparse_mm

__all__ = ["sparse_fsai", "SparseFSAI"]


def _pattern_gather(pattern: torch.Tensor, A: torch.Tensor) -> _pt.RowGather:
    """The row-gather plan of the tensor that carries S, after the refusals."""
    if not isinstance(pattern, torch.Tensor) or pattern.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError("sparse_fsai: pattern should be a sparse tensor in either COO or CSR format")
    if tuple(pattern.shape) != tuple(A.shape):
        raise ValueError(f"sparse_fsai: pattern must have the shape of A, got {tuple(pattern.shape)} and {tuple(A.shape)}")
    if pattern.device != A.device:
        raise ValueError(f"sparse_fsai: pattern must be on the device of A, got {pattern.device} and {A.device}")
    pattern = pattern.detach()
    if pattern.layout == torch.sparse_csr:
        return _pt.from_csr(pattern)
    pattern = pattern if pattern.is_coalesced() else pattern.coalesce()
    return _pt.from_coo_2d(pattern.indices(), pattern.shape, coalesced=True)


class SparseFSAI(_Factor):
    r"""``M⁻¹ = Gᵀ·G`` with ``G`` lower triangular on the pattern ``S`` and ``diag(G·A·Gᵀ) = 1``.

    ``values``  the values of ``G`` on the lower CSR pattern (``crow_indices``, ``col_indices``: ascending columns, the diagonal
                closes every row)
    ``M(R)`` / ``M.solve(R, transpose=False)`` / ``M.matmul(R)``  ``Gᵀ·(G·R)`` for ``R`` of shape ``(n,)`` or ``(n, p)``: two
                sparse products, each on a CSR tensor of its own, so that stencil patterns reach the plane-march kernels.  ``M`` is
                symmetric: ``transpose`` changes nothing, and ``M.T`` is ``M``.  The result is detached.
    ``G``       the CSR lower factor
    ``GT``      the CSR upper factor ``Gᵀ``, built on first use (one ``index_select`` of ``values`` through the cached permutation)
    ``info``    0, or 1 + the lowest row whose local matrix was not positive definite (a device tensor until someone reads it)"""

    def __init__(self, gather: _pt.RowGather, values: torch.Tensor, info: torch.Tensor, shape):
        self._gather, self.values, self.info, self.shape = gather, values, info, tuple(shape)
        self._G = self._GT = None

    @property
    def crow_indices(self):
        return self._gather.crow

    @property
    def col_indices(self):
        return self._gather.col

    @property
    def G(self) -> torch.Tensor:
        if self._G is None:
            self._G = torch.sparse_csr_tensor(self._gather.crow, self._gather.col, self.values, self.shape)
        return self._G

    @property
    def GT(self) -> torch.Tensor:
        if self._GT is None:
            t = self._gather.transposed
            self._GT = torch.sparse_csr_tensor(t.crow, t.col, self.values.index_select(0, t.perm.to(torch.int64)), self.shape)
        return self._GT

    @property
    def T(self) -> "SparseFSAI":
        return self

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        return self._apply(R, (lambda X: sparse_mm(self.G, X), lambda X: sparse_mm(self.GT, X)))

    matmul = solve


def sparse_fsai(A: torch.Tensor, *, pattern: torch.Tensor = None, check: bool = True) -> SparseFSAI:
    r"""The FSAI preconditioner of a square sparse ``A`` (COO or CSR, float32 / float64), meant for symmetric positive definite ``A``.

    Only ``tril(A)`` is read; symmetry is not checked.  ``pattern=None`` builds ``G`` on the pattern of ``tril(A)``.  Otherwise
    ``pattern`` is a sparse COO or CSR tensor of ``A``'s shape on ``A``'s device whose stored lower-triangular positions are ``S``;
    its values and its upper triangle are ignored.  A wider pattern buys fewer Krylov iterations for a costlier build and
    application: ``pattern=sparse_spgemm(A, A)`` gives ``S = tril(A²)``, one more product ``tril(A³)``.  ``S`` must store every
    diagonal entry and no column twice per row (``ValueError`` naming the first offending row), and no row of ``S`` may be longer
    than ``_backend.fsai_geometry(dtype)[0]`` entries (``ValueError`` naming the row: a row of ``m`` entries costs ``m³``).

    For row ``i`` with ``J = cols_S(i)``: ``A[J,J]·y = e_m``, ``g_i = y / sqrt(y_m)``.  For SPD ``A`` this exists for every ``S``;
    a row whose local matrix is not positive definite is finished in IEEE arithmetic without touching any other row.
    ``check=True`` reads the breakdown word (one synchronisation) and raises
    ``RuntimeError("sparse_fsai: local matrix not positive definite in row r")``; ``check=False`` leaves ``.info`` on the device.
    Two calls give the same bits.  No gradient flows through ``G`` (see the module's docstring).

    The result is what ``linear_cg(preconditioner=…)``, ``minres(preconditioner=…)`` and ``BICGSTABSettings.precon`` take."""
    with torch.no_grad():
        g, values = _operand(A, "sparse_fsai")
        capacity = _be.fsai_geometry(values.dtype)[0]
        a_plan = _pt.factor_plan(g)
        a_lower, a_pos, _ = a_plan.lower()
        s_plan = _pt.fsai_plan(g if pattern is None else _pattern_gather(pattern, A), capacity)
        s_lower, order = s_plan.view(a_lower.crow.dtype)
        a_val = a_plan.canonical_values(values).index_select(0, a_pos)
        if values.is_cuda:
            out, info = _be.csr_fsai(a_lower.crow, a_lower.col, a_val, s_lower.crow, s_lower.col, s_lower.n_rows, order=order)
        else:
            from . import _cpu

            out, info = _cpu.csr_fsai(a_lower.crow, a_lower.col, a_val, s_lower.crow, s_lower.col, s_lower.n_rows)
    if check:
        row = int(info.item())
        if row:
            raise RuntimeError(f"sparse_fsai: local matrix not positive definite in row {row - 1}")
    return SparseFSAI(s_lower, out, info, A.shape)
