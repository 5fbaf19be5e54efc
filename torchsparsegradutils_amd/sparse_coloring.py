"""``sparse_coloring`` — a multicolour ordering of a sparse matrix, and the preconditioners that stand on it: the coloured forms of
``sparse_ilu0`` / ``sparse_ic0`` and the symmetric Gauss–Seidel preconditioner ``sparse_sgs``.

In the natural ordering a triangular solve with an incomplete factor is a chain of dependent rows: the sync-free sweep of
``sparse_triangular_solve`` is bound by the rows in flight, and on a 2 M-row stencil an application costs hundreds of Krylov
steps.  A multicolour ordering numbers the rows so that no two rows of one colour are coupled.  In that ordering a
triangular solve is ONE wait-free launch per colour — no tickets, no flags, no polls, no error word — of about ``1/n_colors`` of
the rows each, and an application can be captured in a graph.  The price is paid in iterations: the coloured factors are weaker
than the natural ones (DESIGN.md §4 has the measurements).

The colouring is a pure function of the pattern.  The neighbours of ``i`` are the ``j ≠ i`` with ``(i, j)`` or ``(j, i)`` stored;
node ``i`` has the key ``(lowbias32(i), i)``; the nodes are visited in descending key and each takes the smallest colour no
coloured neighbour holds.  The kernels reach that result by rounds (``csrc/color_impl.h``, C ABI in ``csrc/tsgu_hip_color.h``); for
CPU operands the torch-op forms of ``_cpu.py`` run under the same Python code.  Everything else about the ordering is a plan
cached with the pattern (``_pattern.coloring_plan``).

No gradient flows through the preconditioners, for the reasons given in ``sparse_factor``'s docstring.  ``SparseColoring.permute``
is differentiable: the permuted values are one ``index_select`` of ``A``'s.
"""

from __future__ import annotations

import torch

from . import _backend as _be
from . import _pattern as _pt
from .sparse_factor import _check, _Factor, _factorise, _operand

__all__ = ["sparse_coloring", "SparseColoring", "sparse_sgs", "SparseSGS", "SparseColoredILU0", "SparseColoredIC0"]


def _pattern_of(A: torch.Tensor, what: str):
    """(row-gather plan, value array as the caller handed it) of a 2-D square sparse operand of any value dtype."""
    if not isinstance(A, torch.Tensor):
        raise ValueError(f"{what}: A should be an instance of torch.Tensor")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError(f"{what}: A should be in either COO or CSR sparse format")
    if A.dim() != 2:
        raise ValueError(f"{what}: A must be a 2-D sparse matrix (batched operands are not supported), got {A.dim()} dimensions")
    if A.size(0) != A.size(1):
        raise ValueError(f"{what}: A must be square, got {tuple(A.shape)}")
    if A.layout == torch.sparse_csr:
        return _pt.from_csr(A.detach()), A.values().reshape(-1)
    A = A if A.is_coalesced() else A.coalesce()
    return _pt.from_coo_2d(A.detach().indices(), A.shape, coalesced=True), A.values()


class SparseColoring:
    r"""A multicolour ordering of a square sparse pattern.

    ``colors``     ``(n,)`` int32: the colour of every row;  ``n_colors`` their number
    ``perm``       ``(n,)`` int64, new → old: the rows ordered by (colour, old index);  ``inverse`` old → new
    ``offsets``    ``n_colors + 1`` host integers: class ``c`` is the new rows ``offsets[c] … offsets[c + 1] − 1``
    ``permute(A)`` ``P·A·Pᵀ`` as CSR with ascending columns, for an ``A`` on the pattern the colouring was made for; its values are an
                   ``index_select`` of ``A``'s, so gradients flow
    ``permute_rows(X)`` / ``unpermute_rows(X)``  ``P·X`` and ``Pᵀ·X`` for a dense ``X`` with ``n`` rows"""

    def __init__(self, plan: _pt.ColoringPlan, shape):
        self._plan, self.shape = plan, tuple(shape)

    colors = property(lambda self: self._plan.colors)
    n_colors = property(lambda self: self._plan.n_colors)
    perm = property(lambda self: self._plan.perm)
    inverse = property(lambda self: self._plan.inverse)
    offsets = property(lambda self: self._plan.offsets)

    def _values_of(self, A: torch.Tensor, what: str) -> torch.Tensor:
        g, values = _pattern_of(A, what)
        if tuple(A.shape) != self.shape or values.numel() != self._plan.pos.numel():
            raise ValueError(f"{what}: A does not have the pattern this colouring was made for")
        return values

    def permute(self, A: torch.Tensor) -> torch.Tensor:
        values = self._values_of(A, "SparseColoring.permute")
        g = self._plan.gather
        return torch.sparse_csr_tensor(g.crow, g.col, values.index_select(0, self._plan.pos), self.shape)

    def permute_rows(self, X: torch.Tensor) -> torch.Tensor:
        return X.index_select(0, self._plan.perm)

    def unpermute_rows(self, X: torch.Tensor) -> torch.Tensor:
        return X.index_select(0, self._plan.inverse)


def sparse_coloring(A: torch.Tensor, *, colors=None) -> SparseColoring:
    r"""The multicolour ordering of a square sparse ``A`` (COO or CSR, any value dtype, int32 or int64 indices).

    ``colors=None`` computes the greedy colouring defined in the module's docstring: a pure function of the pattern, the same on
    every run and for every launch geometry; a 7-point stencil takes 2–6 colours, a 27-point stencil 8–15.  ``colors=`` takes the
    caller's colouring instead — ``(x + y + z) % 2`` on a 7-point lattice, say — as ``n`` non-negative integers; a colouring in which
    two coupled rows share a colour raises ``ValueError`` naming the lowest such row.  The plan is cached with the pattern."""
    g, _ = _pattern_of(A, "sparse_coloring")
    with torch.no_grad():
        if colors is not None and not isinstance(colors, torch.Tensor):
            colors = torch.as_tensor(colors, device=g.col.device)
        return SparseColoring(_pt.coloring_plan(g, colors), A.shape)


def _resolve(ordering, g: _pt.RowGather, A: torch.Tensor, what: str) -> _pt.ColoringPlan:
    if isinstance(ordering, SparseColoring):
        if ordering.shape != tuple(A.shape) or ordering._plan.pos.numel() != g.nnz:
            raise ValueError(f"{what}: the SparseColoring was made for another pattern")
        return ordering._plan
    if isinstance(ordering, str) and ordering == "multicolor":
        return _pt.coloring_plan(g)
    raise ValueError(f"{what}: ordering must be None, \"multicolor\" or a SparseColoring, got {ordering!r}")


# ---- the application: 2 · n_colors launches --------------------------------------------------------------------------------------------

def _sweep_group(p: int, device) -> int:
    """Lanes per row of the sweep: the narrowest accepted group whose column tiles cover p (speed only; the torch-op form has none)."""
    if device.type != "cuda":
        return 0
    _, _, widths, tile = _be.color_geometry()
    return next((w for w in widths if (w // widths[0]) * tile >= p), widths[-1])


def _apply(plan: _pt.ColoringPlan, R: torch.Tensor, first, second) -> torch.Tensor:
    """out = Pᵀ·T₂⁻¹·T₁⁻¹·P·R for two triangular sweeps `first` (lower, ascending colours) and `second` (upper, descending colours),
    each a tuple (SweepTable, values, value map or None, mode).  The row gather of R is folded into the loads of the first sweep
    and the scatter of the result into the stores of the second: exactly 2 · n_colors launches, no host synchronisation."""
    if R.is_cuda:
        sweeps = _be.csr_color_sweeps
    else:
        from . import _cpu

        sweeps = _cpu.csr_color_sweeps
    R = _be.rowmajor(R)
    n, p = R.shape
    X = torch.empty((n, p), dtype=R.dtype, device=R.device)
    out = torch.empty_like(X)
    if n == 0 or p == 0:
        return out
    group = _sweep_group(p, R.device)
    rows, classes = plan.perm_index, plan.classes
    t, val, vmap, mode = first
    sweeps(mode, t.begin, t.end, t.idx, t.diag, val, R, X, classes, vmap=vmap, bmap=rows, group=group)
    t, val, vmap, mode = second
    sweeps(mode, t.begin, t.end, t.idx, t.diag, val, X, X, classes[::-1], vmap=vmap, out=out, out_rows=rows, group=group)
    return out


class _Colored(_Factor):
    """Common to the three coloured objects."""

    @property
    def coloring(self) -> SparseColoring:
        return SparseColoring(self._plan, self.shape)

    def _permuted(self, gather: _pt.RowGather, values: torch.Tensor) -> torch.Tensor:
        return torch.sparse_csr_tensor(gather.crow, gather.col, values, self.shape)


class SparseColoredILU0(_Colored):
    r"""``M = Pᵀ·L·U·P``: the ILU(0) of ``P·A·Pᵀ`` in a multicolour ordering ``P`` (``sparse_ilu0(A, ordering=…)``).

    ``coloring``  the ordering;  ``values``  the combined ``L \ U`` array on the pattern of ``P·A·Pᵀ`` (ascending columns)
    ``M(R)`` / ``M.solve(R, transpose=False)``  ``M⁻¹R`` (``M⁻ᵀR``) for ``R`` of shape ``(n,)`` or ``(n, p)`` in the ORIGINAL numbering:
        one launch per colour and sweep, no host synchronisation — an application can be captured in a graph
    ``M.T``       the transposed preconditioner;  ``L`` / ``U``  CSR factors in the permuted numbering (``L`` with a unit diagonal)
    ``info``      0, or 1 + the lowest row (permuted numbering) with a zero pivot"""

    def __init__(self, plan: _pt.ColoringPlan, values: torch.Tensor, info: torch.Tensor, shape, transposed: bool = False, t_values=None):
        self._plan, self.values, self.info, self.shape, self._transposed = plan, values, info, tuple(shape), transposed
        self._t_values = t_values

    def _transposed_values(self) -> torch.Tensor:
        if self._t_values is None:             # gathered once per factorisation, not per application
            self._t_values = self.values.index_select(0, self._plan.transposed()[0].perm.to(torch.int64))
        return self._t_values

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        plan = self._plan
        if transpose != self._transposed:       # (L·U)ᵀ = Uᵀ·Lᵀ: a lower sweep with Uᵀ, a unit upper sweep with Lᵀ
            lower, upper = plan.transposed()[1]
            v = self._transposed_values()
            return self._apply(R, (lambda X: _apply(plan, X, (lower, v, None, _be.SWEEP_DIVIDE), (upper, v, None, _be.SWEEP_UNIT)),))
        lower, upper = plan.tables()
        v = self.values
        return self._apply(R, (lambda X: _apply(plan, X, (lower, v, None, _be.SWEEP_UNIT), (upper, v, None, _be.SWEEP_DIVIDE)),))

    @property
    def T(self) -> "SparseColoredILU0":
        return SparseColoredILU0(self._plan, self.values, self.info, self.shape, not self._transposed, self._transposed_values())

    @property
    def L(self) -> torch.Tensor:
        lg, pos, dp = self._plan.factor.lower()
        val = self.values.index_select(0, pos)
        val[dp.to(torch.int64)] = 1
        return self._permuted(lg, val)

    @property
    def U(self) -> torch.Tensor:
        ug, pos = self._plan.factor.upper()
        return self._permuted(ug, self.values.index_select(0, pos))


class SparseColoredIC0(_Colored):
    r"""``M = Pᵀ·L·Lᵀ·P``: the IC(0) of ``P·A·Pᵀ`` in a multicolour ordering ``P`` (``sparse_ic0(A, ordering=…)``).

    ``coloring``  the ordering;  ``values``  the values of ``L`` on the pattern of ``tril(P·A·Pᵀ)``
    ``M(R)`` / ``M.solve(R, transpose=False)``  ``M⁻¹R`` in the original numbering (``M`` is symmetric: ``M.T`` is ``M``): one launch
        per colour and sweep, no host synchronisation
    ``L`` / ``U``  the CSR factor and its transpose, in the permuted numbering
    ``info``      0, or 1 + the lowest row (permuted numbering) whose radicand was not positive"""

    def __init__(self, plan: _pt.ColoringPlan, values: torch.Tensor, info: torch.Tensor, shape):
        self._plan, self.values, self.info, self.shape = plan, values, info, tuple(shape)
        self._t_values = values.index_select(0, plan.lower_tables()[4])           # Lᵀ's values, gathered once

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        plan = self._plan
        _, _, lower, upper, _ = plan.lower_tables()
        v, vt = self.values, self._t_values
        return self._apply(R, (lambda X: _apply(plan, X, (lower, v, None, _be.SWEEP_DIVIDE), (upper, vt, None, _be.SWEEP_DIVIDE)),))

    @property
    def T(self) -> "SparseColoredIC0":
        return self

    @property
    def L(self) -> torch.Tensor:
        return self._permuted(self._plan.lower_tables()[0], self.values)

    @property
    def U(self) -> torch.Tensor:
        return self._permuted(self._plan.lower_tables()[0].transposed, self._t_values)


class SparseSGS(_Colored):
    r"""The symmetric Gauss–Seidel preconditioner ``M = (D + L)·D⁻¹·(D + U)`` of ``P·A·Pᵀ = L + D + U`` in a multicolour ordering ``P``,
    on ``A``'s own values: no factorisation (``sparse_sgs``).

    ``coloring``  the ordering;  ``values``  ``A``'s values as they were handed over (read through the plan's gather map)
    ``M(R)`` / ``M.solve(R, transpose=False)``  ``M⁻¹R`` in the original numbering: one launch per colour and sweep, no host
        synchronisation.  ``M.T`` is the transposed form, ``(D + Uᵀ)·D⁻¹·(D + Lᵀ)``; for a symmetric ``A`` it is ``M``
    ``refresh(A_new)``  new values on the same pattern
    ``info``      0: nothing can break down but a zero on the diagonal, which shows as inf / nan in the result"""

    def __init__(self, plan: _pt.ColoringPlan, values: torch.Tensor, shape, transposed: bool = False):
        self._plan, self.values, self.shape, self._transposed = plan, values, tuple(shape), transposed
        self.info = torch.zeros((), dtype=torch.int64, device=values.device)

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        plan = self._plan
        if transpose != self._transposed:
            tg, (lower, upper) = plan.transposed()
            vmap = plan._part("sgs_t_map", lambda: plan.pos.index_select(0, tg.perm.to(torch.int64)).to(tg.col.dtype).contiguous())
        else:
            (lower, upper), vmap = plan.tables(), plan.pos_index
        v = self.values
        return self._apply(R, (lambda X: _apply(plan, X, (lower, v, vmap, _be.SWEEP_DIVIDE), (upper, v, vmap, _be.SWEEP_SCALED)),))

    @property
    def T(self) -> "SparseSGS":
        return SparseSGS(self._plan, self.values, self.shape, not self._transposed)

    def refresh(self, A_new: torch.Tensor) -> "SparseSGS":
        with torch.no_grad():
            g, values = _operand(A_new, "SparseSGS.refresh")
            if tuple(A_new.shape) != self.shape or values.numel() != self.values.numel() or values.dtype != self.values.dtype:
                raise ValueError("SparseSGS.refresh: A_new must have the pattern and the dtype of the matrix the preconditioner was built for")
            self.values = values.contiguous()
        return self


def sparse_sgs(A: torch.Tensor, *, ordering="multicolor") -> SparseSGS:
    r"""The symmetric Gauss–Seidel preconditioner of a square sparse ``A`` (COO or CSR, float32 / float64) in a multicolour ordering.

    ``M = (D + L)·D⁻¹·(D + U)`` with the strict triangles and the diagonal of ``P·A·Pᵀ``; for a symmetric positive definite ``A`` it is
    symmetric positive definite.  The pattern must store every diagonal entry and no column twice per row.  ``ordering``:
    ``"multicolor"`` (the greedy colouring) or a :class:`SparseColoring`.  No gradient flows through the preconditioner."""
    with torch.no_grad():
        g, values = _operand(A, "sparse_sgs")
        plan = _resolve(ordering, g, A, "sparse_sgs")
        plan.factor          # (the check of the pattern: ValueError naming the first offending row)
    return SparseSGS(plan, values.contiguous(), A.shape)


def colored_ilu0(A: torch.Tensor, ordering, shift: float, check: bool) -> SparseColoredILU0:
    """``sparse_ilu0(A, ordering=…)``: the existing factorisation kernel on the values gathered into the permuted pattern."""
    with torch.no_grad():
        g, values = _operand(A, "sparse_ilu0")
        plan = _resolve(ordering, g, A, "sparse_ilu0")
        fp = plan.factor
        out, info = _factorise("ilu0", fp.gather, fp.diag_pos, values.index_select(0, plan.pos), float(shift))
    if check:
        _check(info, "sparse_ilu0: zero pivot")
    return SparseColoredILU0(plan, out, info, A.shape)


def colored_ic0(A: torch.Tensor, ordering, shift: float, check: bool) -> SparseColoredIC0:
    """``sparse_ic0(A, ordering=…)``: the existing factorisation kernel on the lower triangle of the permuted pattern."""
    with torch.no_grad():
        g, values = _operand(A, "sparse_ic0")
        plan = _resolve(ordering, g, A, "sparse_ic0")
        lg, lpos, dp = plan.factor.lower()
        out, info = _factorise("ic0", lg, dp, values.index_select(0, plan.pos).index_select(0, lpos), float(shift))
    if check:
        _check(info, "sparse_ic0: non-positive pivot")
    return SparseColoredIC0(plan, out, info, A.shape)
