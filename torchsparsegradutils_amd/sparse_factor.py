"""``sparse_ilu0`` / ``sparse_ic0`` — zero-fill incomplete factorisations of a sparse matrix on its own pattern.

What csrilu02 / csric02 (cuSPARSE, rocSPARSE), MATLAB's ``ilu`` / ``ichol`` without fill, PETSc's ILU(0) / ICC(0) and scipy's
``spilu`` restricted to the pattern compute; the reference package has no counterpart.  The numeric factorisation is ONE persistent,
dependency-driven launch on the gfx950 (``csrc/ilu_impl.h``, C ABI in ``include/tsgu_hip_factor.h``); everything about the pattern
(the check, the diagonal positions, the triangles) is a plan cached with it (``_pattern.factor_plan``).

The result is an application object: ``M(R)`` applies ``M⁻¹`` by two triangular solves on the sync-free sweep of
``sparse_triangular_solve`` and is what ``linear_cg(preconditioner=…)``, ``BICGSTABSettings.precon`` and the MINRES settings take.

No gradient flows through a factor: both functions run under ``no_grad`` on the detached operand.  That is the right thing for a
preconditioner — it changes how fast a Krylov loop reaches the solution of ``A x = b``, not the solution, and inside
``sparse_generic_solve`` the gradients come from the adjoint solve with ``Aᵀ`` (preconditioned by ``M.T``), never from
differentiating through the iterations or through ``M``.  (An incomplete factor used as a MODEL parameter — a learnt
``scale_tril`` — is a different object: build that from a leaf tensor of values.)

CPU operands are factorised by a plain row-by-row loop (``_cpu.csr_factor``: the same semantics, reference speed only); the
switch is the operands' device, as everywhere in the package.
"""

from __future__ import annotations

import torch

from . import _backend as _be
from . import _pattern as _pt
from .sparse_solve import _solve

__all__ = ["sparse_ilu0", "sparse_ic0", "SparseILU0", "SparseIC0"]


def _operand(A: torch.Tensor, what: str):
    """(row-gather plan, value array) of the detached 2-D operand, after the refusals."""
    if not isinstance(A, torch.Tensor):
        raise ValueError(f"{what}: A should be an instance of torch.Tensor")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError(f"{what}: A should be in either COO or CSR sparse format")
    if A.dim() != 2:
        raise ValueError(f"{what}: A must be a 2-D sparse matrix (batched operands are not supported), got {A.dim()} dimensions")
    if A.size(0) != A.size(1):
        raise ValueError(f"{what}: A must be square, got {tuple(A.shape)}")
    if A.dtype not in _be.FACTOR_DTYPES:
        raise TypeError(f"{what}: float32 and float64 operands only, got {A.dtype}")
    A = A.detach()
    if A.layout == torch.sparse_csr:
        return _pt.from_csr(A), A.values().reshape(-1)
    A = A if A.is_coalesced() else A.coalesce()
    return _pt.from_coo_2d(A.indices(), A.shape, coalesced=True), A.values()


def _factorise(kind: str, gather: _pt.RowGather, diag_pos, values, shift: float):
    if values.is_cuda:
        return _be.csr_factor(kind, gather.crow, gather.col, diag_pos, values, gather.n_rows, shift=shift)
    from . import _cpu

    return _cpu.csr_factor(kind, gather.crow, gather.col, diag_pos, values, gather.n_rows, shift=shift)


def _check(info: torch.Tensor, message: str) -> None:
    row = int(info.item())
    if row:
        raise RuntimeError(f"{message} in row {row - 1}")


class _Factor:
    """Common to both application objects: shapes of ``R`` and the call protocol."""

    def __call__(self, R: torch.Tensor) -> torch.Tensor:
        return self.solve(R)

    def _apply(self, R: torch.Tensor, sweeps) -> torch.Tensor:
        if not isinstance(R, torch.Tensor) or R.dim() not in (1, 2) or R.size(0) != self.shape[0]:
            raise ValueError(f"a right-hand side of shape ({self.shape[0]},) or ({self.shape[0]}, p) is required, got "
                             f"{tuple(R.shape) if isinstance(R, torch.Tensor) else type(R).__name__}")
        if R.dtype != self.values.dtype:
            raise RuntimeError(f"expected the factor and R to have the same dtype, got {self.values.dtype} and {R.dtype}")
        X = R.detach().reshape(R.size(0), -1)
        with torch.no_grad():
            for sweep in sweeps:
                X = sweep(X)
        return X.reshape(R.shape)

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def device(self):
        return self.values.device


class SparseILU0(_Factor):
    r"""``M = L·U`` with ``L`` unit lower and ``U`` upper triangular on the pattern of ``A``.

    ``values``  the combined array on the canonical pattern (ascending columns): strict lower part ``L``, diagonal and upper ``U``
    ``M(R)`` / ``M.solve(R, transpose=False)``  ``M⁻¹R`` (``M⁻ᵀR``) for ``R`` of shape ``(n,)`` or ``(n, p)``: two sweeps over the
        combined array — each ignores the entries on the other side of the diagonal, nothing is split
    ``M.T``     the transposed preconditioner (for ``transpose_solve`` of ``sparse_generic_solve``)
    ``L`` / ``U``  CSR factors (``L`` with an explicit unit diagonal), split out on first use
    ``info``    0, or 1 + the lowest row with a zero pivot (a device tensor until someone reads it)"""

    def __init__(self, plan: _pt.FactorPlan, values: torch.Tensor, info: torch.Tensor, shape, transposed: bool = False):
        self._plan, self.values, self.info, self.shape, self._transposed = plan, values, info, tuple(shape), transposed

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        g, v = self._plan.gather, self.values
        if transpose != self._transposed:       # (L·U)⁻ᵀ = L⁻ᵀ·U⁻ᵀ
            return self._apply(R, (lambda X: _solve(g, v, X, True, False, True, combined=True),
                                   lambda X: _solve(g, v, X, False, True, True, combined=True)))
        return self._apply(R, (lambda X: _solve(g, v, X, False, True, False, combined=True),
                               lambda X: _solve(g, v, X, True, False, False, combined=True)))

    @property
    def T(self) -> "SparseILU0":
        return SparseILU0(self._plan, self.values, self.info, self.shape, not self._transposed)

    @property
    def crow_indices(self):
        return self._plan.gather.crow

    @property
    def col_indices(self):
        return self._plan.gather.col

    @property
    def L(self) -> torch.Tensor:
        # the lower triangle of the pattern with the diagonal's values replaced by ones
        lg, pos, dp = self._plan.lower()
        val = self.values.index_select(0, pos)
        val[dp.to(torch.int64)] = 1
        return torch.sparse_csr_tensor(lg.crow, lg.col, val, self.shape)

    @property
    def U(self) -> torch.Tensor:
        ug, pos = self._plan.upper()
        return torch.sparse_csr_tensor(ug.crow, ug.col, self.values.index_select(0, pos), self.shape)


class SparseIC0(_Factor):
    r"""``M = L·Lᵀ`` with ``L`` lower triangular on the pattern of ``tril(A)``.

    ``values``  the values of ``L`` on the lower CSR pattern (ascending columns, the diagonal closes every row)
    ``M(R)`` / ``M.solve(R, transpose=False)``  ``M⁻¹R``: a sweep with ``L``, one with ``Lᵀ`` (``M`` is symmetric: ``transpose``
        changes nothing, and ``M.T`` is ``M``)
    ``L``       the CSR lower factor — a ``scale_tril`` / ``precision_tril`` for ``SparseMultivariateNormal``
    ``info``    0, or 1 + the lowest row whose radicand was not positive"""

    def __init__(self, gather: _pt.RowGather, values: torch.Tensor, info: torch.Tensor, shape):
        self._gather, self.values, self.info, self.shape = gather, values, info, tuple(shape)

    def solve(self, R: torch.Tensor, transpose: bool = False) -> torch.Tensor:
        g, v = self._gather, self.values
        return self._apply(R, (lambda X: _solve(g, v, X, False, False, False), lambda X: _solve(g, v, X, False, False, True)))

    @property
    def T(self) -> "SparseIC0":
        return self

    @property
    def crow_indices(self):
        return self._gather.crow

    @property
    def col_indices(self):
        return self._gather.col

    @property
    def L(self) -> torch.Tensor:
        return torch.sparse_csr_tensor(self._gather.crow, self._gather.col, self.values, self.shape)


def sparse_ilu0(A: torch.Tensor, *, shift: float = 0.0, check: bool = True, ordering=None) -> SparseILU0:
    r"""ILU(0) of a square sparse ``A`` (COO or CSR, float32 / float64): ``A ≈ L·U`` with no entry outside the pattern of ``A``.

    The IKJ form; every update is one IEEE division, multiplication and subtraction in the value type, applied in ascending order
    of the eliminated column, so the result is bit-identical to the sequential loop whatever the launch geometry.  The pattern must
    store every diagonal entry and no column twice per row (``ValueError`` naming the first offending row); unsorted columns are
    sorted through a cached permutation.  ``shift``: the diagonal used is ``a_ii·(1 + shift)``.  ``check=True`` reads the
    breakdown word (one synchronisation) and raises ``RuntimeError("zero pivot in row r")``; ``check=False`` leaves ``.info`` on
    the device.  No gradient flows through the factor (see the module's docstring).

    ``ordering=None`` is the natural ordering.  ``ordering="multicolor"`` (or a ``SparseColoring``) factorises ``P·A·Pᵀ`` in a
    multicolour ordering instead and returns a ``SparseColoredILU0``, whose application is one wait-free launch per colour and sweep
    (``sparse_coloring.py``): a far cheaper application of a weaker preconditioner."""
    if ordering is not None:
        from .sparse_coloring import colored_ilu0

        return colored_ilu0(A, ordering, shift, check)
    with torch.no_grad():
        g, values = _operand(A, "sparse_ilu0")
        plan = _pt.factor_plan(g)
        out, info = _factorise("ilu0", plan.gather, plan.diag_pos, plan.canonical_values(values), float(shift))
    if check:
        _check(info, "sparse_ilu0: zero pivot")
    return SparseILU0(plan, out, info, A.shape)


def sparse_ic0(A: torch.Tensor, *, shift: float = 0.0, check: bool = True, ordering=None) -> SparseIC0:
    r"""IC(0) of a square sparse ``A`` (COO or CSR, float32 / float64): ``A ≈ L·Lᵀ`` with ``L`` on the pattern of ``tril(A)``.

    Only the lower triangle of ``A`` is read; symmetry is not checked.  The pattern conditions and ``shift`` (the usual remedy for
    a breakdown) are those of :func:`sparse_ilu0`.  Two calls give the same bits.  ``check=True`` raises
    ``RuntimeError("non-positive pivot in row r")``.  No gradient flows through the factor.  ``ordering``: as for
    :func:`sparse_ilu0`; the coloured form is a ``SparseColoredIC0``."""
    if ordering is not None:
        from .sparse_coloring import colored_ic0

        return colored_ic0(A, ordering, shift, check)
    with torch.no_grad():
        g, values = _operand(A, "sparse_ic0")
        plan = _pt.factor_plan(g)
        lg, pos, dp = plan.lower()
        out, info = _factorise("ic0", lg, dp, plan.canonical_values(values).index_select(0, pos), float(shift))
    if check:
        _check(info, "sparse_ic0: non-positive pivot")
    return SparseIC0(lg, out, info, A.shape)
