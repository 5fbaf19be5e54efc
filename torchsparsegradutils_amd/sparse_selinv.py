"""``sparse_selected_inverse`` — the entries of ``Σ = (L·Lᵀ)⁻¹`` or ``((L+I)·D·(L+I)ᵀ)⁻¹`` on the pattern of the lower factor ``L``.

The Takahashi recurrence (Takahashi, Fagan & Chin 1973; Erisman & Tinney 1975): what INLA-style inference builds the posterior
marginal variances of a Gaussian Markov random field on, and the exact gradient of ``log det Q`` on ``Q``'s pattern.  It costs what
the factorisation cost and never forms an ``n × n`` matrix; the reference package has no counterpart.  The recurrence is ONE persistent,
dependency-driven launch on the gfx950 (``csrc/selinv_impl.h``, C ABI in ``include/tsgu_hip_selinv.h``); everything about the pattern
(the check, the column view of ``L``) is a plan cached with it (``_pattern.selinv_plan``).

The pattern of ``L`` must be closed under elimination: for every column, every pair of rows stored below the diagonal is itself a
stored position.  Every true Cholesky factor, every full band, every arrow or block-tridiagonal form and every ``sparse_ic0`` result
on such a pattern is; ``cholesky_pattern(A)`` returns the closed pattern of a symmetric ``A``, so that
``sparse_ic0(cholesky_pattern(A)).L`` is an exact factor the recurrence accepts.

Not differentiable (the adjoint recurrence is not written): operands that require grad are refused unless gradients are disabled.
CPU operands are served by a plain column-by-column loop (``_cpu.selected_inverse``: the same semantics, reference speed only).
"""

from __future__ import annotations

import torch

from . import _backend as _be
from . import _pattern as _pt

__all__ = ["sparse_selected_inverse", "SparseSelectedInverse", "cholesky_pattern"]

_NO_GRAD = ("sparse_selected_inverse is not differentiable: the adjoint recurrence is not implemented; detach the operands or call it "
            "under torch.no_grad()")


def _operand(L: torch.Tensor):
    """(row-gather plan, value array, rebuild) of the detached 2-D operand, after the refusals."""
    what = "sparse_selected_inverse"
    if not isinstance(L, torch.Tensor):
        raise ValueError(f"{what}: L should be an instance of torch.Tensor")
    if L.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError(f"{what}: L should be in either COO or CSR sparse format")
    if L.dim() != 2:
        raise ValueError(f"{what}: L must be a 2-D sparse matrix (batched operands are not supported), got {L.dim()} dimensions")
    if L.size(0) != L.size(1):
        raise ValueError(f"{what}: L must be square, got {tuple(L.shape)}")
    if L.dtype not in _be.FACTOR_DTYPES:
        raise TypeError(f"{what}: float32 and float64 operands only, got {L.dtype}")
    L = L.detach()
    if L.layout == torch.sparse_csr:
        crow, col = L.crow_indices(), L.col_indices()
        return _pt.from_csr(L), L.values().reshape(-1), lambda v: torch.sparse_csr_tensor(crow, col, v, L.shape)
    L = L if L.is_coalesced() else L.coalesce()
    idx = L.indices()
    return (_pt.from_coo_2d(idx, L.shape, coalesced=True), L.values(),
            lambda v: torch.sparse_coo_tensor(idx, v, L.shape, is_coalesced=True))


class SparseSelectedInverse(torch.autograd.Function):
    """``(L, D) ↦ (values of Σ on L's stored positions, diag Σ or None, info)`` — forward only: the results are marked
    non-differentiable and :func:`sparse_selected_inverse` refuses operands that require grad before it gets here."""

    @staticmethod
    def forward(ctx, L, D, wg_per_cu):
        g, values, _ = _operand(L)
        plan = _pt.selinv_plan(g, strict=D is not None)
        D = None if D is None else D.detach()
        if values.is_cuda:
            out, diag, info = _be.csc_selinv(plan.colptr, plan.rowidx, plan.perm, plan.diag_pos, values, g.n_rows, D=D,
                                             wg_per_cu=wg_per_cu)
        else:
            from . import _cpu

            out, diag, info = _cpu.selected_inverse(plan.colptr, plan.rowidx, plan.perm, plan.diag_pos, values, g.n_rows, D=D)
        ctx.mark_non_differentiable(*(t for t in (out, diag, info) if t is not None))
        return out, diag, info

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError(_NO_GRAD)


def sparse_selected_inverse(L: torch.Tensor, diagonal: torch.Tensor = None, *, check: bool = True, workgroups_per_cu: int = 1):
    r"""The selected inverse of ``Q = L·Lᵀ`` (``diagonal=None``; ``L`` lower triangular with every diagonal stored) or of
    ``Q = (L+I)·D·(L+I)ᵀ`` (``diagonal=D`` of shape ``(n,)``; ``L`` stored strictly lower — the LDLᵀ form of
    ``SparseMultivariateNormal``): a sparse tensor ``Z`` on ``L``'s own layout and index tensors with ``Z[r, c] = Q⁻¹[r, c]`` at the
    stored positions.  The LDLᵀ form returns ``(Z, diag Q⁻¹)``.

    ``L``: 2-D COO or CSR, float32 / float64, int32 / int64 indices.  Its pattern must be closed under elimination (module
    docstring).  A lookup that misses a stored position contributes a zero; with ``check=True`` the call reads the report (one
    synchronisation) and raises ``ValueError`` naming the lowest offending column; with ``check=False`` nothing synchronises.  A zero
    or non-finite pivot (``L_ii`` or ``D_i``) never raises: the column is finished with IEEE arithmetic and the call returns.  The
    report stays on the device in ``Z.selinv_info`` (two int64: 1 + the lowest column with such a pivot, 1 + the lowest column that
    is not closed; 0 for none).  The order of every sum depends on the pattern
    only: two calls, whatever ``workgroups_per_cu`` (1 … 8), give the same bits.

    Not differentiable: with gradients enabled, an ``L`` or ``diagonal`` that requires grad raises ``NotImplementedError``."""
    if torch.is_grad_enabled() and ((isinstance(L, torch.Tensor) and L.requires_grad)
                                    or (isinstance(diagonal, torch.Tensor) and diagonal.requires_grad)):
        raise NotImplementedError(_NO_GRAD)
    _, values, rebuild = _operand(L)
    n = L.size(0)
    if diagonal is not None:
        if not isinstance(diagonal, torch.Tensor) or diagonal.shape != (n,):
            raise ValueError(f"sparse_selected_inverse: diagonal must have shape ({n},), got "
                             f"{tuple(diagonal.shape) if isinstance(diagonal, torch.Tensor) else type(diagonal).__name__}")
        if diagonal.dtype != L.dtype:
            raise TypeError(f"sparse_selected_inverse: L and diagonal must have the same dtype, got {L.dtype} and {diagonal.dtype}")
        _be.operand_device(values, diagonal)
    with torch.no_grad():
        out, diag, info = SparseSelectedInverse.apply(L, diagonal, int(workgroups_per_cu))
    if check:
        opened = int(info[1].item())
        if opened:
            raise ValueError(f"sparse_selected_inverse: column {opened - 1} needs an entry of the inverse that is not a stored position: "
                             "the pattern of L must be closed under elimination (cholesky_pattern returns such a pattern)")
    Z = rebuild(out)
    Z.selinv_info = info
    return Z if diagonal is None else (Z, diag)


def cholesky_pattern(A: torch.Tensor) -> torch.Tensor:
    """The filled lower pattern of a symmetric sparse ``A`` (2-D COO or CSR; only its lower triangle is read): a symbolic Cholesky
    factorisation by the elimination tree (Liu's row-subtree walk), as a CSR tensor on ``A``'s device with ``A``'s lower values
    scattered in and explicit zeros at the fill.  Plain host code on the index tensors, linear in the size of the result; run once
    per pattern.  The result is closed under elimination, and ``sparse_ic0`` of it is the exact Cholesky factor."""
    import numpy as np

    if not isinstance(A, torch.Tensor) or A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError("cholesky_pattern: A should be in either COO or CSR sparse format")
    if A.dim() != 2 or A.size(0) != A.size(1):
        raise ValueError(f"cholesky_pattern: A must be a square 2-D sparse matrix, got {tuple(A.shape)}")
    A = A.detach()
    n = A.size(0)
    if A.layout == torch.sparse_csr:
        idt = A.col_indices().dtype
        Ac = A.to_sparse_coo().coalesce()
    else:
        Ac = A.coalesce()
        idt = torch.int64
    rows, cols = (t.cpu().numpy().astype(np.int64) for t in Ac.indices())
    vals = Ac.values()
    low = cols <= rows
    lrows, lcols = rows[low], cols[low]                    # coalesced: sorted by row, then column
    starts = np.searchsorted(lrows, np.arange(n + 1))
    parent = np.full(n, -1, dtype=np.int64)
    mark = np.full(n, -1, dtype=np.int64)
    pattern = []
    for i in range(n):
        mark[i] = i
        found = [i]
        for j in lcols[starts[i]:starts[i + 1]]:
            while mark[j] != i:                            # climb from j towards i: every vertex on the way is a column of row i
                if parent[j] < 0:
                    parent[j] = i
                mark[j] = i
                found.append(j)
                j = parent[j]
        found.sort()
        pattern.append(found)
    counts = np.array([len(p) for p in pattern], dtype=np.int64)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=crow[1:])
    col = np.fromiter((j for p in pattern for j in p), dtype=np.int64, count=int(crow[-1]))
    frow = np.repeat(np.arange(n, dtype=np.int64), counts)
    # A's lower entries are a subset of the filled pattern: both keys ascend, one searchsorted places them
    where = np.searchsorted(frow * n + col, lrows * n + lcols)
    values = torch.zeros(int(crow[-1]), dtype=vals.dtype, device=vals.device)
    values[torch.from_numpy(where).to(vals.device)] = vals[torch.from_numpy(np.nonzero(low)[0]).to(vals.device)]
    return torch.sparse_csr_tensor(torch.from_numpy(crow).to(idt).to(vals.device), torch.from_numpy(col).to(idt).to(vals.device), values,
                                   A.shape)
