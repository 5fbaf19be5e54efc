"""``sparse_lobpcg`` — a few extreme eigenpairs of a symmetric sparse matrix, with a gradient that stays on the matrix's pattern.

``torch.lobpcg`` accepts a sparse ``A`` but its backward refuses one (``lobpcg.backward does not support sparse input yet``).
Here the eigenvalues are differentiable with respect to ``A``, and the gradient is what the package exists for:

    ∂(Σ_j g_j·λ_j) / ∂A_ab = Σ_j g_j·v_aj·v_bj      at the stored positions of A only,

one SDDMM with ``G = V·diag(g)`` and ``B = V`` on the pattern's cached plan (``_ops.sddmm``: every kernel family), returned as a
sparse tensor of ``A``'s layout with ``A``'s index tensors, exactly as ``sparse_mm`` returns its ``gradA``.

The iteration is ``utils.lobpcg`` (Knyazev's LOBPCG, the robust variant of scipy): per step one sparse product ``A·W`` through
``sparse_mm``'s machinery and a handful of passes over the tall-skinny basis ``[X, W, P]`` in the three kernels of
``csrc/lobpcg_impl.h``.  CPU operands run the same recurrence on torch ops (``_cpu``): the operands' device selects the path.

Not differentiable: the EIGENVECTORS (``ctx.mark_non_differentiable``).  Their gradient needs ``k`` shifted singular solves
``(A − λ_j·I)⁺``: a later addition.  The eigenvalue gradient is exact at an exact eigenpair and FIRST-ORDER ACCURATE IN THE
RESIDUAL otherwise: an entry is off by at most ``Σ_j |g_j|·2·‖r_j‖₂ / gap_j``.  For a REPEATED eigenvalue the eigenvectors are
determined only up to a rotation of the eigenspace, so the gradient is meaningful only when the whole cluster is selected with
equal weights ``g_j`` (then it is the gradient of the cluster's sum, which is smooth).

Refused, in the style of the other operators: batched operands (3-D ``A``), BSR / BSC layouts, bfloat16 (and anything that is not
float32 / float64), and a generalised problem (there is no ``B`` argument).
"""

from __future__ import annotations

import torch

from . import _backend as _be
from . import _ops
from .sparse_matmul import _Operand
from .utils.lobpcg import lobpcg as _lobpcg

__all__ = ["sparse_lobpcg", "SparseLOBPCG"]


def sparse_lobpcg(A: torch.Tensor, k: int = 1, *, X: torch.Tensor = None, preconditioner=None, niter: int = 500, tol: float = None,
                  largest: bool = True):
    r"""``(eigenvalues (k,), eigenvectors (n, k))`` of the symmetric sparse ``A``: the ``k`` largest in descending order
    (``largest=True``, torch's default) or the ``k`` smallest in ascending order.

    ``A``   2-D square COO or CSR, float32 or float64, int32 or int64 indices; assumed symmetric (not checked).  Batched, BSR and
            bfloat16 operands are refused; there is no generalised problem ``B``.
    ``k``   ``3k <= n`` (``torch.lobpcg``'s own condition) and ``k <= 32`` (``ValueError`` naming the number).
    ``X``   optional ``(n, k)`` initial block of ``A``'s dtype and device; default ``torch.randn``.
    ``preconditioner``  ``None``, any callable on an ``(n, k)`` block (``sparse_fsai(A)``, ``sparse_ic0(A)``, ``sparse_ilu0(A)``, a
            lambda) or a dense tensor (applied with ``@``), called under ``no_grad``.  It should approximate ``A⁻¹`` and be
            symmetric positive definite: meant for ``largest=False`` on a positive definite ``A``.
    ``tol`` default ``sqrt(eps)``; column ``j`` has converged when ``‖A·x_j − λ_j·x_j‖₂ <= tol·‖A‖_est``,
            ``‖A‖_est = ‖A·X₀‖_F / ‖X₀‖_F`` of the orthonormalised initial block.  The loop stops when all have, or at ``niter``;
            ``utils.last_solve_info("lobpcg")`` tells which, with iterations, residual norms and restarts.

    ``eigenvalues`` is differentiable with respect to ``A`` (sparse gradient on ``A``'s pattern, first-order accurate in the
    residual); ``eigenvectors`` is not differentiable — see the module's docstring for both.  The loop computes the smallest pairs
    of ``σ·A``, ``σ = ∓1``, with the sign applied to the product: no second operand is built, the pattern's plans serve both."""
    if not isinstance(A, torch.Tensor):
        raise ValueError("sparse_lobpcg: A should be an instance of torch.Tensor")
    if A.layout in (torch.sparse_bsr, torch.sparse_bsc):
        raise ValueError("sparse_lobpcg: block-sparse (BSR / BSC) operands are not supported; A should be in either COO or CSR format")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError("sparse_lobpcg: A should be in either COO or CSR sparse format")
    if A.dim() != 2:
        raise ValueError(f"sparse_lobpcg: A must be a 2-D sparse matrix (batched operands are not supported), got {A.dim()} dimensions")
    if A.size(0) != A.size(1):
        raise ValueError(f"sparse_lobpcg: A must be square, got {tuple(A.shape)}")
    if A.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"sparse_lobpcg: float32 and float64 operands only, got {A.dtype}")
    n, k = A.size(0), int(k)
    if k < 1:
        raise ValueError(f"sparse_lobpcg: k must be at least 1, got {k}")
    kmax = _be.tall_geometry(A.dtype)[0]         # the widest block of the tall-skinny kernels
    if k > kmax:
        raise ValueError(f"sparse_lobpcg: at most {kmax} eigenpairs per call, got k = {k}")
    if 3 * k > n:
        raise ValueError(f"sparse_lobpcg: 3k <= n is required, got k = {k} and n = {n} (3k = {3 * k})")
    if X is None:
        X = torch.randn((n, k), dtype=A.dtype, device=A.device)
    elif not isinstance(X, torch.Tensor) or X.layout != torch.strided or tuple(X.shape) != (n, k):
        raise ValueError(f"sparse_lobpcg: X must be a dense ({n}, {k}) block, got "
                         f"{tuple(X.shape) if isinstance(X, torch.Tensor) else type(X).__name__}")
    if X.dtype != A.dtype:
        raise TypeError(f"sparse_lobpcg: X must have A's dtype, got {X.dtype} and {A.dtype}")
    if X.device != A.device:
        raise ValueError(f"sparse_lobpcg: X must be on the device of A, got {X.device} and {A.device}")
    if preconditioner is not None and not callable(preconditioner) and not (
            isinstance(preconditioner, torch.Tensor) and preconditioner.layout == torch.strided):
        raise ValueError("sparse_lobpcg: preconditioner must be None, a callable on an (n, k) block or a dense tensor")
    return SparseLOBPCG.apply(A, X, preconditioner, int(niter), tol, bool(largest))


class SparseLOBPCG(torch.autograd.Function):
    """Autograd function behind :func:`sparse_lobpcg`: ``apply(A, X, preconditioner, niter, tol, largest)``."""

    @staticmethod
    def forward(ctx, A, X, preconditioner, niter, tol, largest):
        op = _Operand(A.detach())
        plan, values = op.plan, op.values
        sign = -1.0 if largest else 1.0
        lam, V = _lobpcg(lambda B: _ops.spmm(plan, values, B), X.detach(), sign=sign, preconditioner=preconditioner, niter=niter, tol=tol)
        lam = lam * sign if largest else lam
        ctx.op = op
        ctx.save_for_backward(V)
        ctx.mark_non_differentiable(V)
        return lam, V

    @staticmethod
    def backward(ctx, grad_lam, _grad_vec):  # type: ignore[override]
        (V,) = ctx.saved_tensors
        op: _Operand = ctx.op
        gradA = None
        if ctx.needs_input_grad[0]:
            G = V * grad_lam.to(V.dtype).reshape(1, -1)
            if op.plan.perm is None:
                gvals = _ops.sddmm(op.plan, G, V)
            else:   # un-coalesced COO: one gradient entry per stored duplicate, in A's own order
                gvals = _be.coo_sddmm(op.indices[0], op.indices[1], G, V)
            gradA = op.rebuild(gvals)
        return gradA, None, None, None, None, None
