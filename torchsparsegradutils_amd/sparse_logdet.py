"""``sparse_logdet`` / ``sparse_inv_quad_logdet`` — ``log det A`` of a sparse symmetric positive definite matrix by stochastic
Lanczos quadrature, with a gradient that stays on the matrix's pattern.

    log det A = tr log A ≈ w · Σ_c ‖z_c‖² · e₁ᵀ log(T_c) e₁,        w = n / ‖Z‖_F²

for ``k`` probe columns ``z_c`` (Rademacher by default: ``E[z zᵀ] = I``), where ``T_c`` is the Lanczos tridiagonal matrix of
``(A, z_c / ‖z_c‖)``.  The weight is ``1/k`` for columns of squared norm ``n`` — every Rademacher column, exactly — and ``1`` for
``probes = I``: a plain ``1/k`` on a user's block would make the identity return ``tr log A / n``.  Conjugate gradients on ``A x = z_c`` produce the entries of ``T_c`` from their own coefficients, so ONE CG run
over the columns ``[Z | B]`` gives

* the quadrature (one launch of ``tsgu_tridiag_quadrature`` on the coefficient history the fused CG loop records on the device),
* ``U = A⁻¹Z``, and with it the Hutchinson estimate of ``∂ log det A / ∂A = A⁻¹`` on A's pattern, ``(w/2)·mask(U Zᵀ + Z Uᵀ)``,
* ``X = A⁻¹B``: ``inv_quad_j = b_jᵀ x_j`` with ``∂/∂A = −mask(x_j x_jᵀ)`` and ``∂/∂B = 2 X``

— GPyTorch's ``inv_quad_logdet``, sparse end to end.  The gradient with respect to ``A`` is one SDDMM on the pattern's cached plan
(``_ops.sddmm``) and comes back on ``A``'s own index tensors, as ``sparse_mm`` returns its ``gradA``.  The symmetrised form costs ``k``
more columns in that one launch and gives the entries (i, j) and (j, i) the same noise.

With ``probes = I`` (any block with ``Z Zᵀ`` a multiple of ``I``) the estimate is exact up to the quadrature's own truncation, which
is zero once ``lanczos_steps`` reaches the degree of the minimal polynomial seen from each column.

CPU operands run the same algorithm in torch ops (``_cpu``): a plain CG loop with a per-column history, the same per-column length
rule, ``torch.linalg.eigh`` in float64.  The generated probes are a pure function of ``(seed, row, column)``, the same bits on
either device and independent of torch's generator.

Out of scope: preconditioned quadrature, other matrix functions in the public interface, batched ``A``, double
backward.
"""

from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _ops
from .sparse_matmul import _Operand
from .utils._operator import SparseOperator, record_solve
from .utils.linear_cg import _cg_with_history, _warn_tolerance_missed

__all__ = ["sparse_logdet", "sparse_inv_quad_logdet", "SparseLogDet"]

_CHUNK = 256        # columns per CG run (the fused step kernels' widest block)
_STOP_AFTER = 1e-10  # a column whose normalised residual falls below this is frozen (linear_cg's stop_updating_after)


def _steps_cap() -> int:
    return _be.quadrature_geometry()[0]


def _check(who: str, A, B, num_probes, lanczos_steps, probes, max_cg_iter):
    if not isinstance(A, torch.Tensor):
        raise ValueError(f"{who}: A should be an instance of torch.Tensor")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError(f"{who}: A should be in either COO or CSR sparse format")
    if A.dim() != 2:
        raise ValueError(f"{who}: A must be a 2-D sparse matrix (batched operands are not supported), got {A.dim()} dimensions")
    if A.size(0) != A.size(1):
        raise ValueError(f"{who}: A must be square, got {tuple(A.shape)}")
    if A.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: float32 and float64 operands only, got {A.dtype}")
    n = A.size(0)
    cap = _steps_cap()
    if not 1 <= int(lanczos_steps) <= cap:
        raise ValueError(f"{who}: lanczos_steps must lie in [1, {cap}], got {lanczos_steps}")
    if int(max_cg_iter) < 1:
        raise ValueError(f"{who}: max_cg_iter must be at least 1, got {max_cg_iter}")
    if probes is None:
        if int(num_probes) < 1:
            raise ValueError(f"{who}: num_probes must be at least 1, got {num_probes}")
    else:
        if not isinstance(probes, torch.Tensor) or probes.layout != torch.strided or probes.dim() != 2 or probes.size(0) != n \
                or probes.size(1) < 1:
            raise ValueError(f"{who}: probes must be a dense ({n}, k) block, got "
                             f"{tuple(probes.shape) if isinstance(probes, torch.Tensor) else type(probes).__name__}")
        if probes.dtype != A.dtype:
            raise ValueError(f"{who}: probes must have A's dtype, got {probes.dtype} and {A.dtype}")
        if probes.device != A.device:
            raise RuntimeError(f"{who}: probes must be on the device of A, got {probes.device} and {A.device}")
    if B is not None:
        if not isinstance(B, torch.Tensor) or B.layout != torch.strided:
            raise ValueError(f"{who}: B must be a dense (strided) tensor")
        if B.dim() not in (1, 2) or B.size(0) != n or (B.dim() == 2 and B.size(1) < 1):
            raise ValueError(f"{who}: B must have shape ({n},) or ({n}, m), got {tuple(B.shape)}")
        if B.dtype != A.dtype:
            raise ValueError(f"{who}: B must have A's dtype, got {B.dtype} and {A.dtype}")
        if B.device != A.device:
            raise RuntimeError(f"{who}: B must be on the device of A, got {B.device} and {A.device}")


def _run(who, A, B, num_probes, lanczos_steps, probes, seed, cg_tolerance, max_cg_iter, return_info):
    _check(who, A, B, num_probes, lanczos_steps, probes, max_cg_iter)
    empty = torch.empty((A.size(0), 0), dtype=A.dtype, device=A.device)
    logdet, inv_quad, est, lens, rnorm, iters = SparseLogDet.apply(
        A, empty if B is None else B, empty if probes is None else probes, int(num_probes), int(lanczos_steps), int(seed),
        float(cg_tolerance), int(max_cg_iter), who)
    if not return_info:
        return logdet, inv_quad, None
    k = est.numel()
    stderr = est.std(unbiased=True) / math.sqrt(k) if k > 1 else torch.full((), float("nan"), dtype=est.dtype, device=est.device)
    return logdet, inv_quad, {"estimates": est, "lengths": lens, "iterations": [int(i) for i in iters.tolist()], "residual_norms": rnorm,
                              "stderr": stderr}


def sparse_logdet(A: torch.Tensor, *, num_probes: int = 16, lanczos_steps: int = 30, probes: torch.Tensor = None, seed: int = 0,
                  cg_tolerance: float = 1e-4, max_cg_iter: int = 1000, return_info: bool = False):
    r"""``log det A`` (a scalar tensor) of the sparse symmetric positive definite ``A``, differentiable with respect to ``A``.

    ``A``   2-D square COO or CSR, float32 or float64, int32 or int64 indices; taken as symmetric positive definite (not checked: an
            indefinite ``A`` is noticed when a Lanczos matrix has a non-positive eigenvalue, and raises).  Batched and bfloat16
            operands are refused.
    ``num_probes`` / ``seed``   the generated Rademacher block: ``(n, num_probes)`` of ±1, a pure function of ``(seed, row, column)``.
    ``probes``  an ``(n, k)`` block of ``A``'s dtype and device that replaces it: ``logdet = (n / ‖Z‖_F²) Σ_c ‖z_c‖²·quad_c`` — the mean
            ``(1/k) Σ_c`` for columns of squared norm ``n``, and exact for ``probes = I``.
    ``lanczos_steps``   rows of each tridiagonal matrix at most (``[1, steps cap]``, the cap is 128): CG runs at least that many
            iterations; a column's matrix ends earlier where its Krylov space is exhausted.
    ``cg_tolerance`` / ``max_cg_iter``   the stop rule of the CG run, as ``linear_cg``'s: mean normalised residual norm, tested once
            the history is full.  A run that ends at ``max_cg_iter`` warns with ``linear_cg``'s text.
    ``return_info``     also return a dict: ``estimates`` (the per-probe values ``‖z_c‖²·quad_c``), ``lengths`` (rows of each
            matrix), ``iterations`` (of each CG run: one per 256 columns), ``residual_norms`` (normalised, per column),
            ``stderr`` (the sample standard deviation of ``estimates`` over ``√k``).

    The gradient is the Hutchinson estimate of ``A⁻¹`` on ``A``'s pattern from the same CG run, a sparse tensor on ``A``'s own index
    tensors; its entries carry the solver's error, at most ``cg_tolerance / λ_min(A)`` each for ``probes = I``.  Differentiable
    once."""
    logdet, _, info = _run("sparse_logdet", A, None, num_probes, lanczos_steps, probes, seed, cg_tolerance, max_cg_iter, return_info)
    return (logdet, info) if return_info else logdet


def sparse_inv_quad_logdet(A: torch.Tensor, B: torch.Tensor, *, num_probes: int = 16, lanczos_steps: int = 30, probes: torch.Tensor = None,
                           seed: int = 0, cg_tolerance: float = 1e-4, max_cg_iter: int = 1000, return_info: bool = False):
    r"""``(inv_quad, logdet)``: ``inv_quad_j = b_jᵀ A⁻¹ b_j`` for every column of the dense ``B`` — shape ``()`` for ``B`` of shape
    ``(n,)``, ``(m,)`` for ``(n, m)`` — and ``log det A`` as :func:`sparse_logdet`, from ONE CG run over ``[Z | B]``.  Both are
    differentiable with respect to ``A`` (sparse, on ``A``'s pattern) and ``inv_quad`` with respect to ``B`` (``2 A⁻¹ B``)."""
    if B is None:
        raise ValueError("sparse_inv_quad_logdet: B must be a dense (strided) tensor")
    logdet, inv_quad, info = _run("sparse_inv_quad_logdet", A, B, num_probes, lanczos_steps, probes, seed, cg_tolerance, max_cg_iter,
                                  return_info)
    return (inv_quad, logdet, info) if return_info else (inv_quad, logdet)


class SparseLogDet(torch.autograd.Function):
    """Autograd function behind both entries: ``apply(A, B, probes, num_probes, lanczos_steps, seed, cg_tolerance, max_cg_iter, who)``
    with ``(n, 0)`` blocks for an absent ``B`` / ``probes``; returns ``(logdet, inv_quad, estimates, lengths, residual_norms,
    iterations)``, the last four not differentiable."""

    @staticmethod
    def forward(ctx, A, B, probes, num_probes, lanczos_steps, seed, cg_tolerance, max_cg_iter, who):
        A, B, probes = A.detach(), B.detach(), probes.detach()
        n, dtype, dev = A.size(0), A.dtype, A.device
        vector = B.dim() == 1
        Bm = B.unsqueeze(1) if vector else B
        Z = probes if probes.size(1) else _be.rademacher_fill(n, num_probes, seed, dtype, dev)
        k, m = Z.size(1), Bm.size(1)
        cg_op = SparseOperator(A)
        quad = _be.tridiag_quadrature if A.is_cuda else _cpu_quadrature
        rhs = torch.cat((Z, Bm), dim=1) if m else Z
        n_hist = min(lanczos_steps, n)
        sols, ests, infos, bads, rnorms, iters, reached, fused = [], [], [], [], [], [], True, True
        for c0 in range(0, k + m, _CHUNK):
            c1 = min(c0 + _CHUNK, k + m)
            x, hist, k_done, rnorm, done, norm, on_kernels = _cg_with_history(cg_op, rhs[:, c0:c1], n_hist, cg_tolerance, max_cg_iter,
                                                                              _STOP_AFTER)
            fused = fused and on_kernels
            sols.append(x)
            rnorms.append(rnorm)
            iters.append(k_done)
            if not done:
                reached = False
                _warn_tolerance_missed(k_done, rnorm.mean(), cg_tolerance)
            kz = min(c1, k) - c0         # probe columns of this chunk: they lead
            if kz > 0:
                est, info = quad(hist, _be.QUAD_CG, _be.QUAD_LOG, scale=(norm[:kz] * norm[:kz]), p=kz)
                ests.append(est)
                infos.append(info)
                # CG zeroes alpha where p'Ap is not positive, which ends the matrix as a frozen column does — but a frozen column's
                # residual is below _STOP_AFTER.  A matrix that ends early under a live residual met a direction of non-positive
                # curvature: the same verdict as a non-positive eigenvalue.
                bads.append((info < 0) | ((info.abs() < min(n_hist, k_done)) & (rnorm[:kz] >= _STOP_AFTER)))
        est, info, rnorm, bad = torch.cat(ests), torch.cat(infos), torch.cat(rnorms), torch.cat(bads)
        X = torch.cat(sols, dim=1) if len(sols) > 1 else sols[0]
        record_solve(solver="sparse_logdet", iterations=max(iters), tolerance_reached=reached, residual_norm=rnorm.detach().clone(),
                     tolerance=float(cg_tolerance), fused=fused)
        if bool(bad.any()):        # (the one host read of the quadrature; the CG driver has already read its counters)
            raise RuntimeError("sparse_logdet: A is not positive definite (a Lanczos tridiagonal has a non-positive eigenvalue)")
        # Σ_c ‖z_c‖²·quad_c estimates (‖Z‖_F² / n)·tr log A: the weight is 1/k for columns of squared norm n (every Rademacher
        # column, exactly) and 1 for probes = I
        weight = 1.0 / k if not probes.size(1) else n / (Z * Z).sum()
        logdet = est.sum() * weight
        U, Xb = X[:, :k], X[:, k:]
        inv_quad = _be.coldot(Bm, Xb) if m else torch.zeros(0, dtype=dtype, device=dev)
        if vector:
            inv_quad = inv_quad.reshape(())
        ctx.op = _Operand(A)
        ctx.vector, ctx.weight, ctx.m = vector, weight, m
        ctx.save_for_backward(Z, U, Xb)
        lens = info.abs()
        iters_t = torch.tensor(iters, dtype=torch.int64)
        ctx.mark_non_differentiable(est, lens, rnorm, iters_t)
        return logdet, inv_quad, est, lens, rnorm, iters_t

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logdet, g_iq, *_unused):  # type: ignore[override]
        Z, U, Xb = ctx.saved_tensors
        op: _Operand = ctx.op
        m = ctx.m
        gradA = gradB = None
        g_iq = None if (g_iq is None or m == 0) else g_iq.to(Xb.dtype).reshape(1, m)
        if ctx.needs_input_grad[0]:
            # gradA = g·(weight/2)·mask(U Zᵀ + Z Uᵀ) − Σ_j g_j·mask(x_j x_jᵀ): one SDDMM over the concatenated columns
            left, right = [], []
            if g_logdet is not None:
                w = g_logdet.to(U.dtype) * ctx.weight / 2
                left += [U * w, Z * w]
                right += [Z, U]
            if g_iq is not None:
                left.append(Xb * (-g_iq))
                right.append(Xb)
            if left:
                G = torch.cat(left, dim=1) if len(left) > 1 else left[0]
                R = torch.cat(right, dim=1) if len(right) > 1 else right[0]
                if op.plan.perm is None:
                    gvals = _ops.sddmm(op.plan, G.contiguous(), R.contiguous())
                else:   # un-coalesced COO: one gradient entry per stored duplicate, in A's own order
                    gvals = _be.coo_sddmm(op.indices[0], op.indices[1], G.contiguous(), R.contiguous())
                gradA = op.rebuild(gvals)
        if ctx.needs_input_grad[1] and g_iq is not None:
            gradB = Xb * (2 * g_iq)
            if ctx.vector:
                gradB = gradB.reshape(-1)
        return gradA, gradB, None, None, None, None, None, None, None


def _cpu_quadrature(hist, kind, fn, scale=None, p=None):
    from . import _cpu

    return _cpu.tridiag_quadrature(hist, kind, fn, scale=scale, p=p)
