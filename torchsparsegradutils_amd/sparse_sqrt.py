"""``sparse_inv_sqrt_mm`` / ``sparse_sqrt_mm`` — ``A^{-1/2}·B`` and ``A^{1/2}·B`` for a sparse symmetric positive definite matrix by
contour-integral quadrature (CIQ), with gradients that stay on the matrix's pattern.

    A^{-1/2} ≈ r(A) = Σ_{q=1..N} ω_q (A + σ_q I)^{-1}

is method 3 of Hale, Higham and Trefethen (2008) for the spectrum interval ``[lo, hi]``: with ``k² = lo/hi``, ``m' = 1 − k²`` and
``K' = K(m')``, the nodes are ``u_q = (q − ½) K'/N``, the shifts ``σ_q = lo·sn²/cn²`` and the weights ``ω_q = 2 K' √lo/(π N)·dn/cn²``
(Jacobi elliptic functions of ``(u_q | m')``).  Twelve nodes give 1e-8 relative at a condition number of 1e4 (DESIGN.md §6 has the
table).  The ``N`` shifted solves share one Krylov space: multi-shift MINRES on the Lanczos vectors of ``(A, b_c)``.

What it is for.  With the precision matrix ``Q`` of a Gaussian Markov random field, ``x = μ + Q^{-1/2} z`` with ``z ~ N(0, I)`` is a
draw from ``N(μ, Q⁻¹)`` — no factorisation, only products with ``Q``; the same product whitens residuals (``Q^{1/2} r`` or
``Σ^{-1/2} r`` has identity covariance).  ``sparse_sqrt_mm`` is ``A·(A^{-1/2} B)``.

On the GPU one iteration is the Lanczos step and the Givens phase of the MINRES kernels (``csrc/minres.hip``) followed by
``tsgu_ciq_update`` (``csrc/ciq_impl.h``), which walks the rows once, keeps ``Σ_q ω_q·update_q`` in registers and never stores the
``N`` solutions, and ``tsgu_ciq_stop``, which stops each column on MINRES's own residual estimates: no reductions, one stop launch and one
host read of the stop word every 10 iterations, hipGraph replay of 10-iteration chunks.  CPU operands take the torch-op path (``_cpu.ciq_apply``:
the unfused ``minres(A, B, shifts=σ)`` and the weighted sum).

Gradients.  ``r`` is a rational function of ``A``, so its derivative is exact for the approximant: ``grad_B = r(A)·G`` (one more
run of the same loop) and ``grad_A[i,j] = −Σ_q ω_q Σ_c x^g_q[i,c]·x^b_q[j,c]`` at ``A``'s stored entries, with
``x^b_q = (A+σ_q)⁻¹B`` and ``x^g_q = (A+σ_q)⁻¹G`` — one SDDMM over ``N·p`` columns on ``A``'s own index tensors, unsymmetrised, as
``sparse_generic_solve`` returns its ``gradA``.  The bounds and the rule are constants of the call.

Preconditioning is not supported: a preconditioned Lanczos process builds the Krylov space of ``M⁻¹A``, whose shifted systems are
not those of ``A``.  Out of scope: batched ``A``, bfloat16, double backward.
"""

from __future__ import annotations

import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _ops
from .sparse_matmul import _Operand, sparse_mm
from .utils import _graph
from .utils._operator import SparseOperator, record_solve
from .utils.linear_cg import _cg_with_history

__all__ = ["sparse_inv_sqrt_mm", "sparse_sqrt_mm", "SparseInvSqrtMM"]

_MAX_QUAD = 32         # shifts of one tsgu_ciq_update launch (csrc/ciq_impl.h: kCiqShiftCap)
_SDDMM_WIDTH = 1024    # columns of one SDDMM call of the backward; wider N·p blocks are split by shifts and added
_EPS = 1e-25           # the Givens phase's floor on beta (minres's `eps`)
_STOP_EVERY = 10       # iterations between two tsgu_ciq_stop launches: once per chunk, where the host reads the stop word, as the
                       # stopping tests of linear_cg and minres (at every iteration the launch is 3 % of an
                       # iteration on the C3 pattern, and a column frozen between two host reads only gives accuracy away)
_STOP_AFTER = 1e-10    # the bounds run: a CG column below this residual is frozen (sparse_logdet's rule)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------

def _agm_scale(m: float):
    """The AGM scale of parameter m (Abramowitz and Stegun 16.4, 17.6): a₀ = 1, b₀ = √(1 − m), c₀ = √m, then
    a_{j+1} = (a_j + b_j)/2, b_{j+1} = √(a_j b_j), c_{j+1} = (a_j − b_j)/2 until c vanishes in float64.  Returns (a, c)."""
    a, b, c = [1.0], [math.sqrt(1.0 - m)], [math.sqrt(m)]
    while abs(c[-1]) > 1e-17 * a[-1] and len(a) < 64:
        a.append(0.5 * (a[-1] + b[-1]))
        c.append(0.5 * (a[-2] - b[-1]))
        b.append(math.sqrt(a[-2] * b[-1]))
    return a, c


def _ellipk(m: float) -> float:
    """K(m), the complete elliptic integral of the first kind with parameter m < 1: π / (2·AGM(1, √(1 − m)))."""
    a, _ = _agm_scale(m)
    return math.pi / (2.0 * a[-1])


def _ellipj(u: np.ndarray, m: float):
    """(sn, cn, dn) of (u | m) by the descending Landen recurrence on the AGM scale: φ_N = 2^N a_N u, then
    φ_{j−1} = (φ_j + asin(c_j sin φ_j / a_j)) / 2; sn = sin φ₀, cn = cos φ₀, dn = √(cn² + (1 − m)·sn²) (no cancellation near u = K)."""
    a, c = _agm_scale(m)
    n = len(a) - 1
    phi = (2.0 ** n) * a[n] * np.asarray(u, dtype=np.float64)
    for j in range(n, 0, -1):
        phi = 0.5 * (phi + np.arcsin(np.clip(c[j] * np.sin(phi) / a[j], -1.0, 1.0)))
    sn, cn = np.sin(phi), np.cos(phi)
    return sn, cn, np.sqrt(cn * cn + (1.0 - m) * sn * sn)


def _ciq_rule(lo: float, hi: float, num_quad: int):
    """(σ, ω): float64 arrays of the ``num_quad`` shifts and weights of A^{-1/2} ≈ Σ ω_q (A + σ_q I)⁻¹ for a spectrum in [lo, hi]."""
    lo, hi, N = float(lo), float(hi), int(num_quad)
    if not (0.0 < lo <= hi and math.isfinite(hi)):
        raise ValueError(f"_ciq_rule: 0 < lo <= hi expected, got ({lo}, {hi})")
    mp = 1.0 - lo / hi
    Kp = _ellipk(mp)
    u = (np.arange(1, N + 1, dtype=np.float64) - 0.5) * Kp / N
    sn, cn, dn = _ellipj(u, mp)
    sigma = lo * (sn * sn) / (cn * cn)
    omega = (2.0 * Kp * math.sqrt(lo) / (math.pi * N)) * dn / (cn * cn)
    return sigma, omega


# ---- checks ------------------------------------------------------------------------------------------------------------------------

def _check_operands(who: str, A, B) -> None:
    """The checks every matrix function of a sparse symmetric A applied to a dense block B shares (sparse_expm.py uses them too)."""
    if not isinstance(A, torch.Tensor):
        raise ValueError(f"{who}: A should be an instance of torch.Tensor")
    if A.layout not in (torch.sparse_coo, torch.sparse_csr):
        raise ValueError(f"{who}: A should be in either COO or CSR sparse format")
    if A.dense_dim() != 0:
        raise ValueError(f"{who}: A must be a 2-D sparse matrix (hybrid operands are not supported), got {A.dense_dim()} dense dimensions")
    if A.dim() != 2:
        raise ValueError(f"{who}: A must be a 2-D sparse matrix (batched operands are not supported), got {A.dim()} dimensions")
    if A.size(0) != A.size(1):
        raise ValueError(f"{who}: A must be square, got {tuple(A.shape)}")
    if A.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: float32 and float64 operands only, got {A.dtype}")
    n = A.size(0)
    if not isinstance(B, torch.Tensor) or B.layout != torch.strided:
        raise ValueError(f"{who}: B must be a dense (strided) tensor")
    if B.dim() not in (1, 2) or B.size(0) != n or (B.dim() == 2 and B.size(1) < 1):
        raise ValueError(f"{who}: B must have shape ({n},) or ({n}, p), got {tuple(B.shape)}")
    if B.dtype != A.dtype:
        raise ValueError(f"{who}: B must have A's dtype, got {B.dtype} and {A.dtype}")
    if B.device != A.device:
        raise RuntimeError(f"{who}: B must be on the device of A, got {B.device} and {A.device}")


def _check(who: str, A, B, num_quad, bounds, tolerance, max_iter, lanczos_steps):
    _check_operands(who, A, B)
    if not 1 <= int(num_quad) <= _MAX_QUAD:
        raise ValueError(f"{who}: num_quad must lie in [1, {_MAX_QUAD}], got {num_quad}")
    if int(max_iter) < 1:
        raise ValueError(f"{who}: max_iter must be at least 1, got {max_iter}")
    if not float(tolerance) > 0.0:
        raise ValueError(f"{who}: tolerance must be positive, got {tolerance}")
    if bounds is None:
        if int(lanczos_steps) < 1:
            raise ValueError(f"{who}: lanczos_steps must be at least 1, got {lanczos_steps}")
    else:
        try:
            lo, hi = (float(b) for b in bounds)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bounds must be a pair (lo, hi) of floats or None, got {bounds!r}") from None
        if not (0.0 < lo <= hi and math.isfinite(hi)):
            raise ValueError(f"{who}: bounds must satisfy 0 < lo <= hi, got ({lo}, {hi})")


def _not_spd(who: str):
    return ValueError(f"{who}: A is not positive definite (a Lanczos tridiagonal has a non-positive eigenvalue)")


def _estimate_bounds(who: str, A: torch.Tensor, lanczos_steps: int, seed: int):
    """(0.5·θ_min, 1.1·θ_max) of the Lanczos matrix of (A, one Rademacher column) after ``lanczos_steps`` CG steps: T from the CG
    coefficients by the "kind 0" formulas of csrc/tsgu_hip_quadrature.h, its eigenvalues on the host."""
    n = A.size(0)
    steps = max(1, min(int(lanczos_steps), n))
    z = _be.rademacher_fill(n, 1, seed, A.dtype, A.device)
    _, hist, k_done, rnorm, _, _, _ = _cg_with_history(SparseOperator(A), z, steps, 0.0, steps, _STOP_AFTER)
    h = hist[:, :, 0].detach().to("cpu", torch.float64).numpy()
    alpha, beta = h[:, 0], h[:, 1]
    bad_a = ~((alpha > 0) & np.isfinite(alpha))
    bad_b = ~((beta > 0) & np.isfinite(beta))
    r = int(np.argmax(bad_a)) if bad_a.any() else len(alpha)
    if bad_b[:r].any():
        r = min(r, int(np.argmax(bad_b)) + 1)
    # a matrix that ends before CG did under a live residual met a direction of non-positive curvature (sparse_logdet's verdict)
    if r == 0 or (r < min(steps, k_done) and float(rnorm.reshape(-1)[0]) >= _STOP_AFTER):
        raise _not_spd(who)
    ia = 1.0 / alpha[:r]
    d = ia.copy()
    d[1:] += (beta[:r] * ia)[:-1]
    e = (np.sqrt(beta[:r]) * ia)[:-1]
    theta = np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
    if not (np.all(np.isfinite(theta)) and theta[0] > 0):
        raise _not_spd(who)
    return 0.5 * float(theta[0]), 1.1 * float(theta[-1])


# ---- the fused loop ----------------------------------------------------------------------------------------------------------------

def _tiny(dtype: torch.dtype) -> float:
    return math.sqrt(torch.finfo(dtype).tiny)


def _ciq_fused(op: SparseOperator, rhs: torch.Tensor, sigma: torch.Tensor, omega: torch.Tensor, tolerance: float, max_iter: int,
               want_keep: bool, stop_every: int = _STOP_EVERY):
    """r(A)·rhs for the (n, p) block ``rhs`` on the HIP kernels.  Returns (result, keep [n][S][p] of the per-shift solutions of the
    NORMALISED columns or None, column norms, iterations, all columns done, residual estimates (p,)).  ``stop_every``: the stop
    kernel runs on every k-th iteration of a chunk (k divides 10; default: the last one, just before the host reads the stop word);
    tools/ciqbench.py passes 1 and 10 to measure what the launch costs."""
    n, p = rhs.shape
    S = sigma.numel()
    dev, dtype = rhs.device, rhs.dtype
    vt = _be.vtype_of(rhs)
    cap, align, _, _ = _be.ciq_geometry(dtype, n, p)
    if S > cap:
        raise RuntimeError(f"tsgu_ciq_update takes at most {cap} shifts, got {S}")
    nb = _be.krylov_num_blocks("sparse_inv_sqrt_mm", rhs, n, p)
    lib = _be.load_library()

    norm = _be.coldot(rhs, rhs).sqrt_()
    is_zero = norm.lt(_tiny(dtype))
    norm = norm.masked_fill(is_zero, 1)
    z = [torch.zeros_like(rhs), rhs.div(norm.unsqueeze(0))]      # [z two steps back, z one step back]: unit columns, beta_0 = 1
    prod = torch.empty_like(rhs)
    plane = -(-n * p // align) * align                           # per-shift planes start on 16-byte boundaries
    w = [torch.zeros((S, plane), dtype=dtype, device=dev), torch.zeros((S, plane), dtype=dtype, device=dev)]
    acc = torch.zeros_like(rhs)
    keep = torch.zeros((n, S, p), dtype=dtype, device=dev) if want_keep else None
    scal = torch.zeros((S, 12, p), dtype=dtype, device=dev)
    scal[0, 1] = 1
    scal[0, 11] = 1
    scal[:, 6] = 1                                               # scale_prev = beta_0
    scal[:, 2] = 1
    scal[:, 4] = 1
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    done = is_zero.to(torch.int32)                               # a zero column is done before it starts: its result stays zero
    est = torch.zeros(p, dtype=dtype, device=dev)
    part = torch.empty((nb, p), dtype=dtype, device=dev)
    fold = torch.empty((lib.tsgu_cg_fold_rows(), p), dtype=dtype, device=dev)

    def scalar(phase, partial, rows):
        _be.launch("tsgu_minres_scalar_ms", dev, vt, phase, partial, rows, 0, fold, scal, flags, _EPS, float(tolerance), sigma, S, 1.0, p)

    checked = [True]

    def iteration(j):
        _, pqq = op.matmul_with_dot(z[1], out=prod)             # A z with <z, A z> partials
        scalar(0, pqq, pqq.shape[0])
        _be.launch("tsgu_minres_vector_ms", dev, vt, 0, n, p, z[0], z[1], prod, None, None, None, scal, flags, part, nb * p, 0, S, plane,
                   1.0)                                          # z_c over z two steps back, |z_c|^2 partials
        scalar(1, part, nb)                                      # beta_c, the rotations, sub / subsub / diag / scale of every shift
        _be.ciq_update(z[0], z[1], w[0], w[1], plane, acc, keep, scal, omega, done, flags)
        checked[0] = (j + 1) % stop_every == 0
        if checked[0]:
            _be.ciq_stop(scal, tolerance, est, done, flags)
        z.reverse()                                              # the buffer that held z two steps back now holds z_c
        w.reverse()

    def restore(roles):                                          # a refused capture ran nothing: undo the recorded role swaps
        z[:], w[:] = roles

    with torch.cuda.device(dev):
        i, stopped = _graph.run_chunked(iteration, lambda: bool(flags[0].item()), 10, bound=min(int(max_iter), n + 1),
                                        capturable=_graph.enabled(), snapshot=lambda: (z[:], w[:]), restore=restore)
        if not stopped and not checked[0]:                       # the bound cut a chunk short between two stop launches
            _be.ciq_stop(scal, tolerance, est, done, flags)
            stopped = bool(flags[0].item())
        iters = int(flags[1].item()) if stopped else i
    est = est.masked_fill(is_zero, 0)
    return acc.mul_(norm.unsqueeze(0)), keep, norm, iters, bool(stopped), est


def _apply_rule(A, op, Bm, sigma, omega, tolerance, max_iter, want_keep):
    """r(A)·Bm on either device: (result, keep or None, column scales of keep, info)."""
    if Bm.is_cuda:
        if op is None:
            op = SparseOperator(A)
        out, keep, norm, iters, done, est = _ciq_fused(op, Bm.contiguous(), sigma, omega, tolerance, max_iter, want_keep)
        return out, keep, norm, {"iterations": iters, "converged": done, "residual_estimates": est, "fused": True}
    from . import _cpu

    out, keep, est = _cpu.ciq_apply(A, Bm, sigma, omega, tolerance, max_iter, want_keep)
    info = {"iterations": None, "converged": bool((est <= tolerance).all()), "residual_estimates": est, "fused": False}
    return out, keep, None, info


# ---- the autograd function -----------------------------------------------------------------------------------------------------------

class SparseInvSqrtMM(torch.autograd.Function):
    """Autograd function behind :func:`sparse_inv_sqrt_mm`: ``apply(A, B, sigma, omega, tolerance, max_iter, info)`` with the rule as
    float64 numpy arrays and ``info`` a dict the forward fills (or None); returns ``r(A)·B`` in ``B``'s shape."""

    @staticmethod
    def forward(ctx, A, B, sigma, omega, tolerance, max_iter, info):
        A, B = A.detach(), B.detach()
        vector = B.dim() == 1
        Bm = B.unsqueeze(1) if vector else B
        sig_t = torch.as_tensor(sigma, dtype=A.dtype).to(A.device)
        om_t = torch.as_tensor(omega, dtype=A.dtype).to(A.device)
        want_keep = bool(ctx.needs_input_grad[0])
        out, keep, norm, run = _apply_rule(A, None, Bm, sig_t, om_t, tolerance, max_iter, want_keep)
        record_solve(solver="sparse_inv_sqrt_mm", iterations=run["iterations"], tolerance_reached=run["converged"],
                     tolerance=float(tolerance), shifts=int(sig_t.numel()), fused=run["fused"])
        if info is not None:
            info.update(run)
        ctx.A, ctx.vector, ctx.tolerance, ctx.max_iter = A, vector, tolerance, max_iter
        ctx.save_for_backward(sig_t, om_t, keep, norm)
        return out.squeeze(1) if vector else out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):  # type: ignore[override]
        sig_t, om_t, keep_b, norm_b = ctx.saved_tensors
        A = ctx.A
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_a or need_b):
            return (None,) * 7
        Gm = (G.unsqueeze(1) if ctx.vector else G).to(A.dtype)
        gB, keep_g, norm_g, _ = _apply_rule(A, None, Gm, sig_t, om_t, ctx.tolerance, ctx.max_iter, bool(need_a))
        gradA = gradB = None
        if need_b:
            gradB = gB.squeeze(1) if ctx.vector else gB
        if need_a:
            # gradA = −Σ_q ω_q Σ_c x^g_q[i,c] x^b_q[j,c] on the stored entries: keep holds the solutions of the normalised columns
            n, S, p = keep_g.shape
            col = om_t.reshape(S, 1)
            if norm_g is not None:
                col = col * (norm_g * norm_b).reshape(1, p)
            keep_g.mul_(col.reshape(1, S, -1))
            op = _Operand(A)
            step = S if S * p <= _SDDMM_WIDTH else max(1, _SDDMM_WIDTH // p)
            gvals = None
            for q0 in range(0, S, step):
                q1 = min(S, q0 + step)
                if q0 == 0 and q1 == S:
                    left, right = keep_g.reshape(n, S * p), keep_b.reshape(n, S * p)
                else:
                    left = keep_g[:, q0:q1].reshape(n, (q1 - q0) * p)
                    right = keep_b[:, q0:q1].reshape(n, (q1 - q0) * p)
                if op.plan.perm is None:
                    part = _ops.sddmm(op.plan, left.contiguous(), right.contiguous())
                else:
                    part = _be.coo_sddmm(op.indices[0], op.indices[1], left.contiguous(), right.contiguous())
                gvals = part if gvals is None else gvals.add_(part)
            gradA = op.rebuild(gvals.neg_())
        return gradA, gradB, None, None, None, None, None


# ---- the public entries ---------------------------------------------------------------------------------------------------------------

def sparse_inv_sqrt_mm(A: torch.Tensor, B: torch.Tensor, *, num_quad: int = 12, bounds=None, tolerance: float = 1e-4,
                       max_iter: int = 1000, lanczos_steps: int = 30, seed: int = 0, return_info: bool = False):
    r"""``A^{-1/2}·B`` for the sparse symmetric positive definite ``A``, in ``B``'s shape, differentiable with respect to both.

    With a GMRF's precision matrix ``Q``, ``μ + sparse_inv_sqrt_mm(Q, z)`` for ``z ~ N(0, I)`` is a draw from ``N(μ, Q⁻¹)``; applied
    to residuals the product whitens them.

    ``A``   2-D square COO (coalesced first) or CSR, float32 or float64, int32 or int64 indices; taken as symmetric positive
            definite.  Batched, hybrid and bfloat16 operands are refused.
    ``B``   dense ``(n,)`` or ``(n, p)`` with ``A``'s dtype and device.  A zero column gives a zero column.
    ``num_quad``    nodes of the rule (``[1, 32]``): 8 give 3e-7, 12 give 1e-10 and 15 give 2e-13 relative at a condition number of
            1e3; the error grows slowly with the condition number.
    ``bounds``      ``(lo, hi)`` enclosing ``A``'s spectrum, as Python floats: used as given, with no host synchronisation besides the
            loop's polls of its stop word.  ``None`` estimates them: ``lanczos_steps`` CG steps on one Rademacher column
            (``seed``), the extreme eigenvalues of the Lanczos matrix on the host, widened to ``(0.5·θ_min, 1.1·θ_max)`` — too wide
            costs little, too narrow does not.  A matrix the run shows not to be positive definite raises ``ValueError``.
    ``tolerance`` / ``max_iter``    every column stops once MINRES's residual estimate of each of its shifted systems, relative
            to the column's norm, is at most ``tolerance``, tested every 10 iterations (as ``linear_cg`` and ``minres`` test
            theirs); ``max_iter`` (and ``n + 1``) bounds the iterations.  A run that ends
            there does not raise: ``return_info`` tells.
    ``return_info``     also return a dict: ``iterations``, ``converged``, ``bounds``, ``num_quad``, ``residual_estimates``
            (per column, the largest over the shifts) and ``fused`` (whether the HIP loop ran; CPU operands report the true
            residuals of the unfused solver, and no iteration count).

    The gradient with respect to ``A`` is a sparse tensor on ``A``'s own index tensors (stored entries only, unsymmetrised); the
    bounds and the rule are constants of the call.  Preconditioning is not supported.  Differentiable once."""
    return _entry("sparse_inv_sqrt_mm", A, B, num_quad, bounds, tolerance, max_iter, lanczos_steps, seed, return_info, False)


def sparse_sqrt_mm(A: torch.Tensor, B: torch.Tensor, *, num_quad: int = 12, bounds=None, tolerance: float = 1e-4,
                   max_iter: int = 1000, lanczos_steps: int = 30, seed: int = 0, return_info: bool = False):
    r"""``A^{1/2}·B = A·(A^{-1/2}·B)``: :func:`sparse_inv_sqrt_mm` followed by ``sparse_mm``, same arguments and ``info``.  With a
    covariance matrix ``Σ``, ``μ + sparse_sqrt_mm(Σ, z)`` is a draw from ``N(μ, Σ)``.  Preconditioning is not supported."""
    return _entry("sparse_sqrt_mm", A, B, num_quad, bounds, tolerance, max_iter, lanczos_steps, seed, return_info, True)


def _entry(who, A, B, num_quad, bounds, tolerance, max_iter, lanczos_steps, seed, return_info, times_a):
    _check(who, A, B, num_quad, bounds, tolerance, max_iter, lanczos_steps)
    if A.layout == torch.sparse_coo and not A.is_coalesced():
        A = A.coalesce()
    if bounds is None:
        lo, hi = _estimate_bounds(who, A.detach(), lanczos_steps, seed)
    else:
        lo, hi = (float(b) for b in bounds)
    sigma, omega = _ciq_rule(lo, hi, int(num_quad))
    info = {"bounds": (lo, hi), "num_quad": int(num_quad)} if return_info else None
    out = SparseInvSqrtMM.apply(A, B, sigma, omega, float(tolerance), int(max_iter), info)
    if times_a:
        out = sparse_mm(A, out.unsqueeze(1)).squeeze(1) if out.dim() == 1 else sparse_mm(A, out)
    return (out, info) if return_info else out
