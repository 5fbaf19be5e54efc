"""``gmres`` — restarted GMRES(m), right-preconditioned, for general (non-symmetric) ``A``.  The reference has no counterpart:
the interface follows ``bicgstab`` (a settings tuple, ``max(abstol, reltol·‖r₀‖)`` as the threshold of every column).

All right-hand sides advance in lock-step on the Arnoldi kernels of ``csrc/gmres.hip`` (contracts: ``csrc/tsgu_hip_gmres.h``):
every column has its own basis, Hessenberg column, rotations, stopping point and iteration count on the device, and a finished
column is frozen.  An inner step orthogonalises with classical Gram–Schmidt and one re-orthogonalisation (two global reductions
instead of the ``j + 1`` dependent ones of modified Gram–Schmidt).  One restart cycle is one chunk of ``_graph.run_chunked``: the
host reads one stop word per cycle, and a long solve replays the cycle as a hipGraph.  A column is finished only on the TRUE
residual recomputed at a cycle start (or at ``maxiter``): a rotation estimate that has drifted costs another cycle, never a wrong
answer.

``gmres_t`` solves ``Aᵀx = b``; ``sparse_generic_solve(A, B, solve=gmres, transpose_solve=gmres_t)`` is the pair that gives the
right gradients for a nonsymmetric ``A`` (``solve=gmres`` alone is mirrored to both, which is right only for symmetric ``A``).

Where the fused path does not apply (``ENABLE_FUSED = False``, CPU operands, dtypes other than fp32 / fp64, ``restart`` above the
kernels' cap) the same algorithm runs as torch ops, ``_gmres_torch``: one code path for CPU and GPU tensors.
"""

from __future__ import annotations

import logging
from typing import Callable, NamedTuple, Optional, Union

import torch

from .. import _backend as _be
from .. import _ops
from . import _graph
from ._operator import LAST_SOLVE, SparseOperator, as_operator, checked, record_solve

ENABLE_FUSED = True  # False: the torch-op path on every device (tests compare the two)

_null_log = logging.getLogger("gmres")
_null_log.disabled = True


class GMRESSettings(NamedTuple):
    restart: int = 30
    maxiter: Optional[int] = None        # inner steps (= products with A) per column; default 2·n
    abstol: float = 1.0e-8
    reltol: float = 1.0e-6
    precon: Optional[Union[torch.Tensor, Callable]] = None   # right preconditioner M ≈ A⁻¹
    flexible: bool = False               # store Z_j = M·V_j: M may change between applications
    transpose: bool = False              # solve Aᵀx = b
    logger: logging.Logger = _null_log


def _block(t: torch.Tensor, dtype) -> torch.Tensor:
    """What an operator or a preconditioner returned, as an operand of the kernels: one dtype, contiguous, on a 16-byte boundary
    (a contiguous view at an odd offset is copied)."""
    t = checked(t, dtype).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _operator(matmul_closure, transpose: bool):
    """(v -> A v or Aᵀ v, whether that is this package's sparse product in `dtype`)."""
    if not transpose:
        op = as_operator(matmul_closure)
        return op, (op.dtype if isinstance(op, SparseOperator) else None)
    if torch.is_tensor(matmul_closure):
        if matmul_closure.layout in (torch.sparse_csr, torch.sparse_coo):
            op = SparseOperator(matmul_closure)
            plan_t = op.plan.transposed
            return (lambda v: _ops.spmm(plan_t, op.values, op._cast(v))), op.dtype
        return matmul_closure.t().matmul, None
    if callable(matmul_closure):
        raise RuntimeError("gmres: transpose=True needs a tensor operator; a callable matmul_closure has no transpose "
                           "(pass a closure of Aᵀ with transpose=False instead)")
    raise RuntimeError("matmul_closure must be a tensor, or a callable object!")


def _preconditioner(precon, transpose: bool, dtype):
    """(block (n, p) -> M·block or None, whether it is a tensor: only then may the loop be captured)."""
    if precon is None:
        return None, True
    if torch.is_tensor(precon):
        m_op, _ = _operator(precon, transpose)
        return (lambda V: _block(m_op(V), dtype)), True
    solve = getattr(precon, "solve", None)
    if callable(solve):
        # one of the package's preconditioner objects: the whole block at once; for Aᵀ the right preconditioner is Mᵀ.  Their
        # application is not known to be only this package's launches, so such a loop stays eager.
        return (lambda V: _block(solve(V, transpose=transpose), dtype)), False
    return (lambda V: _block(precon(V), dtype)), False


def gmres(
    matmul_closure: Union[torch.Tensor, Callable[[torch.Tensor], torch.Tensor]],
    rhs: torch.Tensor,
    initial_guess: Optional[torch.Tensor] = None,
    settings: GMRESSettings = GMRESSettings(),
) -> torch.Tensor:
    r"""Solve :math:`A x = b` (:math:`A^T x = b` with ``settings.transpose``) with restarted, right-preconditioned GMRES.

    ``matmul_closure``: tensor (dense or sparse COO/CSR) or callable; ``rhs``: ``(n,)`` or ``(n, k)``.  ``settings.precon``: a
    tensor, one of the package's preconditioner objects (anything with ``solve(R, transpose=...)``: ``sparse_ilu0``,
    ``sparse_fsai``, ``sparse_amg`` ...) or a callable on ``(n, p)`` blocks; ``flexible`` stores the preconditioned basis, for a
    preconditioner that changes between applications.  Returns the solution with the shape of ``rhs``; every column's true
    residual is at most ``max(abstol, reltol·‖b − A x₀‖)`` unless ``maxiter`` inner steps ran out first
    (``last_solve_info("gmres")``: ``finished`` is False when a column was cut off at ``maxiter`` above its threshold).
    ``settings.logger`` receives the residual norms of every cycle start on the torch-op path only: the fused path reads nothing
    but its stop word.

    For gradients through a nonsymmetric ``A`` pass the pair ``sparse_generic_solve(A, B, solve=gmres, transpose_solve=gmres_t)``."""
    if settings.precon is not None and not (torch.is_tensor(settings.precon) or callable(settings.precon)
                                            or callable(getattr(settings.precon, "solve", None))):
        raise RuntimeError("settings.precon must be a tensor, or a callable object!")
    if int(settings.restart) < 1:
        raise RuntimeError(f"settings.restart must be at least 1, got {settings.restart}")
    if rhs.dim() not in (1, 2):
        raise RuntimeError(f"rhs must be (n,) or (n, k), got {tuple(rhs.shape)}")
    is_vector = rhs.dim() == 1
    B = rhs.unsqueeze(-1) if is_vector else rhs
    X0 = None if initial_guess is None else (initial_guess.unsqueeze(-1) if initial_guess.dim() == 1 else initial_guess)
    n, k = B.shape
    m = min(int(settings.restart), max(n, 1))
    fused = (ENABLE_FUSED and B.is_cuda and B.dtype in (torch.float32, torch.float64) and k > 0 and n > 0
             and m <= _be.gmres_geometry(B.dtype, n, 1)[0])
    op, sparse_dtype = _operator(matmul_closure, settings.transpose)
    precon, tensor_precon = _preconditioner(settings.precon, settings.transpose, B.dtype)
    maxiter = min(2 * n if settings.maxiter is None else int(settings.maxiter), 2**31 - 1)
    infos, sols = [], []
    slab = _be.KRYLOV_SLAB if fused else max(k, 1)
    for c0 in range(0, max(k, 1), slab):
        cols = slice(c0, min(c0 + slab, k))
        Bs = _block(B[:, cols], B.dtype)
        xs = None if X0 is None else X0[:, cols]
        if fused:
            x, info = _gmres_fused(op, sparse_dtype, Bs, xs, precon, tensor_precon, m, maxiter, settings)
        else:
            x, info = _gmres_torch(op, Bs, xs, precon, m, maxiter, settings)
        sols.append(x)
        infos.append(info)
    X = sols[0] if len(sols) == 1 else torch.cat(sols, dim=1)
    record_solve(solver="gmres", fused=fused, restart=m, cycles=max(i["cycles"] for i in infos),
                 iterations_enqueued=max(i["iterations_enqueued"] for i in infos),
                 iterations=torch.cat([i["iterations"] for i in infos]),
                 finished=all(i["finished"] for i in infos))
    return X.squeeze(-1) if is_vector else X


def gmres_t(matmul_closure, rhs, initial_guess=None, settings: GMRESSettings = GMRESSettings()) -> torch.Tensor:
    r"""``gmres`` with ``settings.transpose`` flipped: :math:`A^T x = b` by default — the ``transpose_solve`` that goes with
    ``solve=gmres`` in ``sparse_generic_solve``."""
    return gmres(matmul_closure, rhs, initial_guess, settings._replace(transpose=not settings.transpose))


def _gmres_fused(op, sparse_dtype, B, X0, precon, tensor_precon, m, maxiter, settings: GMRESSettings):
    """One slab of columns on the kernels of csrc/gmres.hip."""
    n, p = B.shape
    dev, dtype = B.device, B.dtype
    vt = _be.vtype_of(B)
    _, _, _, nb = _be.gmres_geometry(dtype, n, p)
    rows = _be.gmres_state_rows(m)
    flexible = bool(settings.flexible) and precon is not None
    abstol, reltol = float(settings.abstol), float(settings.reltol)

    x = torch.zeros_like(B) if X0 is None else X0.to(dtype).clone().contiguous()
    slab = -(-n * p // 4) * 4                                           # every basis block starts on a 16-byte boundary
    Vs = torch.zeros((m + 1, slab), dtype=dtype, device=dev)         # the basis: allocated once per call, outside the chunk
    Zs = torch.zeros((m, slab), dtype=dtype, device=dev) if flexible else None
    V = [Vs[i, :n * p].view(n, p) for i in range(m + 1)]
    Z = [Zs[i, :n * p].view(n, p) for i in range(m)] if flexible else None
    scal = torch.zeros((rows["rows"], p), dtype=dtype, device=dev)
    flags = torch.zeros(_be.GMRES_FLAG_WORDS + 4 * p, dtype=torch.int32, device=dev)
    part = torch.empty((nb, m + 1, p), dtype=dtype, device=dev)
    fold = torch.empty((_be.load_library().tsgu_cg_fold_rows(), m + 1, p), dtype=dtype, device=dev)
    ones = torch.ones((1, p), dtype=dtype, device=dev)
    r = torch.empty_like(B)
    u = torch.empty_like(B) if (precon is not None and not flexible) else None
    hnorm, coef, y = scal[rows["hnorm"]], scal[rows["coef"]:], scal[rows["y"]:]

    def scalar(phase, j, partial):
        _be.launch("tsgu_gmres_scalar", dev, vt, phase, j, m, partial, nb, fold, scal, flags, abstol, reltol, maxiter, p)

    def start():
        ax = _block(op(x), dtype)
        _be.launch("tsgu_gmres_subtract", dev, vt, n, p, 1, B, ax, slab, ones, r, part, flags, 0)      # r = b − A x, ‖r‖² partials
        scalar(0, 0, part)
        _be.launch("tsgu_gmres_scale", dev, vt, n, p, r, hnorm, V[0], flags, 0)                  # V₀ = r / β

    def step(j):
        k = j + 1
        z = V[j] if precon is None else precon(V[j])
        if flexible:
            Z[j].copy_(z)
        w = _block(op(z), dtype)
        for phase in (1, 2):                                                                     # CGS2
            _be.launch("tsgu_gmres_project", dev, vt, n, p, k, w, Vs, slab, part, flags, 1)
            scalar(phase, j, part)
            _be.launch("tsgu_gmres_subtract", dev, vt, n, p, k, w, Vs, slab, coef, w, part, flags, 1)
        scalar(3, j, part)                                                                       # rotations, g, estimate, stop rules
        _be.launch("tsgu_gmres_scale", dev, vt, n, p, w, hnorm, V[j + 1], flags, 1)

    def finish_cycle():
        scalar(4, 0, None)
        if precon is None or flexible:
            _be.launch("tsgu_gmres_update", dev, vt, n, p, m, x, Vs if Zs is None else Zs, slab, y, flags)
        else:
            u.zero_()
            _be.launch("tsgu_gmres_update", dev, vt, n, p, m, u, Vs, slab, y, flags)
            _be.launch("tsgu_gmres_update", dev, vt, n, p, 1, x, precon(u), slab, ones, flags)          # x += M (V y), frozen columns kept

    def body(j):
        step(j)
        if j == m - 1:
            finish_cycle()
            start()

    def finished():
        return bool(flags[0].item())

    with torch.cuda.device(dev):
        start()
        queued = 0
        if not finished():
            queued, _ = _graph.run_chunked(body, finished, m, first=m, expected=maxiter,
                                           capturable=sparse_dtype == dtype and _graph.enabled() and tensor_precon)
        head = flags[:_be.GMRES_FLAG_WORDS].tolist()
        iters = flags[_be.GMRES_FLAG_WORDS + 3 * p:].to(torch.int64).cpu()
        met = bool((scal[rows["estimate"]] <= scal[rows["threshold"]]).all().item())      # the residual each column stopped on
    return x, {"cycles": head[2] - 1, "iterations_enqueued": queued, "iterations": iters, "finished": met}


def _gmres_torch(op, B, X0, precon, m, maxiter, settings: GMRESSettings):
    """The same algorithm as torch ops, columns in lock-step, on whatever device the operands live on."""
    n, p = B.shape
    dev, dtype = B.device, B.dtype
    log = settings.logger
    flexible = bool(settings.flexible) and precon is not None
    x = torch.zeros_like(B) if X0 is None else X0.to(dtype).clone()
    V = torch.zeros((m + 1, n, p), dtype=dtype, device=dev)
    Z = torch.zeros((m, n, p), dtype=dtype, device=dev) if flexible else None
    R = torch.zeros((m, m, p), dtype=dtype, device=dev)
    cs, sn = torch.zeros((m, p), dtype=dtype, device=dev), torch.zeros((m, p), dtype=dtype, device=dev)
    g = torch.zeros((m + 1, p), dtype=dtype, device=dev)
    iters = torch.zeros(p, dtype=torch.int64, device=dev)
    fin = torch.zeros(p, dtype=torch.bool, device=dev)
    thr, cycles, queued = None, 0, 0
    zero, one = torch.zeros((), dtype=dtype, device=dev), torch.ones((), dtype=dtype, device=dev)
    while True:
        r = B - checked(op(x), dtype)
        beta = torch.linalg.vector_norm(r, dim=0)
        if thr is None:
            thr = torch.clamp(settings.reltol * beta, min=settings.abstol)
        fin = fin | (beta <= thr) | (iters >= maxiter)
        if not log.disabled:
            log.info("cycle %d: residual %s" % (cycles, beta.tolist()))
        if bool(fin.all()):
            break
        cycles += 1
        ended = fin.clone()
        steps = torch.zeros(p, dtype=torch.int64, device=dev)
        V[0] = torch.where(ended, zero, r * (one / torch.where(ended, one, beta)))
        g[0] = torch.where(ended, g[0], beta)
        for j in range(m):
            queued += 1
            if bool(ended.all()):
                continue
            act = ~ended
            z = V[j] if precon is None else precon(V[j].contiguous())
            if flexible:
                Z[j] = z
            w = checked(op(z.contiguous()), dtype)
            Vk = V[:j + 1]
            h = torch.zeros((j + 1, p), dtype=dtype, device=dev)
            for _ in range(2):                                   # CGS2
                hk = (Vk * w).sum(dim=1)
                w = w - (Vk * hk.unsqueeze(1)).sum(dim=0)
                h = h + hk
            hn = torch.linalg.vector_norm(w, dim=0)
            for i in range(j):
                a, b = h[i].clone(), h[i + 1].clone()
                h[i] = cs[i] * a + sn[i] * b
                h[i + 1] = cs[i] * b - sn[i] * a
            den = torch.sqrt(h[j] * h[j] + hn * hn)
            safe = torch.where(den != 0, den, one)
            cj = torch.where(den != 0, h[j] / safe, one)
            sj = torch.where(den != 0, hn / safe, zero)
            h[j] = cj * h[j] + sj * hn
            R[:j + 1, j] = torch.where(act, h, R[:j + 1, j])
            cs[j] = torch.where(act, cj, cs[j])
            sn[j] = torch.where(act, sj, sn[j])
            gn = -(sj * g[j])
            g[j + 1] = torch.where(act, gn, g[j + 1])
            g[j] = torch.where(act, cj * g[j], g[j])
            steps = torch.where(act, torch.full_like(steps, j + 1), steps)
            iters = iters + act.to(iters.dtype)
            ended = ended | (act & ((gn.abs() <= thr) | (hn == 0) | (iters >= maxiter)))
            V[j + 1] = torch.where(ended, zero, w * (one / torch.where(ended, one, hn)))
        # cycle end: R y = g over the first steps_c unknowns
        y = torch.zeros((m, p), dtype=dtype, device=dev)
        for i in range(m - 1, -1, -1):
            s = g[i].clone()
            for l in range(i + 1, m):
                s = s - R[i, l] * y[l]
            d = R[i, i]
            yi = torch.where(d != 0, s / torch.where(d != 0, d, one), zero)
            y[i] = torch.where(i < steps, yi, zero)
        upd = ((V[:m] if Z is None else Z) * y.unsqueeze(1)).sum(dim=0)
        if precon is not None and not flexible:
            upd = precon(upd.contiguous())
        x = torch.where(steps > 0, x + upd, x)
    return x, {"cycles": cycles, "iterations_enqueued": queued, "iterations": iters.cpu(), "finished": bool((beta <= thr).all())}


def last_solve_info():
    """Diagnostics of this thread's most recent ``gmres`` call: ``iterations`` (inner steps per column), ``cycles``, ``restart``,
    ``fused``."""
    return LAST_SOLVE.info.get("gmres")
