"""LOBPCG (Knyazev 2001; the robust variant of scipy's ``lobpcg``) for the ``k`` smallest eigenpairs of a symmetric operator.

The recurrence is written once, over three primitives on tall-skinny row-major blocks:

``gram(Y, Z)``                      ``YᵀZ``
``combine(inputs, outputs, coefs)``  ``Out_t = beta_t·Out_t + Σ_i S_i·C_ti`` in one pass over the rows
``residual(AX, X, lam)``             ``R = AX − X·diag(lam)`` and the column sums of squares of ``R``

On GPU operands they are the kernels of ``csrc/lobpcg_impl.h`` (``_backend.tall_gram``, ``tall_combine``, ``lobpcg_residual``), on
CPU operands plain torch ops (``_cpu``): the operands' device selects the path, and nothing else does.

The basis ``S = [X, W, P]`` and its image ``A·S`` are two ``(n, 3k)`` allocations each (the iteration reads one pair and writes the
other: no output of ``combine`` is one of its inputs).  One iteration:

1. ``R = A·X − X·Λ`` and its column norms (``residual``);
2. ``W = M(R)`` (the preconditioner, under ``no_grad``);
3. ``W ← W − X·(XᵀW)``, twice (``gram`` + ``combine`` with ``beta = 1``);
4. Cholesky-QR of ``W``: ``gram``, ``torch.linalg.cholesky_ex`` of the k × k matrix on the device, the triangular solve folded
   into the coefficient matrix, ``combine``;
5. ``A·W``, one sparse product (``σ·A`` for ``σ = −1``: the sign is applied to the product);
6. the two Gram matrices ``SᵀS`` and ``Sᵀ(A·S)``, one ``gram`` launch each; ``P`` is NOT normalised by a pass of its own: the
   Rayleigh–Ritz step scales the Gram matrices by ``diag(SᵀS)^-1/2`` and folds the scaling into its coefficients, which updates
   ``P`` and ``A·P`` implicitly with the same coefficients;
7. ONE device→host read: the column sums of squares of step 1, the ``cholesky_ex`` info of step 4 and the two Gram matrices,
   packed into one array.  The convergence test, the Rayleigh–Ritz problem (at most 96 × 96: Cholesky of the scaled ``SᵀS``,
   triangular solves, ``eigh``, all in float64 on the host — ``torch.linalg.eigh`` on the device reads its own error word back,
   which would be a second read per iteration) and the restart decision are made from it.  SOFT LOCKING happens here too: a
   converged column keeps its ``X`` and ``W`` in the problem but not its ``P`` (its residual has stopped moving, so its next
   ``W`` and its ``P`` are the same rounding noise, which makes the basis singular), by selecting rows and columns of the Gram
   matrices — the passes over the rows keep their fixed shapes;
8. ``X' = S·C``, ``A·X' = (A·S)·C``, ``P' = [W, P]·C_wp`` and ``A·P' = [A·W, A·P]·C_wp`` in ONE ``combine`` launch that reads six
   blocks and writes four; the coefficients and the new ``Λ`` go up in one asynchronous copy.

Breakdowns never raise.  A scaled ``SᵀS`` whose Cholesky factorisation fails (or has a pivot below ``32·sqrt(u)``: a direction
within half a degree of the others) restarts the iteration without ``P`` — from the Gram matrices already read, so a restart costs
no pass and no read — and is counted.  A ``W`` whose Gram matrix is not positive definite ends the loop with the current pairs
and ``breakdown = True``.  An initial block without full rank is perturbed (a fixed seed) and counted under ``perturbations``.

Column ``j`` has converged when ``‖A·x_j − λ_j·x_j‖₂ <= tol·‖A‖_est`` with ``‖A‖_est = ‖A·X₀‖_F / ‖X₀‖_F`` of the orthonormalised
initial block (``torch/_lobpcg.py``'s ``A_norm``); the loop stops when all columns have, or at ``niter``.
"""

from __future__ import annotations

import math

import torch

from .. import _backend as _be
from ._operator import LAST_SOLVE, as_operator, checked, record_solve


# a pivot of the scaled Cholesky factor below PIVOT_FLOOR·sqrt(u) counts as a breakdown
PIVOT_FLOOR = 32.0


def _primitives(device: torch.device):
    if device.type == "cuda":
        return _be.tall_gram, _be.tall_combine, _be.lobpcg_residual
    from .. import _cpu

    return _cpu.tall_gram, _cpu.tall_combine, _cpu.lobpcg_residual


class _Uplink:
    """Small host arrays to the operands' device: through one pinned buffer and an asynchronous copy on a GPU (the buffer is
    rewritten only after the next device→host read, which orders it behind the copy)."""

    def __init__(self, numel: int, dtype: torch.dtype, device: torch.device):
        self.device, self.dtype = device, dtype
        self.pinned = torch.empty(numel, dtype=dtype, pin_memory=True) if device.type == "cuda" else None

    def __call__(self, *arrays):
        flat = torch.cat([a.reshape(-1) for a in arrays]).to(self.dtype)
        if self.pinned is None:
            dev = flat
        else:
            self.pinned[: flat.numel()].copy_(flat)
            dev = torch.empty(flat.numel(), dtype=self.dtype, device=self.device)
            dev.copy_(self.pinned[: flat.numel()], non_blocking=True)
        out, at = [], 0
        for a in arrays:
            out.append(dev[at:at + a.numel()].view(a.shape))
            at += a.numel()
        return out


def _scaled_cholesky(G: torch.Tensor, floor: float):
    """(s, L⁻¹) with L·Lᵀ = diag(s)·G·diag(s), s = diag(G)^-1/2, for a float64 host matrix; None when G is not (safely) positive
    definite: a non-finite entry, a diagonal that is not positive, a failed factorisation or a pivot below `floor`."""
    d = G.diagonal()
    if not bool(torch.isfinite(G).all()) or not bool((d > 0).all()):
        return None
    s = d.rsqrt()
    Gs = G * s[:, None] * s[None, :]
    L, info = torch.linalg.cholesky_ex((Gs + Gs.t()) * 0.5)
    if int(info) != 0 or not bool(torch.isfinite(L).all()) or float(L.diagonal().min()) < floor:
        return None
    return s, torch.linalg.solve_triangular(L, torch.eye(G.size(0), dtype=G.dtype), upper=False)


def _rayleigh_ritz(GS: torch.Tensor, GA: torch.Tensor, k: int, floor: float):
    """The k smallest Ritz pairs of the pencil (GA, GS) (float64, host): (values (k,), C (m, k)) with Cᵀ·GS·C = I, or None."""
    got = _scaled_cholesky(GS, floor)
    if got is None or not bool(torch.isfinite(GA).all()):
        return None
    s, Li = got
    GAs = GA * s[:, None] * s[None, :]
    M = Li @ ((GAs + GAs.t()) * 0.5) @ Li.t()
    try:
        w, Z = torch.linalg.eigh((M + M.t()) * 0.5)
    except RuntimeError:        # (LAPACK did not converge: a breakdown like any other)
        return None
    return w[:k], s[:, None] * (Li.t() @ Z[:, :k])


def lobpcg(matmul_closure, X: torch.Tensor, *, sign: float = 1.0, preconditioner=None, niter: int = 500, tol=None):
    """The ``k`` smallest eigenpairs of ``sign·A`` (``sign = ±1``) for the symmetric operator ``matmul_closure`` (a sparse tensor or
    a callable on ``(n, k)`` blocks, as the Krylov loops take) from the initial block ``X`` ``(n, k)``, ``3k <= n``,
    ``k <= _backend.tall_geometry(dtype)[0]`` on a GPU.  ``preconditioner``: ``None``, a callable on an ``(n, k)`` block or a dense
    tensor (applied with ``@``); it approximates ``(sign·A)⁻¹`` and should be symmetric positive definite.  Returns
    ``(values (k,) ascending, vectors (n, k))`` of ``sign·A``.  Runs under ``no_grad``; never raises on a breakdown:
    ``last_solve_info()`` tells how the loop ended.  One device→host read per iteration, plus four around the loop."""
    with torch.no_grad():
        return _lobpcg(as_operator(matmul_closure), X.detach(), float(sign), preconditioner, int(niter), tol)


def _lobpcg(op, X0, sign, preconditioner, niter, tol):
    n, k = X0.shape
    dtype, dev = X0.dtype, X0.device
    gram, combine, residual = _primitives(dev)
    u = torch.finfo(dtype).eps
    tol = math.sqrt(u) if tol is None else float(tol)
    floor = PIVOT_FLOOR * math.sqrt(u)
    up = _Uplink(3 * k * k + k, dtype, dev)

    def product(V, out):
        """out = sign·A·V: the sign rides on the pass that moves the product into its block of A·S."""
        AV = checked(op(V.contiguous()), dtype)
        return out.copy_(AV) if sign == 1.0 else torch.mul(AV, sign, out=out)

    if preconditioner is None:
        precondition = None
    elif torch.is_tensor(preconditioner):
        precondition = lambda R: preconditioner @ R                    # noqa: E731
    else:
        precondition = preconditioner

    S = [torch.zeros((n, 3 * k), dtype=dtype, device=dev) for _ in range(2)]
    AS = [torch.zeros((n, 3 * k), dtype=dtype, device=dev) for _ in range(2)]
    Rbuf = torch.empty((n, k), dtype=dtype, device=dev)
    block = lambda T, j: T[:, j * k:(j + 1) * k]                       # noqa: E731
    restarts = perturbations = 0

    # the initial block, orthonormalised by Cholesky-QR; one without full rank is perturbed (a fixed seed) until it has
    X0 = X0.contiguous().clone()
    for attempt in range(4):
        got = _scaled_cholesky(gram(X0, X0).double().cpu(), floor)
        if got is not None:
            break
        perturbations += 1
        noise = torch.randn((n, k), dtype=torch.float64, generator=torch.Generator().manual_seed(attempt)).to(dtype=dtype, device=dev)
        rms = X0.square().mean().sqrt()
        X0 = X0 + noise * torch.where(torch.isfinite(rms) & (rms > 0), rms, torch.ones_like(rms)) * 0.25
        X0 = torch.nan_to_num(X0, nan=0.0, posinf=0.0, neginf=0.0)
    info = dict(solver="lobpcg", iterations=0, converged=False, converged_columns=[False] * k, residual_norms=[math.inf] * k,
                restarts=restarts, perturbations=perturbations, breakdown=got is None, tolerance=tol, a_norm=math.nan)
    if got is None:
        record_solve(**info)
        return torch.full((k,), math.nan, dtype=dtype, device=dev), X0
    s, Li = got
    (Rinv,) = up(s[:, None] * Li.t())
    combine([X0], [block(S[0], 0)], [[Rinv]])
    product(block(S[0], 0), block(AS[0], 0))
    # ‖A‖_est and the first Rayleigh–Ritz rotation, from one read
    X, AX = block(S[0], 0), block(AS[0], 0)
    first = torch.cat([gram(X, AX).double().reshape(-1), gram(AX, AX).double().diagonal()]).cpu()
    a_norm = math.sqrt(max(float(first[k * k:].sum()), 0.0) / k)
    info["a_norm"] = a_norm
    GA = first[: k * k].view(k, k)
    got = _rayleigh_ritz(torch.eye(k, dtype=torch.float64), GA, k, floor) if bool(torch.isfinite(GA).all()) else None
    if got is None:
        info["breakdown"] = True
        record_solve(**info)
        return torch.full((k,), math.nan, dtype=dtype, device=dev), X.clone()
    lam_host, C = got
    C_dev, lam = up(C, lam_host)
    combine([block(S[0], 0), block(AS[0], 0)], [block(S[1], 0), block(AS[1], 0)], [[C_dev, None], [None, C_dev]])
    cur, have_p = 1, False
    threshold = tol * a_norm
    eye = torch.eye(k, dtype=dtype, device=dev)

    it = 0
    while True:
        Sc, ASc = S[cur], AS[cur]
        X, AX = block(Sc, 0), block(ASc, 0)
        R, sumsq = residual(AX, X, lam, out=Rbuf)
        if it >= niter:
            # (the budget is spent: the norms of the pairs that are handed out, one read)
            norms = sumsq.double().cpu().clamp_min(0).sqrt()
            info.update(residual_norms=norms.tolist(), converged_columns=(norms <= threshold).tolist())
            info["converged"] = all(info["converged_columns"])
            break
        W = R
        if precondition is not None:
            W = precondition(R)
            if not torch.is_tensor(W) or W.shape != R.shape or W.dtype != dtype or W.device != dev:
                raise RuntimeError(f"lobpcg: the preconditioner must map a ({n}, {k}) block of {dtype} on {dev} to one")
            W = W.detach()
            W = W.contiguous() if W.data_ptr() != R.data_ptr() else W
        for _ in range(2):
            combine([X], [W], [[-gram(X, W)]], betas=[1.0])
        GW = gram(W, W)
        d = GW.diagonal().clamp_min(torch.finfo(dtype).tiny).rsqrt()
        L, info_w = torch.linalg.cholesky_ex(GW * d[:, None] * d[None, :])
        Rinv = d[:, None] * torch.linalg.solve_triangular(L.mT, eye, upper=True)
        ok = (info_w == 0) & torch.isfinite(Rinv).all()
        Rinv = torch.where(ok, Rinv, eye).contiguous()
        combine([W], [block(Sc, 1)], [[Rinv]])
        product(block(Sc, 1), block(ASc, 1))
        m = 3 * k if have_p else 2 * k
        GS, GA = gram(Sc[:, :m], Sc[:, :m]), gram(Sc[:, :m], ASc[:, :m])
        # the one device→host read of the iteration
        host = torch.cat([sumsq.double(), (~ok).double().reshape(1), GS.double().reshape(-1), GA.double().reshape(-1)]).cpu()
        norms = host[:k].clamp_min(0).sqrt()
        done = norms <= threshold
        info.update(iterations=it, residual_norms=norms.tolist(), converged_columns=done.tolist(), restarts=restarts)
        if bool(done.all()):
            info["converged"] = True
            break
        if host[k] != 0 or not bool(torch.isfinite(norms).all()):
            info["breakdown"] = True
            break
        GS, GA = host[k + 1:k + 1 + m * m].view(m, m), host[k + 1 + m * m:].view(m, m)
        # soft locking: a converged column keeps its X and W, but not its P (its residual has stopped moving, so its next W and its
        # P are the same rounding noise: a singular basis)
        sel = list(range(2 * k)) + [2 * k + j for j in range(k) if have_p and not bool(done[j])]
        got = _rayleigh_ritz(GS[sel][:, sel], GA[sel][:, sel], k, floor)
        if got is None and len(sel) > 2 * k:
            restarts += 1
            info["restarts"] = restarts
            sel = sel[: 2 * k]
            got = _rayleigh_ritz(GS[sel][:, sel], GA[sel][:, sel], k, floor)
        if got is None:
            info["breakdown"] = True
            break
        lam_host, C = got
        C = torch.zeros((m, k), dtype=torch.float64).index_copy_(0, torch.tensor(sel), C)
        C_dev, lam = up(C, lam_host)
        Cb = [C_dev[j * k:(j + 1) * k] for j in range(m // k)]
        nb = len(Cb)
        ins = [block(Sc, j) for j in range(nb)] + [block(ASc, j) for j in range(nb)]
        none = [None] * nb
        Sn, ASn = S[1 - cur], AS[1 - cur]
        combine(ins, [block(Sn, 0), block(ASn, 0), block(Sn, 2), block(ASn, 2)],
                [Cb + none, none + Cb, [None] + Cb[1:] + none, none + [None] + Cb[1:]])
        cur, have_p = 1 - cur, True
        it += 1
        info["iterations"] = it
    record_solve(**info)
    return lam.clone(), block(S[cur], 0).clone()


def last_solve_info():
    """Diagnostics of this thread's most recent ``lobpcg`` call: ``iterations``, ``converged`` (all columns), ``converged_columns``,
    ``residual_norms`` (``‖A·x_j − λ_j·x_j‖₂`` of the returned pairs), ``restarts`` (iterations redone without ``P``),
    ``perturbations`` (of an initial block without full rank), ``breakdown`` (the loop ended on a ``W`` or a basis that could not be
    orthonormalised), ``tolerance`` and ``a_norm`` (``‖A‖_est``)."""
    return LAST_SOLVE.info.get("lobpcg")
