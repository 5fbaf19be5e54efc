"""``sparse_expm_mm`` — ``exp(t·A)·B`` for a sparse symmetric matrix by a Chebyshev expansion, with gradients that stay on the
matrix's pattern.

For a spectrum inside ``[lo, hi]`` let ``ρ = (hi − lo)/2``, ``mid = (hi + lo)/2``, ``Â = a·A + b·I`` with ``a = 1/ρ``, ``b = −mid/ρ`` and
``z = t·ρ``.  Then

    exp(t·A)·B = Σ_{k=0..K} c_k·w_k,     w_0 = B,  w_1 = Â·w_0,  w_{k+1} = 2·Â·w_k − w_{k−1}
    c_k = e^{t·mid + |z|}·(2 − δ_{k0})·sign(z)^k·ive_k(|z|)

with ``ive_k(x) = I_k(x)·e^{−x}`` the scaled modified Bessel functions (``_ive``: Miller's backward recurrence in float64, normalised by
``ive_0 + 2·Σ_{k≥1} ive_k = 1``).  ``K`` is the smallest index with ``2·Σ_{k>K} ive_k(|z|) ≤ tolerance``, so that before rounding
``‖Y − exp(tA)·b‖₂ ≤ tolerance·e^{max(t·lo, t·hi)}·‖b‖₂`` for every column; it grows like ``√(2·|z|·ln(1/tolerance))`` and is known before
the first launch: the loop has no inner products, no stopping test and no host read.

What it is for.  Heat-kernel diffusion ``exp(−t·L)·X`` on meshes and graphs with a learned time per channel (``t`` of shape ``(1, p)``),
heat-kernel signatures at several scales (``t`` of shape ``(T,)``: the ``w_k`` are shared, every further time costs ``2/m`` planes per step)
and exponential integrators for stencil operators.

On the GPU one step is the product ``A·w_k`` by the best kernel family of the pattern (``SparseOperator.matmul``) followed by
``tsgu_cheb_step`` (``csrc/expm_impl.h``), which writes ``w_{k+1}`` over ``w_{k−1}`` and into a slot of a chunk ``[n][m][p]``; once per
chunk ``tsgu_cheb_combine`` adds the chunk's ``m`` terms to the ``T`` results.  CPU operands take the torch-op path
(``_cpu.expm_apply``: the same recurrence with ``A @ w`` and elementwise ops, the same coefficient table).

Gradients, exact for the approximant.  With ``G = ∂L/∂Y``, ``f_0 = 1``, ``f_k = 2``: ``μ_k = c_k·G + f_k·Â·μ_{k+1} − μ_{k+2}`` downwards from
``μ_{K+1} = μ_{K+2} = 0``; ``grad_B = μ_0`` and ``grad_A[i,j] = a·Σ_{k<K} f_k Σ_c μ_{k+1}[i,c]·w_k[j,c]`` at ``A``'s stored entries, unsymmetrised
— one SDDMM per chunk on ``A``'s own index tensors, as ``sparse_inv_sqrt_mm`` does with its solution blocks.  ``grad_t = ⟨G, A·Y⟩`` per
time (and column) is the true derivative.  The bounds and the coefficients are constants of the call.

Out of scope: non-symmetric ``A``, bfloat16, batched ``A``, double backward, regenerating ``w_k`` by the reversed recurrence.
"""

from __future__ import annotations

import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _ops
from .sparse_matmul import _Operand
from .sparse_sqrt import _check_operands
from .utils._operator import SparseOperator, record_solve

__all__ = ["sparse_expm_mm", "SparseExpmMM"]

_MAX_TIMES = 8         # time planes of one tsgu_cheb_combine launch (csrc/expm_impl.h: kChebTimeCap)
_SDDMM_WIDTH = 1024    # columns of one SDDMM call of the backward (sparse_sqrt's): a chunk holds at most this many
_EXACT_BELOW = 1e6     # |t|·ρ up to which K is always computed exactly; above it a K that is clearly beyond max_terms is refused on
                       # the estimate √(2·|z|·ln(1/tolerance)), without running a host recurrence of |z| steps


# ---- the coefficients --------------------------------------------------------------------------------------------------------------

def _ive_many(xs, tolerance: float):
    """(table, K) for the 1-D array ``xs`` ≥ 0: table[k][u] = ive_k(xs[u]) for k = 0 ... M as float64 and K[u] the smallest index with
    2·Σ_{k>K} ive_k(xs[u]) ≤ tolerance.  Miller's backward recurrence f_{k−1} = f_{k+1} + (2k/x)·f_k from one start index M beyond
    the largest x, normalised by ive_0 + 2·Σ_{k≥1} ive_k = 1, for all arguments at once: M numpy steps on vectors, whatever the
    number of distinct times (a learned time per channel has p of them)."""
    xs = np.asarray(xs, dtype=np.float64).reshape(-1)
    xmax = float(xs.max())
    if xmax == 0.0:
        return np.ones((1, xs.size)), np.zeros(xs.size, dtype=np.int64)
    M = int(xmax + 20.0 * max(1.0, xmax) ** (1.0 / 3.0) + 60.0)
    pos = xs > 0
    two_over_x = np.where(pos, 2.0 / np.where(pos, xs, 1.0), 0.0)
    f = np.zeros((M + 2, xs.size))
    f[M, pos] = 1e-300
    for k in range(M, 0, -1):
        nxt = f[k + 1] + (k * two_over_x) * f[k]
        big = nxt > 1e250
        if big.any():                                             # rescale what exists: the tail only loses what is below 1e-250
            f[k:, big] *= 1e-250
            nxt[big] *= 1e-250
        f[k - 1] = nxt
    f = f[: M + 1]
    f[0, ~pos] = 1.0                                              # ive_k(0) = δ_{k0}
    f /= f[0] + 2.0 * f[1:].sum(axis=0)
    tail = 2.0 * np.cumsum(f[::-1], axis=0)[::-1]                 # tail[k] = 2·Σ_{j≥k} ive_j
    ok = tail <= tolerance
    K = np.where(ok.any(axis=0), np.maximum(np.argmax(ok, axis=0) - 1, 0), M)
    return f, K


def _ive(x: float, tolerance: float):
    """(ive_0 ... ive_M of one x ≥ 0, K): the same recurrence on Python floats, ten times faster than a numpy step per k for one
    argument (0.1 ms against 2 ms at x = 100)."""
    x = float(x)
    if x == 0.0:
        return np.ones(1), 0
    M = int(x + 20.0 * max(1.0, x) ** (1.0 / 3.0) + 60.0)
    f = [0.0] * (M + 2)
    f[M] = 1e-300
    hi, cur, two_over_x = 0.0, 1e-300, 2.0 / x
    for k in range(M, 0, -1):
        nxt = hi + k * two_over_x * cur
        if nxt > 1e250:
            for j in range(k, M + 1):
                f[j] *= 1e-250
            nxt, cur = nxt * 1e-250, cur * 1e-250
        f[k - 1] = nxt
        hi, cur = cur, nxt
    f = np.asarray(f[: M + 1])
    f /= f[0] + 2.0 * f[1:].sum()
    tail = 2.0 * np.cumsum(f[::-1])[::-1]
    ok = tail <= tolerance
    K = max(int(np.argmax(ok)) - 1, 0) if ok.any() else M
    return f, K


_VECTOR_FROM = 48      # distinct |t|·ρ from which one vectorised recurrence beats a scalar recurrence each (0.04 ms each against 1.9 ms at |z| = 100)


def _ive_table(xs, tolerance: float):
    """(table [k][u], K[u]) for the distinct arguments ``xs``: scalar recurrences for a few, the vectorised one for many."""
    if len(xs) >= _VECTOR_FROM:
        return _ive_many(xs, tolerance)
    each = [_ive(x, tolerance) for x in xs]
    table = np.zeros((max(f.size for f, _ in each), len(each)))
    for u, (f, _) in enumerate(each):
        table[: f.size, u] = f
    return table, np.array([k for _, k in each], dtype=np.int64)


def _terms_estimate(z: float, tolerance: float) -> float:
    """√(2·|z|·ln(1/tolerance)): what K grows like (an over-estimate by a few per cent for |z| ≥ 10)."""
    return math.sqrt(2.0 * abs(z) * max(1.0, math.log(1.0 / min(tolerance, 0.5))))


def _coefficients(who: str, t: np.ndarray, lo: float, hi: float, tolerance: float, max_terms: int):
    """(c, a, b, K): the float64 table c[k][...] = c_k of every time of the array ``t`` (c has shape (K + 1, *t.shape)), the affine map
    Â = a·A + b·I and the common K (the largest any time needs).  A degenerate interval gives K = 0, c_0 = e^{t·lo}, a = b = 0."""
    t = np.asarray(t, dtype=np.float64)
    rho, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    if rho == 0.0:
        return np.exp(t * lo)[None], 0.0, 0.0, 0
    z = t * rho
    zmax = float(np.abs(z).max()) if z.size else 0.0
    if zmax > _EXACT_BELOW and 0.5 * _terms_estimate(zmax, tolerance) > max_terms:   # (the recurrence below takes |z| host steps)
        raise ValueError(f"{who}: |t|·ρ = {zmax:.6g} needs about K = {int(_terms_estimate(zmax, tolerance))} terms at tolerance "
                         f"{tolerance:g}, above max_terms = {max_terms}")
    uniq, inverse = np.unique(np.abs(z).reshape(-1), return_inverse=True)
    table, needed = _ive_table(uniq, tolerance)
    K = int(needed.max())
    if K > max_terms:
        raise ValueError(f"{who}: |t|·ρ = {zmax:.6g} needs K = {K} terms at tolerance {tolerance:g}, above max_terms = {max_terms}")
    ive = np.zeros((K + 1, uniq.size))
    m = min(K + 1, table.shape[0])
    ive[:m] = table[:m]
    c = ive[:, inverse.reshape(-1)].reshape((K + 1,) + z.shape)
    c[1:] *= 2.0
    sign = np.where(z < 0, -1.0, 1.0)
    c[1::2] *= sign
    c *= np.exp(t * mid + np.abs(z))
    return np.ascontiguousarray(c), 1.0 / rho, -mid / rho, K


# ---- checks ------------------------------------------------------------------------------------------------------------------------

def _check(who: str, A, B, t, bounds, tolerance, max_terms):
    _check_operands(who, A, B)
    p = 1 if B.dim() == 1 else B.size(1)
    if isinstance(t, torch.Tensor):
        if t.layout != torch.strided or not t.dtype.is_floating_point:
            raise ValueError(f"{who}: t must be a float or a dense floating-point tensor")
        if t.dim() > 2 or (t.dim() >= 1 and t.size(0) < 1) or (t.dim() == 2 and t.size(1) != p):
            raise ValueError(f"{who}: t must be a scalar, have shape (T,) or (T, {p}), got {tuple(t.shape)}")
        if t.dim() >= 1 and t.size(0) > _MAX_TIMES:
            raise ValueError(f"{who}: at most {_MAX_TIMES} times per call, got {t.size(0)}")
    else:
        try:
            t = float(t)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: t must be a float or a dense floating-point tensor") from None
    if int(max_terms) < 0:
        raise ValueError(f"{who}: max_terms must not be negative, got {max_terms}")
    if not float(tolerance) > 0.0:
        raise ValueError(f"{who}: tolerance must be positive, got {tolerance}")
    if bounds is not None:
        try:
            lo, hi = (float(b) for b in bounds)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: bounds must be a pair (lo, hi) of floats or None, got {bounds!r}") from None
        if not (lo <= hi and math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"{who}: bounds must satisfy lo <= hi and be finite, got ({lo}, {hi})")


def _gershgorin(A: torch.Tensor):
    """(min_i a_ii − r_i, max_i a_ii + r_i) with r_i = Σ_{j≠i} |a_ij|: |A|·1 by the package's product, the diagonal from the stored
    entries, one host read."""
    op = _Operand(A)
    n = A.size(0)
    vals = op.values
    total = _ops.spmm(op.plan, vals.abs(), torch.ones((n, 1), dtype=vals.dtype, device=vals.device)).reshape(n)
    if A.layout == torch.sparse_csr:
        crow = A.crow_indices()
        rows = torch.repeat_interleave(torch.arange(n, device=crow.device), (crow[1:] - crow[:-1]).to(torch.int64), output_size=vals.numel())
        cols = A.col_indices()
    else:
        rows, cols = op.indices[0], op.indices[1]
    on_diag = torch.where(rows == cols, vals, torch.zeros_like(vals))
    diag = torch.zeros(n, dtype=vals.dtype, device=vals.device).index_add_(0, rows.to(torch.int64), on_diag)
    r = total - diag.abs()                                       # (coalesced COO and CSR store a diagonal entry once)
    ends = torch.stack(((diag - r).min(), (diag + r).max())).to("cpu", torch.float64)
    lo, hi = float(ends[0]), float(ends[1])
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"sparse_expm_mm: A has non-finite entries (Gershgorin interval ({lo}, {hi}))")
    return lo, max(lo, hi)


# ---- the fused loops ---------------------------------------------------------------------------------------------------------------

def _chunk_length(dtype, n: int, p: int, K: int, chunk=None) -> int:
    cap = _be.expm_geometry(dtype, n, p)[1]
    if chunk is not None:
        if not 1 <= int(chunk) <= cap:
            raise ValueError(f"sparse_expm_mm: chunk must lie in [1, {cap}], got {chunk}")
        return int(chunk)
    return max(1, min(K + 1, cap, _SDDMM_WIDTH // p))


def _aligned(x: torch.Tensor) -> torch.Tensor:
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _planes(n: int, p: int, T: int, dtype, device, align: int, source=None):
    """(buffer (T, plane), plane): T planes of n·p values on 16-byte boundaries; `source` (T, n, p) is copied in (or used as it is
    when its planes already lie so)."""
    plane = -(-n * p // align) * align
    if source is not None and plane == n * p and source.is_contiguous() and source.data_ptr() % 16 == 0:
        return source.view(T, plane), plane
    buf = torch.zeros((T, plane), dtype=dtype, device=device)
    if source is not None:
        buf[:, : n * p] = source.reshape(T, n * p)
    return buf, plane


def _expm_fused(op: SparseOperator, B: torch.Tensor, coef: torch.Tensor, a: float, b: float, want_keep: bool, chunk=None):
    """Σ_k coef[k] ∘ w_k for the (n, p) block ``B`` on the HIP kernels; ``coef`` (K + 1, T, p) in B's dtype on B's device.  Returns
    (Y (T, n, p), the chunks of w_k as a list of contiguous (n, m_q, p) buffers or None, m).  ``chunk``: the chunk length instead of
    the rule's (tests and tools/expmbench.py)."""
    n, p = B.shape
    K, T = coef.size(0) - 1, coef.size(1)
    dev, dtype = B.device, B.dtype
    tcap, _, align, _, _ = _be.expm_geometry(dtype, n, p)
    if T > tcap:
        raise RuntimeError(f"tsgu_cheb_combine takes at most {tcap} times, got {T}")
    m = _chunk_length(dtype, n, p, K, chunk)
    B = _aligned(B)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)        # the kernels' stop word: never set, this loop has no stopping test
    ring = [torch.zeros_like(B), torch.zeros_like(B)]
    Y, plane = _planes(n, p, T, dtype, dev, align)
    n_chunks = -(-(K + 1) // m)
    flat = None if want_keep else torch.empty(n * m * p, dtype=dtype, device=dev)
    kept = [] if want_keep else None

    def buffer(q):
        mq = min(m, K + 1 - q * m)
        if want_keep:
            kept.append(torch.empty((n, mq, p), dtype=dtype, device=dev))
            return kept[-1]
        return flat[: n * mq * p].view(n, mq, p)                 # one buffer serves every chunk: the emit has read it by then

    with torch.cuda.device(dev):
        cur = buffer(0)
        _be.cheb_step(None, B, ring[0], 0.0, 1.0, 0.0, flags, chunk=cur, slot=0)                     # w_0
        for k in range(K + 1):                                   # w_k is in ring[k % 2] and in slot k % m of `cur`
            q, s = divmod(k, m)
            if s == cur.size(1) - 1:
                _be.cheb_combine(0, cur, coef[q * m: q * m + cur.size(1)], Y, plane, flags, accumulate=q > 0)
                if q + 1 < n_chunks:
                    cur = buffer(q + 1)
            if k == K:
                break
            f = 1.0 if k == 0 else 2.0
            prod = op.matmul(ring[k % 2])
            _be.cheb_step(prod, ring[k % 2], ring[(k + 1) % 2], f * a, f * b, 0.0 if k == 0 else 1.0, flags, chunk=cur,
                          slot=(k + 1) % m)
    out = Y[:, : n * p].reshape(T, n, p)
    return out, kept, m


def _adjoint_fused(op: SparseOperator, operand: _Operand, G: torch.Tensor, coef: torch.Tensor, a: float, b: float, kept, m: int,
                   need_a: bool, need_b: bool):
    """The adjoint recurrence on the HIP kernels for ``G`` (T, n, p): (a·Σ_{k<K} f_k·SDDMM(μ_{k+1}, w_k) at the stored entries in
    A's value order or None, μ_0 or None).  ``kept``: the forward's chunks of w_k (chunk length m)."""
    T, n, p = G.shape
    K = coef.size(0) - 1
    dev, dtype = G.device, G.dtype
    align = _be.expm_geometry(dtype, n, p)[2]
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    Gp, plane = _planes(n, p, T, dtype, dev, align, source=G)
    ring = [torch.zeros((n, p), dtype=dtype, device=dev), torch.zeros((n, p), dtype=dtype, device=dev)]   # μ_j lives in ring[j % 2]
    gvals = None
    with torch.cuda.device(dev):
        for q in range((K - 1) // m, -1, -1) if K > 0 else ():
            cq = min(m, K - q * m)                               # slot s holds μ_{qm+s+1}, the partner of w_{qm+s}
            M = torch.empty((n, cq, p), dtype=dtype, device=dev)
            _be.cheb_combine(1, M, coef[q * m + 1: q * m + 1 + cq], Gp, plane, flags)
            for s in range(cq - 1, -1, -1):
                j = q * m + s + 1
                x, prev = ring[(j + 1) % 2], ring[j % 2]         # μ_{j+1} and μ_{j+2}, which μ_j replaces
                if j == K:
                    _be.cheb_step(None, x, prev, 0.0, 0.0, 0.0, flags, src=M, src_slot=s, chunk=M, slot=s)
                else:
                    _be.cheb_step(op.matmul(x), x, prev, 2.0 * a, 2.0 * b, 1.0, flags, src=M, src_slot=s, chunk=M, slot=s)
            if need_a:
                if q == 0:
                    M[:, 0].mul_(0.5)                            # f_0 = 1 against the 2·a every other slot carries
                W = kept[q]
                left = M.reshape(n, cq * p)
                right = (W if W.size(1) == cq else W[:, :cq].contiguous()).reshape(n, cq * p)
                if operand.plan.perm is None:
                    part = _ops.sddmm(operand.plan, left, right)
                else:
                    part = _be.coo_sddmm(operand.indices[0], operand.indices[1], left, right)
                gvals = part if gvals is None else gvals.add_(part)
        mu0 = None
        if need_b:
            S0 = torch.empty((n, 1, p), dtype=dtype, device=dev)
            _be.cheb_combine(1, S0, coef[0:1], Gp, plane, flags)
            if K == 0:
                _be.cheb_step(None, ring[1], ring[0], 0.0, 0.0, 0.0, flags, src=S0, src_slot=0)
            else:
                _be.cheb_step(op.matmul(ring[1]), ring[1], ring[0], a, b, 1.0, flags, src=S0, src_slot=0)
            mu0 = ring[0]
    if need_a:
        gvals = torch.zeros_like(operand.values) if gvals is None else gvals.mul_(2.0 * a)
    return gvals, mu0


# ---- the autograd function -----------------------------------------------------------------------------------------------------------

class SparseExpmMM(torch.autograd.Function):
    """Autograd function behind :func:`sparse_expm_mm`: ``apply(A, B, t, coef, a, b, chunk, info)`` with ``t`` a tensor (the gradient's
    shape; its values are already in ``coef``) or None, ``coef`` the float64 numpy table (K + 1, T, 1 or p) and ``info`` a dict the
    forward fills (or None); returns ``Σ_k c_k·w_k`` as (T, *B.shape)."""

    @staticmethod
    def forward(ctx, A, B, t, coef, a, b, chunk, info):
        A, B = A.detach(), B.detach()
        vector = B.dim() == 1
        Bm = B.unsqueeze(1) if vector else B
        n, p = Bm.shape
        K, T = coef.shape[0] - 1, coef.shape[1]
        table = torch.as_tensor(np.array(np.broadcast_to(coef, (K + 1, T, p)), order="C"), dtype=A.dtype).to(A.device).contiguous()  # [k][time][column]
        want_keep = bool(ctx.needs_input_grad[0])
        if Bm.is_cuda:
            op = SparseOperator(A)
            Y, kept, m = _expm_fused(op, Bm, table, a, b, want_keep, chunk)
            fused = True
        else:
            from . import _cpu

            op = SparseOperator(A)
            Y, kept = _cpu.expm_apply(op.matmul, Bm, table, a, b, want_keep)
            m, fused = 1, False
        record_solve(solver="sparse_expm_mm", iterations=K, tolerance_reached=True, terms=K, times=T, chunk=m, fused=fused)
        if info is not None:
            info.update(terms=K, chunk=m, fused=fused)
        ctx.A, ctx.vector, ctx.kept, ctx.m, ctx.a, ctx.b, ctx.fused = A, vector, kept, m, a, b, fused
        ctx.t_shape, ctx.t_dtype = (None, None) if t is None else (tuple(t.shape), t.dtype)
        ctx.save_for_backward(table, Y if ctx.needs_input_grad[2] else None)
        return Y.squeeze(2) if vector else Y

    @staticmethod
    @once_differentiable
    def backward(ctx, G):  # type: ignore[override]
        table, Y = ctx.saved_tensors
        A = ctx.A
        need_a, need_b, need_t = ctx.needs_input_grad[:3]
        if not (need_a or need_b or need_t):
            return (None,) * 8
        Gm = (G.unsqueeze(2) if ctx.vector else G).to(A.dtype)
        Gm = _aligned(Gm) if Gm.is_cuda else Gm.contiguous()
        T, n, p = Gm.shape
        op = SparseOperator(A)
        operand = _Operand(A)
        gradA = gradB = gradT = None
        if need_a or need_b:
            if ctx.fused:
                gvals, mu0 = _adjoint_fused(op, operand, Gm, table, ctx.a, ctx.b, ctx.kept, ctx.m, bool(need_a), bool(need_b))
            else:
                from . import _cpu

                if operand.plan.perm is None:
                    sddmm = lambda L, R: _ops.sddmm(operand.plan, L, R)                                   # noqa: E731
                else:
                    sddmm = lambda L, R: _cpu.coo_sddmm(operand.indices[0], operand.indices[1], L, R)      # noqa: E731
                gvals, mu0 = _cpu.expm_adjoint(op.matmul, sddmm, Gm, table, ctx.a, ctx.b, ctx.kept if need_a else None, bool(need_b))
                if need_a and gvals is None:
                    gvals = torch.zeros_like(operand.values)
            if need_a:
                gradA = operand.rebuild(gvals.reshape(operand.values.shape))
            if need_b:
                gradB = mu0.squeeze(1) if ctx.vector else mu0
        if need_t:
            # d/dt exp(tA) b = A exp(tA) b: <G_j, A Y_j> per time and column
            per = torch.stack([_be.coldot(Gm[j], op.matmul(Y[j].contiguous())) for j in range(T)])       # (T, p)
            shape = ctx.t_shape
            gradT = per.sum() if len(shape) == 0 else per.sum(dim=1) if len(shape) == 1 else per
            gradT = gradT.reshape(shape).to(ctx.t_dtype)
        return gradA, gradB, gradT, None, None, None, None, None


# ---- the public entry ------------------------------------------------------------------------------------------------------------------

def sparse_expm_mm(A: torch.Tensor, B: torch.Tensor, t=1.0, *, bounds=None, tolerance: float = 1e-6, max_terms: int = 4096,
                   return_info: bool = False):
    r"""``exp(t·A)·B`` for the sparse symmetric ``A``, differentiable with respect to ``A``, ``B`` and ``t``.

    With a graph or mesh Laplacian ``L``, ``sparse_expm_mm(L, X, -t)`` is heat-kernel diffusion of the features ``X`` for the time ``t``.

    ``A``   2-D square COO (coalesced first) or CSR, float32 or float64, int32 or int64 indices; taken as symmetric.  Batched, hybrid
            and bfloat16 operands are refused.
    ``B``   dense ``(n,)`` or ``(n, p)`` with ``A``'s dtype and device.  On the GPU the kernels take any ``p ≤ 256`` and wider blocks in
            multiples of the 16-byte lane (4 float32 / 2 float64 columns, up to 256 lanes); another width raises ``RuntimeError``
            with this rule — split such a block by columns.
    ``t``   a Python float or 0-d tensor: the result has ``B``'s shape.  A ``(T,)`` tensor of times: the result is ``(T, *B.shape)``.
            A ``(T, p)`` tensor: one time per slice and column (``(1, p)`` is a learned time per channel).  ``T`` is at most 8.  ``t``
            is read on the host to build the coefficient table (for a GPU tensor the call's one synchronisation); a ``t`` tensor
            that requires grad receives ``⟨G, A·Y⟩`` in its own shape.  ``t = 0`` returns ``B`` exactly.
    ``bounds``  ``(lo, hi)`` enclosing ``A``'s spectrum, as floats with ``lo ≤ hi``: used as given (with a float ``t`` the call then
            reads nothing on the host).  ``None`` computes Gershgorin's interval from the values (one host read): rigorous, no
            definiteness needed; a loose interval only costs terms.  ``lo = hi`` reduces to ``e^{t·lo}·B``, a polynomial of degree 0 in
            ``A``: its ``grad_A`` is ZERO although that of ``exp(t·A)·B`` is not.  Gershgorin's interval is such a point for the
            1 × 1 matrix and for ``c·I``; pass a wider interval to differentiate those with respect to ``A``.
    ``tolerance`` / ``max_terms``   the expansion is cut at the smallest ``K`` with ``2·Σ_{k>K} ive_k(|t|·ρ) ≤ tolerance``
            (``ρ = (hi − lo)/2``), which bounds every column's 2-norm error by ``tolerance·e^{max(t·lo, t·hi)}·‖b‖`` before rounding;
            a ``K`` above ``max_terms`` raises ``ValueError`` naming ``|t|·ρ`` and the ``K`` needed.
    ``return_info``     also return a dict: ``terms`` (K), ``bounds``, ``chunk`` (steps between two updates of the results) and
            ``fused`` (whether the HIP loop ran).

    The gradient with respect to ``A`` is a sparse tensor on ``A``'s own index tensors (stored entries only, unsymmetrised), exact
    for the approximant; the bounds and the coefficients are constants of the call.  Differentiable once."""
    return _entry(A, B, t, bounds, tolerance, max_terms, return_info)


def _entry(A, B, t, bounds, tolerance, max_terms, return_info, chunk=None):
    """:func:`sparse_expm_mm` with the fused loop's chunk length as an argument (tests and tools/expmbench.py)."""
    who = "sparse_expm_mm"
    _check(who, A, B, t, bounds, tolerance, max_terms)
    if A.layout == torch.sparse_coo and not A.is_coalesced():
        A = A.coalesce()
    if bounds is None:
        lo, hi = _gershgorin(A.detach())
    else:
        lo, hi = (float(x) for x in bounds)
    t_tensor = t if isinstance(t, torch.Tensor) else None
    t_host = t_tensor.detach().to("cpu", torch.float64).numpy() if t_tensor is not None else np.float64(t)
    p = 1 if B.dim() == 1 else B.size(1)
    scalar_t = t_host.ndim == 0
    t2 = t_host.reshape(1, 1) if scalar_t else t_host.reshape(-1, 1) if t_host.ndim == 1 else t_host
    coef, a, b, K = _coefficients(who, t2, lo, hi, float(tolerance), int(max_terms))
    info = {"bounds": (lo, hi)} if return_info else None
    if t_tensor is not None and t_tensor.device != B.device and t_tensor.requires_grad:
        raise RuntimeError(f"{who}: a t that requires grad must be on the device of B, got {t_tensor.device} and {B.device}")
    out = SparseExpmMM.apply(A, B, t_tensor, coef, a, b, chunk, info)
    if scalar_t:
        out = out.squeeze(0)
    return (out, info) if return_info else out
