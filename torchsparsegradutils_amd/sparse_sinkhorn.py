"""Entropic optimal transport on a sparse pattern: a fixed number of log-domain Sinkhorn iterations over the stored entries.

The doubly-normalised form of :func:`sparse_log_softmax`.  The stored values of ``S`` are a log-kernel (``−C/ε``); only stored
entries are admissible couplings (absent entries are −inf, not ``exp(0)`` terms).  With ``v⁰ = 0``, iteration ``t = 1..T`` does

    u^t_i = log_a_i − LSE_{j ∈ row i}(S_ij + v^{t−1}_j)
    v^t_j = log_b_j − LSE_{i ∈ col j}(S_ij + u^t_i)

and the result is ``log_P_ij = S_ij + u^T_i + v^T_j`` on ``S``'s own index tensors, with the potentials ``u^T`` and ``v^T``.  The
column marginals of ``exp(log_P)`` are exact after every iteration, the row marginals converge.  The reference has no counterpart.

The groups are those of the log-sum-exp: the rows of a CSR / coalesced-COO matrix are the segments of its own ``crow``, its
columns those of the cached transpose (values read through its ``perm``), a CSC matrix is the same with the roles exchanged, and
a batched input is one block-diagonal pattern.  GPU operands run the fused kernels of ``csrc/sinkhorn.hip`` (one launch per half
step, two where a group crosses a range of the walk, and an n- or m-sized addition after it when a gradient is kept); CPU operands the torch-op path of ``_cpu.py``.  The loop has a fixed
length, synchronises nothing and allocates only through torch, so it can be captured in a ``torch.cuda.graph``.

Autograd is first order only and exact for the ``T`` unrolled iterations: a reverse sweep that recomputes every softmax weight
from what the forward keeps of its iteration — ``u^1..u^T`` and ``v^1..v^T`` less their log marginals, that is the negated
log-sum-exps of the ``2T`` half steps (``T·(n + m)`` accumulator values; ``v⁰ = 0`` is not kept) — and no nnz-sized tensor beyond
the values of ``S``.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch.autograd.function import once_differentiable

from . import _backend as _be
from . import _cpu
from .sparse_logsumexp import _check_input, _Operand
from .sparse_softmax import _crossing, _restrict

__all__ = ["sparse_sinkhorn", "SparseSinkhorn"]

_DTYPES = (torch.float32, torch.float64, torch.bfloat16)


class _Direction(NamedTuple):
    """One direction of the pattern as the kernels walk it: group g holds the entries [ptr[g], ptr[g + 1]), entry k is value
    perm[k] (k without a perm), lies in group idx[k] of the other direction and in group grp[k] of this one."""
    ptr: torch.Tensor
    perm: Optional[torch.Tensor]
    idx: torch.Tensor
    grp: torch.Tensor
    n: int
    crossing: bool


def _directions(op: _Operand, dtype: torch.dtype):
    """(row direction, column direction) of the operand's block-diagonal pattern; cached with the pattern, per range length
    (whether a group crosses a range of the kernels is read back once, when the pattern is first seen)."""
    g = op.plan
    R = _be.segment_softmax_range(dtype) if g.crow.is_cuda else 0
    own, key = g.core.own, f"sinkhorn_directions{R}"
    d = own.get(key)
    if d is None:
        def one(h):
            ptr = h.crow.contiguous()
            return _Direction(ptr, None if h.perm is None else h.perm.contiguous(), h.col.contiguous(), h.row_indices().contiguous(),
                              h.n_rows, bool(R) and _crossing(ptr, R))
        first, second = one(g), one(g.transposed)
        d = own[key] = (first, second) if op.rows_first else (second, first)
    return d


def _accumulator(dtype: torch.dtype) -> torch.dtype:
    return torch.float32 if dtype == torch.bfloat16 else dtype


def _workspace(val: torch.Tensor, *dirs: _Direction):
    if val.is_cuda and val.numel() and any(d.crossing for d in dirs):
        return torch.empty(_be.sinkhorn_workspace_bytes(val.dtype, val.numel()), dtype=torch.uint8, device=val.device)
    return None


def _potential(log_marg, neg_lse: torch.Tensor, out=None) -> torch.Tensor:
    """The potential of a half step from what the history keeps of it, −lse: log_marg − lse, with the rounding of the subtraction
    the half step itself does (a sum with the negated value is the same operation)."""
    if log_marg is None:
        return neg_lse
    return torch.add(log_marg, neg_lse, out=out)


def _iterate(rowd: _Direction, cold: _Direction, val: torch.Tensor, la, lb, T: int, keep: bool):
    """(NU, NV, u^T, v^T).  With `keep`, NU[t − 1] = −LSE_row(S + v^{t−1}) and NV[t − 1] = −LSE_col(S + u^t): the potentials of
    iteration t less their log marginals, which is what the reverse sweep wants — the weight of an entry is then the exponential of
    the half step's own staged value less its own lse, and the weights of a group sum to one up to the rounding of the sum, whatever
    the size of the potentials.  Without `keep` (None, None): one buffer each, written by the half steps themselves."""
    acc = _accumulator(val.dtype)
    if not val.is_cuda:
        return _cpu.sinkhorn_forward(rowd, cold, val, la, lb, T, keep)
    dev = val.device
    ws = _workspace(val, rowd, cold)
    wr, wc = (ws if rowd.crossing else None), (ws if cold.crossing else None)
    u = torch.empty(rowd.n, dtype=acc, device=dev)
    v = torch.zeros(cold.n, dtype=acc, device=dev)
    if not keep:
        for _ in range(T):       # (the column step does not read v)
            _be.sinkhorn_half(rowd.ptr, rowd.perm, rowd.idx, val, v, la, u, wr)
            _be.sinkhorn_half(cold.ptr, cold.perm, cold.idx, val, u, lb, v, wc)
        return None, None, u, v
    NU = torch.empty((T, rowd.n), dtype=acc, device=dev)
    NV = torch.empty((T, cold.n), dtype=acc, device=dev)
    pu, pv = u, v
    for t in range(T):
        _be.sinkhorn_half(rowd.ptr, rowd.perm, rowd.idx, val, pv, None, NU[t], wr)
        pu = _potential(la, NU[t], out=u)
        _be.sinkhorn_half(cold.ptr, cold.perm, cold.idx, val, pu, None, NV[t], wc)
        pv = _potential(lb, NV[t], out=v)
    return NU, NV, pu, pv


class SparseSinkhorn(torch.autograd.Function):
    """Autograd kernel behind :func:`sparse_sinkhorn` (once differentiable)."""

    @staticmethod
    def forward(ctx, A, log_a, log_b, op, T):
        val = op.values.reshape(-1)
        rowd, cold = _directions(op, val.dtype)
        la = None if log_a is None else log_a.detach().reshape(-1).contiguous()
        lb = None if log_b is None else log_b.detach().reshape(-1).contiguous()
        keep = any(ctx.needs_input_grad[:3])
        NU, NV, u, v = _iterate(rowd, cold, val, la, lb, T, keep)
        first, pots = (rowd, (u, v)) if op.rows_first else (cold, (v, u))
        if val.is_cuda:
            y = _be.sinkhorn_plan(first.ptr, first.idx, val, *pots)
        else:
            y = _cpu.sinkhorn_plan(first.grp, first.idx, val, *pots)
        ctx.op, ctx.T, ctx.in_dtype = op, T, val.dtype
        ctx.has_a, ctx.has_b = la is not None, lb is not None
        if keep:
            ctx.save_for_backward(op.values, NU, NV, *(t for t in (la, lb) if t is not None))
        b = op.batch
        shape = (lambda n: (n,)) if b is None else (lambda n: (b, n // b))
        # (copies: a potential may be a row of the history, which stays the backward's own)
        return op.rebuild(y), u.clone().view(shape(rowd.n)), v.clone().view(shape(cold.n))

    @staticmethod
    @once_differentiable
    def backward(ctx, gP, gu, gv):
        need_S, need_a, need_b = ctx.needs_input_grad[:3]
        values, NU, NV, *marg = ctx.saved_tensors
        la = marg.pop(0) if ctx.has_a else None
        lb = marg.pop(0) if ctx.has_b else None
        op: _Operand = ctx.op
        val = values.reshape(-1)
        acc = NU.dtype
        rowd, cold = _directions(op, val.dtype)
        dev = val.device
        if gP is None:
            dS = torch.zeros(val.numel(), dtype=acc, device=dev)
        else:
            dS = _restrict(op, gP).reshape(-1).to(acc).clone(memory_format=torch.contiguous_format)
        gu = None if gu is None else gu.reshape(-1).to(acc).contiguous()
        gv = None if gv is None else gv.reshape(-1).to(acc).contiguous()
        if val.is_cuda:
            dla, dlb = _gpu_sweep(rowd, cold, val, la, lb, NU, NV, dS, gu, gv, ctx.T)
        else:
            dla, dlb = _cpu.sinkhorn_backward(rowd, cold, val, la, lb, NU, NV, dS, gu, gv, ctx.T)
        b = op.batch
        shape = (lambda n: (n,)) if b is None else (lambda n: (b, n // b))
        return (op.rebuild(dS.to(ctx.in_dtype)) if need_S else None,
                dla.view(shape(rowd.n)) if need_a and ctx.has_a else None,
                dlb.view(shape(cold.n)) if need_b and ctx.has_b else None, None, None)


def _gpu_sweep(rowd, cold, val, la, lb, NU, NV, dS, gu, gv, T: int):
    """The reverse sweep on the kernels: `dS` comes in as the cotangent of log_P and leaves as the gradient of the values."""
    acc, dev = NU.dtype, val.device
    ws = _workspace(val, rowd, cold)
    wr, wc = (ws if rowd.crossing else None), (ws if cold.crossing else None)
    ub = torch.empty(rowd.n, dtype=acc, device=dev)
    vb = torch.empty(cold.n, dtype=acc, device=dev)
    _be.segment_sum(rowd.ptr, rowd.perm, dS, gu, ub, wr)
    _be.segment_sum(cold.ptr, cold.perm, dS, gv, vb, wc)
    dla = torch.zeros(rowd.n, dtype=acc, device=dev)
    dlb = torch.zeros(cold.n, dtype=acc, device=dev)
    u_buf = None if la is None else torch.empty_like(ub)
    v_buf = None if lb is None else torch.empty_like(vb)
    v0 = torch.zeros_like(vb)
    for t in range(T, 0, -1):
        dlb += vb
        u_t = _potential(la, NU[t - 1], out=u_buf)
        # v^t = log_b − LSE_col(S + u^t), −lse kept in NV[t − 1]: w_ij = exp((S_ij + u^t_i) + NV[t − 1]_j); the row walk gives
        # ū −= Σ_j v̄_j·w_ij (ū is zero again after the first pass)
        _be.sinkhorn_half_backward(rowd.ptr, rowd.perm, rowd.idx, rowd.grp, val, u_t, NV[t - 1], None, vb, dS, ub, t == T, wr)
        dla += ub
        v_before = _potential(lb, NV[t - 2], out=v_buf) if t > 1 else v0
        # u^t = log_a − LSE_row(S + v^{t−1}), −lse kept in NU[t − 1]: the column walk gives v̄ = −Σ_i ū_i·w_ij
        _be.sinkhorn_half_backward(cold.ptr, cold.perm, cold.idx, cold.grp, val, v_before, NU[t - 1], None, ub, dS, vb, False, wc)
    return dla, dlb


def _check_marginal(name: str, t, want_shape, acc: torch.dtype, S: torch.Tensor):
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided:
        raise TypeError(f"sparse_sinkhorn: {name} must be a dense tensor or None")
    if tuple(t.shape) != tuple(want_shape):
        raise ValueError(f"sparse_sinkhorn: {name} must have shape {tuple(want_shape)} for S of shape {tuple(S.shape)}, "
                         f"got {tuple(t.shape)}")
    if t.dtype != acc:
        raise TypeError(f"sparse_sinkhorn: {name} must have dtype {acc} for {S.dtype} values, got {t.dtype}")
    if t.device != S.device:
        raise RuntimeError(f"all operands must be on the same device, got {S.device} and {t.device}")


def sparse_sinkhorn(S: torch.Tensor, log_a: Optional[torch.Tensor] = None, log_b: Optional[torch.Tensor] = None, n_iters: int = 20):
    r"""``n_iters`` log-domain Sinkhorn iterations on the stored entries of a sparse COO / CSR / CSC tensor: ``(log_P, u, v)``.

    ``S`` is ``(n, m)`` or batched ``(b, n, m)`` with float32, float64 or bfloat16 values (the log-kernel ``−C/ε``) and int32 or
    int64 indices; uncoalesced COO is coalesced first.  Only stored entries are admissible: an absent entry, like a stored
    ``-inf``, carries no mass.  ``log_a`` (``(n,)`` / ``(b, n)``) and ``log_b`` (``(m,)`` / ``(b, m)``) are the log marginals,
    ``None`` meaning zeros (matrix balancing); they and the potentials have ``S``'s dtype, float32 for bfloat16 values.

    With ``v⁰ = 0``, every iteration sets ``u_i = log_a_i − LSE_{j ∈ row i}(S_ij + v_j)`` and then
    ``v_j = log_b_j − LSE_{i ∈ col j}(S_ij + u_i)``.  ``log_P`` has ``S``'s layout and shape and carries its index tensors
    themselves; its values are ``S_ij + u_i + v_j`` (bfloat16: computed in float32 and rounded once), so the columns of
    ``exp(log_P)`` sum to ``exp(log_b)`` exactly and its rows to ``exp(log_a)`` in the limit.  A row or column without entries has
    the potential ``+inf``, which no entry reads.  There is no tolerance and no early stop.

    Differentiable once in ``S``, ``log_a`` and ``log_b`` for cotangents of all three outputs: the exact derivative of the unrolled
    iterations; the gradient of ``S`` is sparse on the same index tensors.
    """
    if not isinstance(S, torch.Tensor):
        raise TypeError(f"sparse_sinkhorn: S must be a sparse tensor, got {type(S).__name__}")
    _check_input(S, "sparse_sinkhorn")
    if S.dtype not in _DTYPES:
        raise TypeError(f"sparse_sinkhorn: values must be float32, float64 or bfloat16, got {S.dtype}")
    if not isinstance(n_iters, int) or isinstance(n_iters, bool):
        raise TypeError(f"sparse_sinkhorn: n_iters must be an int, got {type(n_iters).__name__}")
    if n_iters < 1:
        raise ValueError(f"sparse_sinkhorn: n_iters must be at least 1, got {n_iters}")
    acc = _accumulator(S.dtype)
    lead = tuple(S.shape[:-2])
    _check_marginal("log_a", log_a, lead + (S.size(-2),), acc, S)
    _check_marginal("log_b", log_b, lead + (S.size(-1),), acc, S)
    op = _Operand(S)
    return SparseSinkhorn.apply(op.A, log_a, log_b, op, n_iters)
