"""Restatements of sparse_sinkhorn in plain torch, differentiable by torch autograd (never the package's code).

`dense` is the definition: the stored entries scattered into a dense −inf matrix, `torch.logsumexp` along rows and columns, T
iterations from v⁰ = 0.  `entries` is the same arithmetic on the stored entries only (group maximum by `scatter_reduce`, the sum
of exponentials by `index_add`), for patterns whose dense form does not fit: a matrix of the structural cases has ~10³ rows and
~10⁵ columns.  The CPU tests hold `entries` against `dense`.  Both run in the dtype of `vals`: float64 is the reference, float32
the yardstick of what single precision can reach on the same inputs.

All take COO positions `rows`, `cols` (int64, distinct pairs) and return (log_P values in the given order, u, v).
"""

import torch

NEG_INF = float("-inf")


def _masked_lse(X, mask, dim):
    """logsumexp over the admissible entries along `dim`; −inf where there is none (with a zero, not NaN, gradient)."""
    some = mask.any(dim=dim, keepdim=True)
    safe = torch.where(mask, X, torch.full_like(X, NEG_INF))
    safe = torch.where(some, safe, torch.zeros_like(X))
    out = torch.logsumexp(safe, dim=dim)
    return torch.where(some.squeeze(dim), out, torch.full_like(out, NEG_INF))


def dense(rows, cols, vals, n, m, log_a=None, log_b=None, T=20):
    dt = vals.dtype
    D = torch.full((n, m), NEG_INF, dtype=dt).index_put((rows, cols), vals)
    mask = torch.zeros((n, m), dtype=torch.bool).index_put((rows, cols), torch.ones_like(rows, dtype=torch.bool))
    mask = mask & (D > NEG_INF)                    # a stored −inf acts as an absent entry
    la = torch.zeros(n, dtype=dt) if log_a is None else log_a
    lb = torch.zeros(m, dtype=dt) if log_b is None else log_b
    v = torch.zeros(m, dtype=dt)
    for _ in range(T):
        u = la - _masked_lse(D + v[None, :], mask, 1)
        v = lb - _masked_lse(D + u[:, None], mask, 0)
    return vals + u[rows] + v[cols], u, v


def _group_lse(x, grp, n_groups):
    """log Σ exp of x over the groups `grp`; −inf for a group without finite entries."""
    top = torch.full((n_groups,), NEG_INF, dtype=x.dtype).scatter_reduce(0, grp, x.detach(), "amax", include_self=True)
    shift = torch.where(top.isfinite(), top, torch.zeros_like(top))
    total = torch.zeros(n_groups, dtype=x.dtype).index_add(0, grp, (x - shift[grp]).exp())
    some = total > 0
    return torch.where(some, shift + torch.where(some, total, torch.ones_like(total)).log(), torch.full_like(total, NEG_INF))


def entries(rows, cols, vals, n, m, log_a=None, log_b=None, T=20):
    dt = vals.dtype
    la = torch.zeros(n, dtype=dt) if log_a is None else log_a
    lb = torch.zeros(m, dtype=dt) if log_b is None else log_b
    v = torch.zeros(m, dtype=dt)
    for _ in range(T):
        u = la - _group_lse(vals + v[cols], rows, n)
        v = lb - _group_lse(vals + u[rows], cols, m)
    return vals + u[rows] + v[cols], u, v


def with_grads(fn, rows, cols, vals, n, m, log_a, log_b, T, cot):
    """((log_P, u, v), (dS, dlog_a, dlog_b)) of restatement `fn` in the dtype of `vals` for the cotangents `cot` = (gP, gu, gv) of
    its outputs (cast to that dtype)."""
    dt = vals.dtype
    leaves = [vals.detach().clone().requires_grad_(True)]
    la = lb = None
    if log_a is not None:
        la = log_a.detach().to(dt).clone().requires_grad_(True)
        leaves.append(la)
    if log_b is not None:
        lb = log_b.detach().to(dt).clone().requires_grad_(True)
        leaves.append(lb)
    lp, u, v = fn(rows, cols, leaves[0], n, m, la, lb, T)
    grads = list(torch.autograd.grad((lp, u, v), leaves, tuple(c.to(dt) for c in cot)))
    dS = grads.pop(0)
    dla = grads.pop(0) if log_a is not None else None
    dlb = grads.pop(0) if log_b is not None else None
    return (lp.detach(), u.detach(), v.detach()), (dS, dla, dlb)
