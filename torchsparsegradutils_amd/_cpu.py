"""CPU tensors: the package's own torch-op path.

BASELINE ``configs[0]`` is "sparse_mm COO 4096×4096 … on CPU (plumbing, no GPU)" and the reference runs on CPU by default
(``sparse_matmul.py:141-163``; its tests use ``DEVICES=[torch.device("cpu")]``).  Operands that live on the CPU are therefore
computed here, with the ATen calls the reference itself makes at the cited lines — and ONLY such operands: the switch is the
device of the tensors, nothing else.  A tensor on the GPU never reaches this module (every function refuses one), and a missing
``libtsgu_hip.so`` is an error for GPU operands, not a reason to come here: this is the reference's own CPU behaviour for CPU
callers, not a fallback of the MI355X path.  Nothing here touches ``oracle/`` (test infrastructure).

=========================================  ====================================================================
reference (file:line)                      here
=========================================  ====================================================================
``torch.sparse.mm(A, B)``  :155            :func:`spmm` on the cached 2-D (block-diagonal if batched) pattern
gathers · mul · sum  :186-205              :func:`sddmm`, in entry chunks: the nnz×p temporaries never exist
``torch.sparse.mm(A.t(), G)``  :229        :func:`spmm` on the cached transposed pattern
``torch.triangular_solve``  _compat:42-48  :func:`sptrsm` (the same call, same flags)
column dots of the Krylov loops            :func:`coldot`
``_scatter_logsumexp``  sparse_logsumexp.py:10-73   :func:`segment_logsumexp` / :func:`segment_logsumexp_backward` on the
                                           segments of a cached pattern (every stored entry is one term)
nested-tensor ``segment_mm`` / ``gather_mm``        :func:`segment_mm` / :func:`segment_mm_grad_b`: rows in plan order (a
  indexed_matmul.py:95-105, :203-217       stable argsort of ``idx_b`` for gather_mm), one ``torch.matmul`` per segment,
                                           scattered back
(none: the reference has no attention)     :func:`attention` / :func:`attention_backward`: gather, per-entry dot,
                                           :func:`segment_softmax` per head, ``index_add``
``torch.sparse.mm(A, B, reduce)`` (ATen)   :func:`mm_reduce` / :func:`mm_reduce_backward` on the 2-D CSR arrays
``torch.sparse.mm(S1, S2)`` (ATen)         :func:`spgemm` / :func:`spgemm_backward` on coalesced COO operands
(none: torch's CPU BSR product refuses     :func:`bsr_mm` / :func:`bsr_mm_backward`: gather the slabs of ``B`` by block column,
  non-square blocks and bfloat16)          ``torch.bmm``, ``index_add_`` by block row — and the mirror for the gradients
=========================================  ====================================================================
"""

from __future__ import annotations

import torch

from . import _pattern as _pt

# entries per chunk of the masked product: chunk × p elements of temporaries (two gathers and a product) at a time
_SDDMM_CHUNK_ELEMS = 1 << 22


def _cpu_only(*tensors) -> None:
    for t in tensors:
        if t is not None and t.is_cuda:
            raise RuntimeError("torchsparsegradutils_amd._cpu was handed a GPU tensor: the torch-op path serves CPU operands only")


def _values_in_plan_order(plan: _pt.RowGather, values: torch.Tensor) -> torch.Tensor:
    v = values.reshape(-1)
    return v if plan.perm is None else v.index_select(0, plan.perm.reshape(-1).to(torch.int64))


def matrix(plan: _pt.RowGather, values: torch.Tensor) -> torch.Tensor:
    """The 2-D torch CSR tensor of (plan, values): A's own index arrays (int32 stays int32), block diagonal for a batched plan —
    what the reference assembles with ``sparse_block_diag`` for every batched input (sparse_matmul.py:151-153)."""
    f = _pt.flat_of(plan)
    return torch.sparse_csr_tensor(f.crow, f.col, _values_in_plan_order(f, values), (f.n_rows, f.n_cols))


def spmm(plan: _pt.RowGather, values: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A·B (reference sparse_matmul.py:155); with a transposed plan (``perm`` into A's values) it is Aᵀ·G (:229)."""
    _cpu_only(values, B, plan.crow)
    p = B.size(-1)
    out = torch.sparse.mm(matrix(plan, values), B.reshape(-1, p))
    return out.view(B.shape[:-2] + (plan.n_rows, p))


def sddmm(plan: _pt.RowGather, G: torch.Tensor, B: torch.Tensor, alpha: float = 1.0, swap_roles: bool = False) -> torch.Tensor:
    """alpha·<G[row k], B[col k]> (roles swapped: <B[row k], G[col k]>) at the plan's entries, in plan order, shaped like the
    plan's column array (reference sparse_matmul.py:186-205, sparse_solve.py:216-235)."""
    _cpu_only(G, B, plan.crow)
    f = _pt.flat_of(plan)
    p = G.size(-1)
    row_side = (B if swap_roles else G).reshape(-1, p)
    col_side = (G if swap_roles else B).reshape(-1, p)
    rows, cols = f.row_indices().reshape(-1).to(torch.int64), f.col.reshape(-1).to(torch.int64)
    nnz = cols.numel()
    out = torch.empty(nnz, dtype=torch.result_type(G, B), device=G.device)
    step = max(1, _SDDMM_CHUNK_ELEMS // max(p, 1))
    for s in range(0, nnz, step):
        e = min(nnz, s + step)
        torch.sum(row_side.index_select(0, rows[s:e]) * col_side.index_select(0, cols[s:e]), dim=-1, out=out[s:e])
    if alpha != 1.0:
        out.mul_(alpha)
    return out.view(plan.col.shape)


def coo_sddmm(rows: torch.Tensor, cols: torch.Tensor, G: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """The same product at explicit (row, column) pairs: un-coalesced COO, one gradient entry per stored duplicate
    (reference sparse_matmul.py:185,201-205)."""
    _cpu_only(rows, cols, G, B)
    nnz, p = rows.numel(), G.size(-1)
    out = torch.empty(nnz, dtype=torch.result_type(G, B), device=G.device)
    step = max(1, _SDDMM_CHUNK_ELEMS // max(p, 1))
    for s in range(0, nnz, step):
        e = min(nnz, s + step)
        torch.sum(G.index_select(0, rows[s:e]) * B.index_select(0, cols[s:e]), dim=-1, out=out[s:e])
    return out


def sptrsm(plan: _pt.RowGather, values: torch.Tensor, rhs: torch.Tensor, upper: bool, unit: bool, transpose: bool) -> torch.Tensor:
    """X = op(A)⁻¹·rhs by the legacy ATen call the reference keeps for sparse operands (_compat.py:42-48), same flags."""
    _cpu_only(values, rhs, plan.crow)
    if plan.n_rows == 0 or rhs.size(-1) == 0:
        return torch.empty_like(rhs)
    return torch.triangular_solve(rhs.contiguous(), matrix(plan, values), upper=upper, transpose=transpose, unitriangular=unit).solution


def coldot(X: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """Column-wise dot products of two (n, p) arrays -> (p,)."""
    _cpu_only(X, Y)
    return (X * Y).sum(dim=0)


def segment_logsumexp(ptr: torch.Tensor, perm, val: torch.Tensor, n_groups: int, include_zeros: bool, axis_len: int) -> torch.Tensor:
    """log Σ exp over the segments [ptr[g], ptr[g+1]) of val (through perm when given), plus one exp(0) per absent entry of the
    axis when include_zeros.  Shifted by the group's maximum (0 at least when absent entries count; 0 when it is not finite),
    so that NaN stays NaN, +inf gives +inf and an empty group gives -inf.  bf16 values accumulate in fp32."""
    _cpu_only(ptr, perm, val)
    acc = torch.float32 if val.dtype == torch.bfloat16 else val.dtype
    v = val.reshape(-1) if perm is None else val.reshape(-1).index_select(0, perm.to(torch.int64))
    v = v.to(acc)
    counts = (ptr[1:] - ptr[:-1]).to(torch.int64)
    grp = torch.repeat_interleave(torch.arange(n_groups), counts, output_size=v.numel())
    top = torch.full((n_groups,), float("-inf"), dtype=acc).scatter_reduce(0, grp, v, "amax", include_self=True)
    top = torch.where(torch.zeros(n_groups, dtype=acc).index_add(0, grp, v.isnan().to(acc)) > 0, float("nan"), top)
    zeros = (axis_len - counts).to(acc) if include_zeros else torch.zeros(n_groups, dtype=acc)
    shift = torch.where(zeros > 0, top.clamp(min=0.0), top)
    shift = torch.where(shift.isfinite(), shift, torch.zeros_like(shift))
    total = torch.zeros(n_groups, dtype=acc).index_add(0, grp, (v - shift[grp]).exp())
    total = total + torch.where(zeros > 0, zeros * (-shift).exp(), torch.zeros_like(total))
    out = torch.where(total == 0, float("-inf"), shift + total.log())
    return out.to(val.dtype)


def segment_logsumexp_backward(val, ptr, g_grp, lse_grp, idx, g_idx, lse_idx) -> torch.Tensor:
    """grad[k] = g_grp[grp(k)]·exp(val[k] − lse_grp[grp(k)]) + g_idx[idx[k]]·exp(val[k] − lse_idx[idx[k]]) in stored order."""
    _cpu_only(val, ptr, idx)
    acc = torch.float32 if val.dtype == torch.bfloat16 else val.dtype
    v = val.reshape(-1).to(acc)
    grad = torch.zeros_like(v)
    if ptr is not None:
        grp = torch.repeat_interleave(torch.arange(ptr.numel() - 1), (ptr[1:] - ptr[:-1]).to(torch.int64), output_size=v.numel())
        grad = grad + g_grp.to(acc)[grp] * (v - lse_grp.to(acc)[grp]).exp()
    if idx is not None:
        j = idx.reshape(-1).to(torch.int64)
        grad = grad + g_idx.to(acc)[j] * (v - lse_idx.to(acc)[j]).exp()
    return grad.to(val.dtype)


def _segment_ids(ptr: torch.Tensor, n_groups: int, nnz: int) -> torch.Tensor:
    return torch.repeat_interleave(torch.arange(n_groups), (ptr[1:] - ptr[:-1]).to(torch.int64), output_size=nnz)


def _from_plan_order(x: torch.Tensor, perm, dtype: torch.dtype) -> torch.Tensor:
    x = x.to(dtype)
    return x if perm is None else torch.empty_like(x).index_copy_(0, perm.to(torch.int64), x)


def segment_softmax(ptr: torch.Tensor, perm, val: torch.Tensor, n_groups: int, log_form: bool) -> torch.Tensor:
    """Softmax (or log-softmax) of val over the segments [ptr[g], ptr[g+1]) (entry k of a segment is val[perm[k]] when perm is
    given), returned in val's own order.  A group whose maximum is not finite (a NaN, a +inf, nothing but -inf) is NaN
    throughout, as torch.softmax on the group's values.  bf16 values are computed in fp32 and rounded once."""
    _cpu_only(ptr, perm, val)
    acc = torch.float32 if val.dtype == torch.bfloat16 else val.dtype
    v = (val.reshape(-1) if perm is None else val.reshape(-1).index_select(0, perm.to(torch.int64))).to(acc)
    grp = _segment_ids(ptr, n_groups, v.numel())
    top = torch.full((n_groups,), float("-inf"), dtype=acc).scatter_reduce(0, grp, v, "amax", include_self=True)
    top = torch.where(torch.zeros(n_groups, dtype=acc).index_add(0, grp, v.isnan().to(acc)) > 0, float("nan"), top)
    shift = torch.where(top.isfinite(), top, torch.zeros_like(top))
    d = v - shift[grp]
    e = d.exp()
    total = torch.zeros(n_groups, dtype=acc).index_add(0, grp, e)
    y = d - total.log()[grp] if log_form else e / total[grp]
    y = torch.where(top.isfinite()[grp], y, torch.full_like(y, float("nan")))
    return _from_plan_order(y, perm, val.dtype)


def segment_softmax_backward(ptr: torch.Tensor, perm, y: torch.Tensor, g: torch.Tensor, n_groups: int, log_form: bool) -> torch.Tensor:
    """gin = y·(g − Σ_group g·y), or g − exp(y)·Σ_group g for the log form; y, g and gin in the values' own order."""
    _cpu_only(ptr, perm, y, g)
    acc = torch.float32 if y.dtype == torch.bfloat16 else y.dtype
    pick = (lambda t: t.reshape(-1)) if perm is None else (lambda t: t.reshape(-1).index_select(0, perm.to(torch.int64)))
    yy, gg = pick(y).to(acc), pick(g).to(acc)
    grp = _segment_ids(ptr, n_groups, yy.numel())
    a, b = (gg, yy.exp()) if log_form else (gg * yy, yy)
    total = torch.zeros(n_groups, dtype=acc).index_add(0, grp, a)
    return _from_plan_order(a - b * total[grp], perm, y.dtype)


def _attention_terms(ptr, idx, perm, bias, Q, K, heads: int, scale: float):
    """(row of every entry, its column, the logits [nnz, heads]) of the walk (ptr, idx, perm) in the accumulator type."""
    acc = torch.float32 if Q.dtype == torch.bfloat16 else Q.dtype
    n, nnz = ptr.numel() - 1, idx.numel()
    rows, cols = _segment_ids(ptr, n, nnz), idx.reshape(-1).to(torch.int64)
    q, k = Q.to(acc).view(Q.size(0), heads, -1), K.to(acc).view(K.size(0), heads, -1)
    t = (q.index_select(0, rows) * k.index_select(0, cols)).sum(-1) * scale
    if bias is not None:
        b = bias.reshape(-1) if perm is None else bias.reshape(-1).index_select(0, perm.to(torch.int64))
        t = t + b.to(acc).unsqueeze(1)
    return rows, cols, t


def attention(ptr, idx, perm, bias, Q, K, V, heads: int, scale: float):
    """(O [n, heads·d], P [nnz, heads]) of attention over the pattern walked by rows as (ptr, idx, perm): gather, per-entry dot,
    the segmented softmax of every head over the rows' entries, index_add.  A row without entries gives zeros; a row whose logits
    hold a NaN or +inf, or nothing but -inf, is NaN (as :func:`segment_softmax`).  bf16 is computed in fp32 and rounded once."""
    _cpu_only(ptr, idx, perm, bias, Q, K, V)
    n = ptr.numel() - 1
    rows, cols, t = _attention_terms(ptr, idx, perm, bias, Q, K, heads, scale)
    P = torch.stack([segment_softmax(ptr, None, t[:, h].contiguous(), n, False) for h in range(heads)], 1)
    v = V.to(P.dtype).view(V.size(0), heads, -1)
    O = torch.zeros((n, heads, v.size(-1)), dtype=P.dtype).index_add_(0, rows, P.unsqueeze(-1) * v.index_select(0, cols))
    return O.view(n, -1).to(Q.dtype), P


def attention_backward(ptr, idx, perm, Q, K, V, dO, P, heads: int, scale: float, want_dA: bool):
    """(dQ, dK, dV, dA or None) of :func:`attention` from its probabilities P: dP = <dO[i], V[j]>, δ[i] = Σ_j P·dP,
    dS = P·(dP − δ); dQ = scale·Σ_j dS·K[j], dK = scale·Σ_i dS·Q[i], dV = Σ_i P·dO[i], dA = Σ_heads dS at the entry's own
    position of the value array."""
    _cpu_only(ptr, idx, perm, Q, K, V, dO, P)
    acc = P.dtype
    n, m, nnz = Q.size(0), K.size(0), idx.numel()
    rows, cols = _segment_ids(ptr, n, nnz), idx.reshape(-1).to(torch.int64)
    q, k, v, g = (x.to(acc).view(x.size(0), heads, -1) for x in (Q, K, V, dO))
    gi = g.index_select(0, rows)
    dP = (gi * v.index_select(0, cols)).sum(-1)
    delta = torch.zeros((n, heads), dtype=acc).index_add_(0, rows, P * dP)
    dS = P * (dP - delta.index_select(0, rows))
    dQ = torch.zeros_like(q).index_add_(0, rows, dS.unsqueeze(-1) * k.index_select(0, cols)) * scale
    dK = torch.zeros_like(k).index_add_(0, cols, dS.unsqueeze(-1) * q.index_select(0, rows)) * scale
    dV = torch.zeros_like(v).index_add_(0, cols, P.unsqueeze(-1) * gi)
    dA = _from_plan_order(dS.sum(1), perm, acc) if want_dA else None
    return dQ.view(n, -1).to(Q.dtype), dK.view(m, -1).to(Q.dtype), dV.view(m, -1).to(Q.dtype), dA


def segment_mm(bounds, perm, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """out[perm[i]] = a[perm[i]] @ b[r] for the positions i in [bounds[r], bounds[r + 1]) (perm None: identity); rows outside
    [bounds[0], bounds[-1]) are zeros.  One torch.matmul per segment; `b` may be a transposed view."""
    _cpu_only(a, b, perm)
    n, d2 = a.size(0), b.size(-1)
    ap = a if perm is None else a.index_select(0, perm)
    res = torch.zeros((n, d2), dtype=a.dtype)
    for r in range(len(bounds) - 1):
        lo, hi = bounds[r], bounds[r + 1]
        if hi > lo:
            res[lo:hi] = torch.matmul(ap[lo:hi], b[r])
    return res if perm is None else torch.zeros_like(res).index_copy_(0, perm, res)


def segment_mm_grad_b(bounds, perm, a: torch.Tensor, g: torch.Tensor, n_seg: int) -> torch.Tensor:
    """grad_b[r] = a[perm[i]]ᵀ g[perm[i]] summed over the positions i of segment r (zeros for an empty segment)."""
    _cpu_only(a, g, perm)
    ap = a if perm is None else a.index_select(0, perm)
    gp = g if perm is None else g.index_select(0, perm)
    out = torch.zeros((n_seg, a.size(1), g.size(1)), dtype=a.dtype)
    for r in range(n_seg):
        lo, hi = bounds[r], bounds[r + 1]
        if hi > lo:
            out[r] = torch.matmul(ap[lo:hi].t(), gp[lo:hi])
    return out


# ---- density reductions of the sparse multivariate normal (the torch-op twins of csrc/mvn.hip) ------------------------------------
def csr_diag_positions(crow: torch.Tensor, col: torch.Tensor, perm, n_rows: int) -> torch.Tensor:
    """pos[i] = position in the owner's value array of the first entry of row i with col == i, -1 when the row stores none."""
    _cpu_only(crow, col, perm)
    counts = (crow[1:] - crow[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n_rows), counts, output_size=col.numel())
    hit = torch.nonzero(col.to(torch.int64) == rows).flatten()
    big = col.numel()
    first = torch.full((n_rows,), big, dtype=torch.int64).scatter_reduce(0, rows[hit], hit, "amin", include_self=True)
    found = first < big
    at = first.clamp(max=max(big - 1, 0))
    own = at if perm is None else perm.to(torch.int64)[at] if big else at
    return torch.where(found, own, torch.full_like(own, -1)).to(crow.dtype)


def diag_logsum(pos, val: torch.Tensor, n_rows: int, rows_per_item: int) -> torch.Tensor:
    """Σ_i log(val[pos[i]]) per item (pos None: of the dense vector val); a row without a stored diagonal is log 0 = -inf."""
    _cpu_only(pos, val)
    v = val.reshape(-1)
    if pos is not None:
        p = pos.to(torch.int64)
        d = torch.where(p >= 0, v[p.clamp(min=0)] if v.numel() else torch.zeros(n_rows, dtype=v.dtype), torch.zeros((), dtype=v.dtype))
    else:
        d = v
    return d.log().view(-1, rows_per_item).sum(dim=1)


def diag_logsum_backward(pos, val: torch.Tensor, g: torch.Tensor, n_rows: int, rows_per_item: int, grad=None) -> torch.Tensor:
    """g[item] / val[pos[i]] at the diagonal positions: into a zero array, or added in place to `grad`."""
    _cpu_only(pos, val, g, grad)
    v = val.reshape(-1)
    ge = g.reshape(-1).repeat_interleave(rows_per_item)
    if pos is None:
        return ge / v
    if grad is None:
        grad = torch.zeros_like(v)
    p = pos.to(torch.int64)
    keep = p >= 0
    grad.view(-1)[p[keep]] += ge[keep] / v[p[keep]]
    return grad


def _quad_weight(w, w_mode: int):
    if w is None or w_mode == 0:
        return None
    return w.reshape(-1, 1) if w_mode == 1 else w.reshape(-1, 1).reciprocal()


def quadform(Y: torch.Tensor, E, w, w_mode: int, rows_per_item: int) -> torch.Tensor:
    """(items, k): Σ_i w_i^{±1} (Y[i,c] + E[i,c])² over the item's rows."""
    _cpu_only(Y, E, w)
    t = Y if E is None else Y + E
    q = t * t
    s = _quad_weight(w, w_mode)
    if s is not None:
        q = q * s
    return q.view(-1, rows_per_item, Y.size(1)).sum(dim=1)


def quadform_backward(Y: torch.Tensor, E, w, w_mode: int, rows_per_item: int, g: torch.Tensor, want_w: bool):
    """(grad_Y, grad_w or None) of `quadform`."""
    _cpu_only(Y, E, w, g)
    t = Y if E is None else Y + E
    ge = g.reshape(-1, 1, Y.size(1)).expand(-1, rows_per_item, -1).reshape(Y.shape)
    s = _quad_weight(w, w_mode)
    gY = 2 * ge * (t if s is None else s * t)
    gw = None
    if want_w and s is not None:
        gw = (ge * t * t).sum(dim=1)
        if w_mode == 2:
            gw = -gw * (s * s).reshape(-1)
    return gY, gw


def csr_row_sumsq(plan: _pt.RowGather, values: torch.Tensor, w, add) -> torch.Tensor:
    """out[i] = add[i] + Σ_{k in row i} val[k]² w[col[k]] on the 2-D plan."""
    _cpu_only(values, w, add, plan.crow)
    v = _values_in_plan_order(plan, values)
    q = v * v
    if w is not None:
        q = q * w.reshape(-1)[plan.col.reshape(-1).to(torch.int64)]
    out = torch.zeros(plan.n_rows, dtype=values.dtype).index_add_(0, plan.row_indices().reshape(-1).to(torch.int64), q)
    return out if add is None else out + add.reshape(-1)


def csr_row_sumsq_backward(plan: _pt.RowGather, values: torch.Tensor, w, g: torch.Tensor) -> torch.Tensor:
    """grad_val[k] = 2 g[row(k)] val[k] w[col[k]] in the value array's order."""
    _cpu_only(values, w, g, plan.crow)
    v = _values_in_plan_order(plan, values)
    q = 2 * g.reshape(-1)[plan.row_indices().reshape(-1).to(torch.int64)] * v
    if w is not None:
        q = q * w.reshape(-1)[plan.col.reshape(-1).to(torch.int64)]
    if plan.perm is None:
        return q
    out = torch.empty_like(q)
    out[plan.perm.reshape(-1).to(torch.int64)] = q
    return out


def mm_reduce(crow: torch.Tensor, col: torch.Tensor, values: torch.Tensor, B: torch.Tensor, shape, reduce: str) -> torch.Tensor:
    """``torch.sparse.mm(A, B, reduce)`` for the 2-D CSR arrays of A (block diagonal for a batched operand: absent entries do not
    take part, so the items do not see each other) — the CPU op whose semantics the HIP kernels of csrc/mm_reduce.hip restate."""
    _cpu_only(crow, col, values, B)
    # With an operand that requires a gradient the op runs the loop that tracks the winners — strict compare, the first of equal
    # candidates stays — and without one a vectorised maximum, which picks another sign for a tie of +0.0 and -0.0: the tracking
    # loop always, so that the result does not depend on who asks for gradients.
    with torch.enable_grad():
        A = torch.sparse_csr_tensor(crow, col, values.detach(), shape).requires_grad_(True)
        return torch.sparse.mm(A, B.detach(), reduce).detach()


def mm_reduce_backward(crow, col, values, B, shape, reduce: str, G, need_a: bool, need_b: bool):
    """(gradient of the values or None, gradient of B or None) of :func:`mm_reduce` by the op's own backward: the forward is
    evaluated again (the op keeps its winners to itself)."""
    _cpu_only(crow, col, values, B, G)
    with torch.enable_grad():
        A = torch.sparse_csr_tensor(crow, col, values.detach(), shape).requires_grad_(need_a)
        Bg = B.detach().requires_grad_(need_b)
        C = torch.sparse.mm(A, Bg, reduce)
        wanted = [t for t, need in ((A, need_a), (Bg, need_b)) if need]
        grads = list(torch.autograd.grad(C, wanted, G))
    ga = grads.pop(0).values() if need_a else None
    gb = grads.pop(0) if need_b else None
    return ga, gb


def spgemm(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``torch.sparse.mm(A, B)`` of two coalesced COO operands (float32 or float64): the structural product, coalesced."""
    _cpu_only(A, B)
    return torch.sparse.mm(A, B).coalesce()


def spgemm_backward(A: torch.Tensor, B: torch.Tensor, G: torch.Tensor, need_a: bool, need_b: bool):
    """(values of dL/dA, values of dL/dB) of :func:`spgemm` for the sparse gradient ``G`` on the product's pattern: torch's own
    backward of the op, which masks either gradient by its operand's pattern; values in the operand's (coalesced) order."""
    _cpu_only(A, B, G)
    with torch.enable_grad():
        a, b = A.detach().requires_grad_(need_a), B.detach().requires_grad_(need_b)
        C = torch.sparse.mm(a, b)
    wanted = [t for t, need in ((a, need_a), (b, need_b)) if need]
    grads = list(torch.autograd.grad(C, wanted, G)) if wanted else []
    out = []
    for t, need in ((A, need_a), (B, need_b)):
        if not need:
            out.append(None)
            continue
        g = grads.pop(0).coalesce()
        if g._nnz() != t._nnz() or not torch.equal(g._indices(), t._indices()):
            raise RuntimeError("torch.sparse.mm returned a gradient that is not on its operand's pattern")
        out.append(g._values())
    return out[0], out[1]


def _bsr_acc(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def bsr_mm(plan: _pt.RowGather, blocks: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """A·B for the 2-D block pattern `plan` with `blocks` (nnzb, bh, bw) and B (n_block_cols·bw, p): the slabs of B gathered by block
    column, one ``torch.bmm``, ``index_add_`` by block row (a block row's blocks in stored order).  Every stored block is a term.
    Accumulated in float32 for float32 and bfloat16 (rounded once), in float64 for float64.  No torch BSR product is called."""
    _cpu_only(plan.crow, blocks, B)
    nnzb, bh, bw = blocks.shape
    p = B.size(-1)
    acc = _bsr_acc(B.dtype)
    out = torch.zeros((plan.n_rows, bh, p), dtype=acc)
    if nnzb:
        slabs = B.reshape(plan.n_cols, bw, p).index_select(0, plan.col.to(torch.int64)).to(acc)
        out.index_add_(0, plan.row_indices().to(torch.int64), torch.bmm(blocks.to(acc), slabs))
    return out.reshape(plan.n_rows * bh, p).to(B.dtype)


def bsr_mm_backward(plan: _pt.RowGather, blocks: torch.Tensor, B: torch.Tensor, G: torch.Tensor, need_a: bool, need_b: bool):
    """(gradient of the blocks or None, gradient of B or None) of :func:`bsr_mm`: its mirror — dV[e] = G[I_e] · B[J_e]ᵀ per stored
    block, and dB = Aᵀ·G by ``index_add_`` of V[e]ᵀ · G[I_e] by block column."""
    _cpu_only(plan.crow, blocks, B, G)
    nnzb, bh, bw = blocks.shape
    p = B.size(-1)
    acc = _bsr_acc(B.dtype)
    rows, cols = plan.row_indices().to(torch.int64), plan.col.to(torch.int64)
    g_slabs = G.reshape(plan.n_rows, bh, p).index_select(0, rows).to(acc) if nnzb else None
    dblocks = dB = None
    if need_a:
        dblocks = torch.zeros((nnzb, bh, bw), dtype=B.dtype)
        if nnzb:
            b_slabs = B.reshape(plan.n_cols, bw, p).index_select(0, cols).to(acc)
            dblocks = torch.bmm(g_slabs, b_slabs.transpose(1, 2)).to(B.dtype)
    if need_b:
        out = torch.zeros((plan.n_cols, bw, p), dtype=acc)
        if nnzb:
            out.index_add_(0, cols, torch.bmm(blocks.to(acc).transpose(1, 2), g_slabs))
        dB = out.reshape(plan.n_cols * bw, p).to(B.dtype)
    return dblocks, dB


def bsr_element_walk(plan: _pt.RowGather, bh: int, bw: int):
    """(ptr, idx, perm) of the element pattern that the 2-D block pattern `plan` of bh × bw blocks covers, walked by rows: every
    element row lists its block row's blocks in stored order, each block's bw columns in order; perm is the element's position in
    the packed (nnzb, bh, bw) value array.  A repeated (I, J) lists its columns twice."""
    crow, col = plan.crow.to(torch.int64), plan.col.to(torch.int64)
    nrb = plan.n_rows
    counts = (crow[1:] - crow[:-1]) * bw                                    # entries per element row, by block row
    ptr = torch.zeros(nrb * bh + 1, dtype=torch.int64)
    ptr[1:] = counts.repeat_interleave(bh).cumsum(0)
    blocks = _segment_ids(crow, nrb, col.numel())                           # block row of every block
    # entries of element row (I, r): for e in block row I, for c < bw -> built as (e, r, c) sorted by (I, r, e, c)
    e = torch.arange(col.numel())
    first = crow[blocks]                                                    # first block of e's block row
    n_in_row = (crow[1:] - crow[:-1])[blocks]
    r = torch.arange(bh).view(1, bh, 1)
    c = torch.arange(bw).view(1, 1, bw)
    # position of entry (e, r, c) in the walk: start of block row + r·(blocks in row)·bw + (e − first)·bw + c
    start = ptr[:-1][blocks * bh].view(-1, 1, 1)
    pos = start + r * (n_in_row * bw).view(-1, 1, 1) + ((e - first) * bw).view(-1, 1, 1) + c
    idx = torch.empty(col.numel() * bh * bw, dtype=torch.int64)
    perm = torch.empty_like(idx)
    idx[pos.reshape(-1)] = (col.view(-1, 1, 1) * bw + c).expand(-1, bh, -1).reshape(-1)
    perm[pos.reshape(-1)] = (e.view(-1, 1, 1) * (bh * bw) + r * bw + c).reshape(-1)
    return ptr, idx, perm


def bsr_attention(plan: _pt.RowGather, bias, bh: int, bw: int, Q, K, V, heads: int, scale: float):
    """(O, (the element walk, P)) of block-sparse attention by :func:`attention` over the element pattern the blocks cover."""
    walk = bsr_element_walk(plan, bh, bw)
    O, P = attention(*walk, None if bias is None else bias.reshape(-1), Q, K, V, heads, scale)
    return O, walk, P


def bsr_attention_backward(walk, bh: int, bw: int, Q, K, V, dO, P, heads: int, scale: float, want_dA: bool):
    """(dQ, dK, dV, dA [nnzb, bh, bw] or None) by :func:`attention_backward`; dA folded back into the blocks (perm)."""
    dQ, dK, dV, dA = attention_backward(*walk, Q, K, V, dO, P, heads, scale, want_dA)
    return dQ, dK, dV, (dA.view(-1, bh, bw) if want_dA else None)


def csr_factor(kind: str, crow: torch.Tensor, col: torch.Tensor, diag_pos: torch.Tensor, val: torch.Tensor, n: int, shift: float = 0.0):
    """ILU(0) (``kind = "ilu0"``, the combined L \\ U array) or IC(0) (``"ic0"``, on the arrays of tril(A)) of a CSR matrix with
    ascending, unique columns and a stored diagonal per row (include/tsgu_hip_factor.h has the recurrences): a plain row-by-row
    loop in the value type.  Reference speed only — one Python iteration per stored lower entry; it exists so that CPU operands
    have the semantics of the kernels (the ILU(0) bits included), not to be fast.  Returns (out, info) like `_backend.csr_factor`."""
    import numpy as np

    _cpu_only(crow, col, diag_pos, val)
    ptr, idx, dpos = crow.numpy().astype(np.int64), col.numpy().astype(np.int64), diag_pos.numpy().astype(np.int64)
    a = val.detach().numpy()
    dt = a.dtype.type
    out = np.empty_like(a)
    scale = dt(1.0 + shift)
    bad = 0
    with np.errstate(all="ignore"):
        for i in range(n):
            s, e, d = ptr[i], ptr[i + 1], dpos[i]
            cols = idx[s:e]
            w = a[s:e].copy()
            w[d - s] = w[d - s] * scale
            for q in range(d - s):
                k = cols[q]
                sk, ek, dk = ptr[k], ptr[k + 1], dpos[k]
                if kind == "ilu0":
                    w[q] = w[q] / out[dk]
                    js, us = idx[dk + 1:ek], out[dk + 1:ek]
                    m = np.searchsorted(cols, js)
                    hit = (m < cols.size) & (cols[np.minimum(m, cols.size - 1)] == js)
                    w[m[hit]] = w[m[hit]] - w[q] * us[hit]
                else:
                    js, ls = idx[sk:dk], out[sk:dk]
                    m = np.searchsorted(cols[:q], js)
                    hit = (m < q) & (cols[np.minimum(m, max(q - 1, 0))] == js)
                    w[q] = (w[q] - np.sum(w[m[hit]] * ls[hit], dtype=a.dtype)) / out[dk]
            if kind == "ilu0":
                broke = w[d - s] == 0
            else:
                rad = w[d - s] - np.sum(w[:d - s] * w[:d - s], dtype=a.dtype)
                broke = not rad > 0
                w[d - s] = np.sqrt(rad)
            if broke and not bad:
                bad = i + 1
            out[s:e] = w
    return torch.from_numpy(out), torch.tensor(bad, dtype=torch.int64)


def csr_fsai(a_crow: torch.Tensor, a_col: torch.Tensor, a_val: torch.Tensor, s_crow: torch.Tensor, s_col: torch.Tensor, n: int):
    """The FSAI factor G on the lower pattern (s_crow, s_col) for the CSR of tril(A) (include/tsgu_hip_fsai.h has the semantics;
    both patterns with ascending, unique columns and the diagonal last): a plain loop over the rows, one dense Cholesky
    factorisation and one triangular solve each, in the value type.  Reference speed only.  A row whose local matrix is not
    positive definite is filled with NaN.  Returns (out, info) like `_backend.csr_fsai`."""
    import numpy as np

    _cpu_only(a_crow, a_col, a_val, s_crow, s_col)
    aptr, aidx = a_crow.numpy().astype(np.int64), a_col.numpy().astype(np.int64)
    sptr, sidx = s_crow.numpy().astype(np.int64), s_col.numpy().astype(np.int64)
    a = a_val.detach().numpy()
    out = np.empty(sidx.size, dtype=a.dtype)
    bad = 0
    for i in range(n):
        J = sidx[sptr[i]:sptr[i + 1]]
        m = J.size
        M = np.zeros((m, m), dtype=a.dtype)
        for t in range(m):                           # row j_t of tril(A) against J[0 … t]
            s, e = aptr[J[t]], aptr[J[t] + 1]
            cols = aidx[s:e]
            b = np.searchsorted(J[:t + 1], cols)
            hit = (b <= t) & (J[np.minimum(b, t)] == cols)
            M[t, b[hit]] = a[s:e][hit]
        M = M + np.tril(M, -1).T
        rhs = np.zeros(m, dtype=a.dtype)
        rhs[m - 1:] = 1
        try:
            if not np.all(np.isfinite(M)):
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky(M)
            g = np.linalg.solve(L.T, rhs)            # = y / sqrt(y_m) of A[J,J]·y = e_m
        except np.linalg.LinAlgError:
            g = np.full(m, np.nan, dtype=a.dtype)
            bad = bad or i + 1
        out[sptr[i]:sptr[i + 1]] = g
    return torch.from_numpy(out), torch.tensor(bad, dtype=torch.int64)


# ---- the three primitives of the LOBPCG loop (utils/lobpcg.py): csrc/tsgu_hip_lobpcg.h in torch ops -------------------------------

def tall_gram(Y: torch.Tensor, Z: torch.Tensor, out=None, workspace=None, workgroups: int = 0) -> torch.Tensor:
    """YᵀZ for (n, a) and (n, b) views."""
    _cpu_only(Y, Z, out)
    return torch.matmul(Y.t(), Z) if out is None else torch.matmul(Y.t(), Z, out=out)


def _views_meet(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Do two row-major (n, w) views share an element?  The kernel's rule (csrc/lobpcg_impl.h, tall_views_meet): views that
    interleave in one allocation (equal row strides, disjoint column windows) do not, any other overlap of the address ranges does."""
    size = a.element_size()
    lda, ldb = (t.stride(0) if t.size(0) > 1 else t.size(1) for t in (a, b))
    a0, b0 = a.data_ptr(), b.data_ptr()
    a1, b1 = a0 + ((a.size(0) - 1) * lda + a.size(1)) * size, b0 + ((b.size(0) - 1) * ldb + b.size(1)) * size
    if a1 <= b0 or b1 <= a0:
        return False
    if lda != ldb or (b0 - a0) % size:
        return True
    d = ((b0 - a0) // size) % lda
    return not (d >= a.size(1) and d + b.size(1) <= lda)


def tall_combine(inputs, outputs, coefs, betas=None, workgroups: int = 0):
    """outputs[t] = betas[t]·outputs[t] + Σ_i inputs[i] @ coefs[t][i]; a None coefficient does not contribute.  The same refusal
    as the kernel's: an output shares no element with an input or with another output."""
    _cpu_only(*inputs, *outputs)
    for t, o in enumerate(outputs):
        if any(_views_meet(o, s) for s in inputs) or any(_views_meet(o, q) for q in outputs[:t]):
            raise RuntimeError("tall_combine: an output may share no element with an input or another output")
    for t, out in enumerate(outputs):
        beta = 0.0 if betas is None else float(betas[t])
        acc = out * beta if beta != 0.0 else torch.zeros_like(out)
        for s, c in zip(inputs, coefs[t]):
            if c is not None:
                acc = acc + s @ c
        out.copy_(acc)
    return outputs


def lobpcg_residual(AX: torch.Tensor, X: torch.Tensor, lam: torch.Tensor, out=None, workspace=None, workgroups: int = 0):
    """(R = AX − X·diag(lam), the column sums of squares of R)."""
    _cpu_only(AX, X, lam, out)
    R = AX - X * lam
    if out is not None:
        R = out.copy_(R)
    return R, (R * R).sum(dim=0)


# ---- the primitives of the aggregation multigrid (sparse_amg.py): csrc/tsgu_hip_amg.h in torch ops --------------------------------

_SIGN = -(1 << 63)       # x ^ _SIGN maps the unsigned order of 64-bit words onto the signed order of int64


def _rows_of(ptr: torch.Tensor, nnz: int) -> torch.Tensor:
    n = ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(n, dtype=torch.int64), (ptr[1:] - ptr[:-1]).to(torch.int64), output_size=nnz)


def amg_hop(ptr: torch.Tensor, idx: torch.Tensor, keys: torch.Tensor, n: int, group: int = 8, out=None) -> torch.Tensor:
    """out[i] = max(keys[i], max of keys[j] over the stored entries (i, j)) in unsigned 64-bit order (the bits travel as int64)."""
    _cpu_only(ptr, idx, keys, out)
    s = keys ^ _SIGN
    far = s.scatter_reduce(0, _rows_of(ptr, idx.numel()), s.index_select(0, idx.to(torch.int64)), "amax", include_self=True) ^ _SIGN
    return far if out is None else out.copy_(far)


def _lowbias32(x: torch.Tensor) -> torch.Tensor:
    """lowbias32 of the low words of an int64 tensor, in 32-bit arithmetic."""
    m = 0xFFFFFFFF
    x = x & m
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m
    return x ^ (x >> 16)


def amg_mis2_update(mode: int, n: int, key=None, t=None, out=None, undecided=None, device=None) -> torch.Tensor:
    """One node-wise step of the MIS-2 aggregation, as `_backend.amg_mis2_update` (mode 0: initial keys, 1: a round, 2: root keys)."""
    _cpu_only(key, t, out, undecided)
    low = (1 << 62) - 1
    if mode == 0:
        i = torch.arange(n, dtype=torch.int64)
        nxt = (1 << 62) | ((_lowbias32(i) >> 2) << 32) | i
    elif mode == 2:
        nxt = torch.where((key >> 62) == -2, key, torch.zeros_like(key))
    else:
        und = (key >> 62) == 1
        root = und & ((t & 0xFFFFFFFF) == torch.arange(n, dtype=torch.int64))
        gone = und & ~root & ((t >> 62) == -2)
        nxt = torch.where(root, (key & low) | _SIGN, torch.where(gone, key & low, key))
        if undecided is not None:
            undecided.fill_(int(bool((und & ~root & ~gone).any())))
    return nxt if out is None else out.copy_(nxt)


def csr_affine_spmm(ptr, idx, val, X, n_rows: int, n_cols: int, C=None, B=None, w=None, alpha: float = 1.0, out=None) -> torch.Tensor:
    """out = C + alpha·w∘(B − A·X) for the CSR matrix (ptr, idx, val) and X (n_cols, p); None stands for 0, 0 and 1.  A row is summed
    in entry order (``index_add_``), the epilogue in the kernel's order of operations."""
    _cpu_only(ptr, idx, val, X, C, B, w, out)
    ax = torch.zeros((n_rows, X.size(1)), dtype=val.dtype)
    ax.index_add_(0, _rows_of(ptr, idx.numel()), val.unsqueeze(1) * X.index_select(0, idx.to(torch.int64)))
    r = (B - ax) if B is not None else -ax
    if w is not None:
        r = w.unsqueeze(1) * r
    r = alpha * r
    if C is not None:
        r = C + r
    return r if out is None else out.copy_(r)


# ---- the primitives of the multicolour ordering (sparse_coloring.py): csrc/tsgu_hip_color.h in torch ops --------------------------

def _color_edges(ptr, idx, tptr, tidx, n: int):
    """(u, v) int64: every stored entry (u, v) of A and, when given, of Aᵀ, without the diagonal and the columns outside the matrix."""
    u, v = _rows_of(ptr, idx.numel()), idx.to(torch.int64)
    if tptr is not None:
        u, v = torch.cat((u, _rows_of(tptr, tidx.numel()))), torch.cat((v, tidx.to(torch.int64)))
    else:
        u, v = torch.cat((u, v)), torch.cat((v, u))
    keep = (u != v) & (v >= 0) & (v < n) & (u >= 0) & (u < n)
    return u[keep], v[keep]


def color_greedy(ptr, idx, tptr, tidx, n: int) -> torch.Tensor:
    """The colouring of csrc/tsgu_hip_color.h by its own rounds: an uncoloured node with no uncoloured neighbour of greater key
    (lowbias32(i), i) takes the smallest colour no neighbour holds.  int32 colours; reference speed only."""
    _cpu_only(ptr, idx, tptr, tidx)
    u, v = _color_edges(ptr, idx, tptr, tidx, n)
    ar = torch.arange(n, dtype=torch.int64)
    key = _lowbias32(ar) * (1 << 31) + ar
    up = key[v] > key[u]
    colors = torch.full((n,), -1, dtype=torch.int64)
    for _ in range(n + 1):
        unc = colors < 0
        if not bool(unc.any()):
            break
        blocked = torch.zeros(n, dtype=torch.bool)
        blocked[u[up & unc[v]]] = True
        ready = unc & ~blocked
        live = ready[u] & (colors[v] >= 0)
        lu, lc = u[live], colors[v[live]]
        cand = torch.zeros(n, dtype=torch.int64)
        while True:
            hit = lu[lc == cand[lu]]
            if hit.numel() == 0:
                break
            cand[torch.unique(hit)] += 1
        colors = torch.where(ready, cand, colors)
    return colors.to(torch.int32)


def color_check(ptr, idx, tptr, tidx, colors, n: int, n_colors: int) -> torch.Tensor:
    """An int64 scalar: 0 for a colouring with `n_colors` colours, else 1 + the lowest row whose colour is outside [0, n_colors) or
    held by a neighbour."""
    _cpu_only(ptr, idx, tptr, tidx, colors)
    u, v = _color_edges(ptr, idx, tptr, tidx, n)
    c = colors.to(torch.int64)
    bad = (c < 0) | (c >= n_colors)
    bad[u[c[u] == c[v]]] = True
    rows = torch.nonzero(bad).reshape(-1)
    return rows[:1].sum() + 1 if rows.numel() else torch.zeros((), dtype=torch.int64)


def csr_color_sweep(mode: int, begin, end, idx, diag, val, B, X, row0: int, row1: int, vmap=None, bmap=None, out=None, out_rows=None,
                    group: int = 8) -> torch.Tensor:
    """The rows [row0, row1) of one colour class of a triangular sweep, in place in X, as `_backend.csr_color_sweep`; a row is
    summed in entry order (``index_add_``) in the value type."""
    _cpu_only(begin, end, idx, diag, val, B, X, vmap, bmap, out, out_rows)
    if row1 <= row0:
        return X
    rows = torch.arange(row0, row1, dtype=torch.int64)
    s, e = begin[row0:row1].to(torch.int64), end[row0:row1].to(torch.int64)
    lens = (e - s).clamp_(min=0)
    total = int(lens.sum())
    local = torch.repeat_interleave(torch.arange(row1 - row0, dtype=torch.int64), lens, output_size=total)
    ent = s[local] + (torch.arange(total, dtype=torch.int64) - (torch.cumsum(lens, 0) - lens)[local])
    q = ent if vmap is None else vmap.to(torch.int64)[ent]
    acc = torch.zeros((row1 - row0, X.size(1)), dtype=val.dtype)
    acc.index_add_(0, local, val[q].unsqueeze(1) * X[idx.to(torch.int64)[ent]])
    rhs = B[rows if bmap is None else bmap.to(torch.int64)[rows]]
    if mode == 1:
        r = rhs - acc
    else:
        dq = diag.to(torch.int64)[rows]
        d = val[dq if vmap is None else vmap.to(torch.int64)[dq]].unsqueeze(1)
        r = (rhs - acc) / d if mode == 0 else rhs - acc / d
    X[rows] = r
    if out is not None:
        out[rows if out_rows is None else out_rows.to(torch.int64)[rows]] = r
    return X


def csr_color_sweeps(mode: int, begin, end, idx, diag, val, B, X, classes, vmap=None, bmap=None, out=None, out_rows=None, group: int = 8):
    """One triangular sweep by colour classes, as `_backend.csr_color_sweeps`."""
    for row0, row1 in classes:
        csr_color_sweep(mode, begin, end, idx, diag, val, B, X, row0, row1, vmap=vmap, bmap=bmap, out=out, out_rows=out_rows)
    return X


# ---- Lanczos quadrature (sparse_logdet.py): csrc/tsgu_hip_quadrature.h in torch ops ------------------------------------------------

def rademacher_fill(n: int, p: int, seed: int, dtype: torch.dtype) -> torch.Tensor:
    """The (n, p) block of ±1 of tsgu_rademacher_fill, bit for bit: the sign bit of lowbias32(c + lowbias32(i + s)) with
    s = lowbias32(lo32(seed) ^ lowbias32(hi32(seed))) and sums modulo 2^32."""
    m = 0xFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s = _lowbias32(torch.tensor(seed & m, dtype=torch.int64) ^ _lowbias32(torch.tensor(seed >> 32, dtype=torch.int64)))
    rows = _lowbias32((torch.arange(n, dtype=torch.int64) + s) & m)
    h = _lowbias32((torch.arange(p, dtype=torch.int64).unsqueeze(0) + rows.unsqueeze(1)) & m)
    return torch.where((h >> 31) != 0, -1.0, 1.0).to(dtype)


def cg_history_loop(matmul, dot, rhs: torch.Tensor, n_hist: int, tolerance: float, max_iter: int, eps: float, stop_after: float):
    """Conjugate gradients from x = 0 on the normalised columns `rhs` (n, p) with every column's coefficients kept:
    (x, hist [n_hist][2][p] of (alpha, beta), iterations, residual norms (p,), tolerance reached).  The recurrences, guards and the
    stop rule are those of `linear_cg._two_launch_loop` (alpha = 0 for a column whose residual fell below `stop_after` or whose
    p'Ap is below `eps`; the mean residual norm is tested from iteration max(min(10, max_iter - 1), min(n_hist, max_iter - 1)) on),
    written in torch ops around the closures `matmul` (v -> A v) and `dot` (column-wise dot products): CPU operands, and the GPU
    solves the fused loop declines."""
    p = rhs.size(1)
    x = torch.zeros_like(rhs)
    r = rhs.clone()
    pv = r.clone()
    rr = dot(r, r)
    hist = torch.zeros((n_hist, 2, p), dtype=rhs.dtype, device=rhs.device)
    rnorm = rr.sqrt()
    frozen = rnorm < stop_after
    floor = max(min(10, max_iter - 1), min(n_hist, max_iter - 1))
    one, zero = torch.ones_like(rr), torch.zeros_like(rr)
    iters, done = 0, False
    for k in range(max_iter):
        Ap = matmul(pv)
        pap = dot(pv, Ap)
        ok = (pap >= eps) & ~frozen
        alpha = torch.where(ok, rr / torch.where(ok, pap, one), zero)
        x = torch.addcmul(x, alpha.unsqueeze(0), pv)
        r = torch.addcmul(r, alpha.unsqueeze(0), Ap, value=-1)
        rr_new = dot(r, r)
        ok = rr >= eps
        beta = torch.where(ok, rr_new / torch.where(ok, rr, one), zero)
        if k < n_hist:
            hist[k, 0], hist[k, 1] = alpha, beta
        pv = torch.addcmul(r, beta.unsqueeze(0), pv)
        rr = rr_new
        rnorm = rr.sqrt()
        frozen = rnorm < stop_after
        iters = k + 1
        if k >= floor and bool(rnorm.mean() < tolerance):
            done = True
            break
    return x, hist, iters, rnorm, done


def tridiag_quadrature(coef: torch.Tensor, kind: int = 0, fn: int = 0, scale=None, p: int = None):
    """(out, info) of tsgu_tridiag_quadrature in torch ops: the same entries, the same per-column length rule, `torch.linalg.eigh`
    in float64.  out in coef's dtype, info int32."""
    _cpu_only(coef, scale)
    r, width = coef.size(0), coef.size(2)
    p = width if p is None else int(p)
    c64 = coef[:, :, :p].to(torch.float64)
    out = torch.zeros(p, dtype=torch.float64)
    info = torch.zeros(p, dtype=torch.int32)
    for c in range(p):
        a, b = c64[:, 0, c], c64[:, 1, c]
        if kind == 0:
            bad_a = ~((a > 0) & torch.isfinite(a))
            bad_b = ~((b > 0) & torch.isfinite(b))
            n = int(bad_a.nonzero()[0]) if bool(bad_a.any()) else r
            if bool(bad_b[:n].any()):
                n = min(n, int(bad_b.nonzero()[0]) + 1)
            ia = 1.0 / a[:n]
            d = ia.clone()
            d[1:] += (b[:n] * ia)[:-1]
            e = (b[:n].sqrt() * ia)[:-1]
        else:
            bad_b = (b == 0) | ~torch.isfinite(b)
            n = int(bad_b.nonzero()[0]) + 1 if bool(bad_b.any()) else r
            d, e = a[:n], b[: n - 1]
        if n == 0:
            continue
        lam, vec = torch.linalg.eigh(torch.diag(d) + torch.diag(e, 1) + torch.diag(e, -1))
        w = vec[0] ** 2
        f = (lam.log(), lam.reciprocal(), lam, torch.ones_like(lam))[fn]
        bad = fn <= 1 and bool((lam <= 0).any())
        out[c] = float("nan") if bad else (w * f).sum()
        info[c] = -n if bad else n
    if scale is not None:
        out = out * scale.to(torch.float64)
    return out.to(coef.dtype), info


# ---- contour quadrature (sparse_sqrt.py): the composition the fused loop of csrc/ciq_impl.h replaces ---------------------------------

def ciq_apply(A: torch.Tensor, B: torch.Tensor, sigma: torch.Tensor, omega: torch.Tensor, tolerance: float, max_iter: int, want_keep: bool):
    """Σ_q ω_q (A + σ_q I)⁻¹ B for the dense (n, p) block B: the unfused multi-shift `minres(A, B, shifts=σ)` and the weighted sum.
    Returns (result, keep, est): `keep` [n][S][p] holds the S solutions as an SDDMM operand (None unless `want_keep`), `est` (p,)
    each column's largest TRUE relative residual over the shifts (the unfused solver keeps no estimates; a zero column reports 0)."""
    from .utils._operator import SparseOperator
    from .utils.minres import MINRESSettings, minres

    _cpu_only(B, sigma, omega)
    n, p = B.shape
    S = sigma.numel()
    sols = minres(A, B, shifts=sigma, max_iter=int(max_iter),
                  settings=MINRESSettings(max_cg_iterations=int(max_iter), minres_tolerance=float(tolerance))).reshape(S, n, p)
    out = torch.einsum("q,qnc->nc", omega, sols)
    keep = sols.permute(1, 0, 2).contiguous()
    resid = SparseOperator(A)(keep.reshape(n, S * p)).reshape(n, S, p) + sigma.reshape(1, S, 1) * keep - B.unsqueeze(1)
    bnorm = torch.linalg.vector_norm(B, dim=0)
    est = torch.linalg.vector_norm(resid, dim=0).amax(dim=0) / torch.where(bnorm > 0, bnorm, torch.ones_like(bnorm))
    return out, (keep if want_keep else None), est


# ---- Chebyshev expansion of exp(t A) B (sparse_expm.py): the composition the fused loop of csrc/expm_impl.h replaces --------------------

def expm_apply(matmul, B: torch.Tensor, coef: torch.Tensor, a: float, b: float, want_keep: bool):
    """Σ_k coef[k] ∘ w_k for the dense (n, p) block B with w_0 = B, w_1 = Â w_0, w_{k+1} = 2 Â w_k − w_{k−1}, Â = a·A + b·I, in torch
    ops around the closure `matmul` (v -> A v): CPU operands, and the baseline tools/expmbench.py times on the GPU.  `coef` is the
    (K + 1, T, p) table of sparse_expm._coefficients in B's dtype.  Returns (Y (T, n, p), [w_0 ... w_K] or None)."""
    K = coef.size(0) - 1
    w_prev, w = None, B
    Y = coef[0].unsqueeze(1) * w.unsqueeze(0)
    W = [w] if want_keep else None
    for k in range(K):
        f = 1.0 if k == 0 else 2.0
        nxt = torch.add(matmul(w).mul_(f * a), w, alpha=f * b)
        if w_prev is not None:
            nxt.sub_(w_prev)
        w_prev, w = w, nxt
        Y.addcmul_(coef[k + 1].unsqueeze(1), w.unsqueeze(0))
        if want_keep:
            W.append(w)
    return Y, W


def expm_adjoint(matmul, sddmm, G: torch.Tensor, coef: torch.Tensor, a: float, b: float, W, need_b: bool = True):
    """The adjoint of :func:`expm_apply` for G (T, n, p): μ_k = Σ_j coef[k, j] ∘ G_j + f_k Â μ_{k+1} − μ_{k+2} for k = K ... 0 with
    f_0 = 1, f_k = 2.  Returns (a Σ_{k<K} f_k sddmm(μ_{k+1}, w_k) or None without `W`, μ_0 or None): `sddmm(L, R)` gives
    Σ_c L[i, c] R[j, c] at the stored entries (i, j)."""
    K = coef.size(0) - 1
    mu1 = mu2 = None                                              # μ_{k+1}, μ_{k+2}; None stands for zero
    gvals = None
    for k in range(K, -1, -1):
        if k == 0 and not need_b:
            break
        f = 1.0 if k == 0 else 2.0
        mu = (coef[k].unsqueeze(1) * G).sum(dim=0)
        if mu1 is not None:
            mu.add_(matmul(mu1), alpha=f * a).add_(mu1, alpha=f * b)
        if mu2 is not None:
            mu.sub_(mu2)
        mu2, mu1 = mu1, mu
        if W is not None and k >= 1:                              # μ_k pairs with w_{k−1}, weighted f_{k−1}·a
            part = sddmm(mu1, W[k - 1])
            fk = a if k == 1 else 2.0 * a
            gvals = part.mul_(fk) if gvals is None else gvals.add_(part, alpha=fk)
    return gvals, (mu1 if need_b else None)


# ---- the k largest of a dense product per row (sparse_topk.py): the composition the fused kernel of csrc/topk_impl.h replaces -----------

def topk_mm(Q: torch.Tensor, K: torch.Tensor, bias, k: int, scale: float, causal: bool, exclude_self: bool, counts: torch.Tensor,
            index_dtype):
    """(col (b, nnz), val (b, nnz)) of the best `counts[i]` allowed scores of every row of scale·Q·Kᵀ + bias for Q (b, n, d), K (b, m, d)
    and bias (b, m) or None: the dense product in float32 (float64 for float64), a stable descending sort (NaN first, the lower
    column first among equal scores), the allowed columns moved to the front by a second stable sort, columns ascending at the end."""
    _cpu_only(Q, K, bias)
    b, n, _ = Q.shape
    m = K.size(1)
    acc = torch.float64 if Q.dtype == torch.float64 else torch.float32
    S = torch.matmul(Q.to(acc), K.to(acc).transpose(1, 2))
    if scale != 1.0:
        S = S * scale
    if bias is not None:
        S = S + bias.to(acc).unsqueeze(1)
    i = torch.arange(n).unsqueeze(1)
    j = torch.arange(m).unsqueeze(0)
    allowed = torch.ones((n, m), dtype=torch.bool)
    if causal:
        allowed &= j <= i + (m - n)
    if exclude_self:
        allowed &= j != i
    order = torch.sort(S, dim=-1, descending=True, stable=True).indices
    barred = (~allowed).expand(b, n, m).gather(2, order)
    order = order.gather(2, torch.sort(barred.to(torch.uint8), dim=-1, stable=True).indices)
    kk = min(k, m)
    keep = torch.arange(kk).unsqueeze(0) < counts.unsqueeze(1)                 # (n, kk): a row's first counts[i] places
    cols = torch.where(keep, order[:, :, :kk], torch.full((), m, dtype=torch.int64)).sort(dim=-1).values
    vals = S.gather(2, cols.clamp(max=max(m - 1, 0))) if m else S[:, :, :0]
    keep = keep.expand(b, n, kk)
    return cols[keep].reshape(b, -1).to(index_dtype), vals[keep].reshape(b, -1).to(Q.dtype)


# ---- 2:4 semi-structured operands (sparse_semi_structured.py): what the kernels of csrc/semi_impl.h compute, in torch ops ---------------

def semi_prune(W: torch.Tensor):
    """(values (m, k / 2), positions (m, k / 4, 2) int64, ascending) of the dense (m, k) matrix W: per aligned group of four the two
    entries that rank first by (|w| descending, column ascending).  A stable descending sort of |w|: torch sorts NaN above inf, and
    -0 equals +0 once the sign is gone."""
    _cpu_only(W)
    m, k = W.shape
    groups = W.reshape(m, k // 4, 4)
    order = torch.sort(groups.abs(), dim=-1, descending=True, stable=True).indices
    pos = order[..., :2].sort(dim=-1).values
    return groups.gather(-1, pos).reshape(m, k // 2), pos


def semi_dense(values: torch.Tensor, cols: torch.Tensor, k: int, dtype=None) -> torch.Tensor:
    """The dense (m, k) matrix with `values` at the columns `cols` (both (m, k / 2)), +0 elsewhere."""
    _cpu_only(values, cols)
    out = torch.zeros((values.size(0), k), dtype=dtype or values.dtype)
    return out.scatter_(1, cols, values.to(out.dtype))


def semi_mm(values: torch.Tensor, cols: torch.Tensor, k: int, Y: torch.Tensor, bias, linear: bool) -> torch.Tensor:
    """A·Y for Y (k, p), or with `linear` Y·Aᵀ (+ bias) for Y (p, k): accumulated in float32 for float32 and bfloat16 (float64 for
    float64), rounded once."""
    _cpu_only(values, cols, Y, bias)
    acc = _bsr_acc(values.dtype)
    A = semi_dense(values, cols, k, acc)
    if not linear:
        return (A @ Y.to(acc)).to(values.dtype)
    out = Y.to(acc) @ A.t()
    if bias is not None:
        out = out + bias.to(acc)
    return out.to(values.dtype)


def semi_mm_backward(values, cols, k: int, Y, G, linear: bool, need_values: bool, need_dense: bool):
    """(gradient of the kept values or None, gradient of the dense operand or None) of :func:`semi_mm`: the dense product G·Yᵀ read at
    the kept columns, and Aᵀ·G."""
    _cpu_only(values, cols, Y, G)
    acc = _bsr_acc(values.dtype)
    Ga, Ya = G.to(acc), Y.to(acc)
    dvalues = ddense = None
    if need_values:
        full = Ga.t() @ Ya if linear else Ga @ Ya.t()                   # (m, k)
        dvalues = full.gather(1, cols).to(values.dtype)
    if need_dense:
        A = semi_dense(values, cols, k, acc)
        ddense = (Ga @ A if linear else A.t() @ Ga).to(values.dtype)
    return dvalues, ddense


# ---- sparse_sinkhorn (sparse_sinkhorn.py): a direction is (ptr, perm, idx, grp, n groups, ...) ------------------------------------
def _sk_at(d, v: torch.Tensor) -> torch.Tensor:
    """The values in the direction's walking order."""
    return v if d.perm is None else v.index_select(0, d.perm.to(torch.int64))


def _sk_half(d, v: torch.Tensor, other: torch.Tensor, log_marg) -> torch.Tensor:
    """log_marg − LSE over the direction's groups of (value + the other side's potential); an empty group gives +inf."""
    x = _sk_at(d, v)
    # (a stored −inf is an absent entry, also beside the +inf potential of a group that holds nothing else)
    x = torch.where(x == float("-inf"), x, x + other[d.idx.to(torch.int64)])
    lse = segment_logsumexp(d.ptr, None, x, d.n, False, 0)
    return -lse if log_marg is None else log_marg - lse


def _sk_potential(log_marg, neg_lse: torch.Tensor) -> torch.Tensor:
    """The potential of a half step from what it keeps: log_marg − lse (the same rounding as the subtraction)."""
    return neg_lse if log_marg is None else log_marg + neg_lse


def sinkhorn_forward(rowd, cold, val: torch.Tensor, log_a, log_b, T: int, keep: bool):
    """(NU, NV, u^T, v^T) of the T iterations from v⁰ = 0: NU[t − 1] = −LSE_row(S + v^{t−1}) and NV[t − 1] = −LSE_col(S + u^t), the
    potentials less their log marginals, when `keep` (else None).  Accumulator precision (float32 for bfloat16 values)."""
    _cpu_only(val, log_a, log_b)
    acc = torch.float32 if val.dtype == torch.bfloat16 else val.dtype
    x = val.reshape(-1).to(acc)
    NU = torch.empty((T, rowd.n), dtype=acc) if keep else None
    NV = torch.empty((T, cold.n), dtype=acc) if keep else None
    v = torch.zeros(cold.n, dtype=acc)
    for t in range(T):
        nu = _sk_half(rowd, x, v, None)
        u = _sk_potential(log_a, nu)
        nv = _sk_half(cold, x, u, None)
        v = _sk_potential(log_b, nv)
        if keep:
            NU[t], NV[t] = nu, nv
    return NU, NV, u, v


def sinkhorn_plan(grp: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, pot_group: torch.Tensor, pot_other: torch.Tensor) -> torch.Tensor:
    """val + pot_group[grp] + pot_other[idx] in stored order, rounded once to the values' dtype."""
    _cpu_only(val, pot_group, pot_other)
    v = val.reshape(-1).to(pot_group.dtype)
    # (a stored −inf stays −inf, also beside the +inf potential of a group that holds nothing else)
    return torch.where(v == float("-inf"), v, (v + pot_group[grp.to(torch.int64)]) + pot_other[idx.to(torch.int64)]).to(val.dtype)


def _sk_half_backward(d, v, pot_group, pot_other, log_marg_other, g_other, dS) -> torch.Tensor:
    """term = g_other[idx]·exp(value + pot_group[grp] + pot_other[idx] − log_marg_other[idx]); dS −= term at the entries' own
    positions; returns −Σ_group term.  With pot_other = −lse of the other direction's half step (and no log marginal) the argument
    is that step's own staged value less its own lse."""
    j, g = d.idx.to(torch.int64), d.grp.to(torch.int64)
    x = (_sk_at(d, v) + pot_group[g]) + pot_other[j]
    if log_marg_other is not None:
        x = x - log_marg_other[j]
    term = torch.where(_sk_at(d, v) == float("-inf"), torch.zeros_like(x), g_other[j] * x.exp())   # (a stored −inf: absent)
    if d.perm is None:
        dS -= term
    else:
        dS.index_add_(0, d.perm.to(torch.int64), term, alpha=-1)
    return torch.zeros(d.n, dtype=v.dtype).index_add_(0, g, term).neg_()


def sinkhorn_backward(rowd, cold, val, log_a, log_b, NU, NV, dS, gu, gv, T: int):
    """The reverse sweep of `sinkhorn_forward`: dS comes in as the cotangent of log_P (accumulator precision, stored order) and
    leaves as the gradient of the values; returns (dlog_a, dlog_b)."""
    _cpu_only(val, NU, NV, dS)
    v = val.reshape(-1).to(NU.dtype)
    ub = torch.zeros(rowd.n, dtype=NU.dtype).index_add_(0, rowd.grp.to(torch.int64), _sk_at(rowd, dS))
    vb = torch.zeros(cold.n, dtype=NU.dtype).index_add_(0, cold.grp.to(torch.int64), _sk_at(cold, dS))
    if gu is not None:
        ub += gu
    if gv is not None:
        vb += gv
    dla, dlb = torch.zeros_like(ub), torch.zeros_like(vb)
    for t in range(T, 0, -1):
        dlb += vb
        u_t = _sk_potential(log_a, NU[t - 1])
        v_before = _sk_potential(log_b, NV[t - 2]) if t > 1 else torch.zeros_like(vb)
        ub = _sk_half_backward(rowd, v, u_t, NV[t - 1], None, vb, dS) + (ub if t == T else 0)
        dla += ub
        vb = _sk_half_backward(cold, v, v_before, NU[t - 1], None, ub, dS)
    return dla, dlb
