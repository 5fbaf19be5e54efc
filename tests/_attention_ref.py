"""Shared by the sparse_attention tests: the dense float64 oracle, and sparse operands built from a mask and dense values.

The oracle is the dense masked computation: logits scale·<Q[i,h], K[j,h]> + bias[i,j], −inf at absent positions, torch.softmax over
each row, zero rows where nothing is stored, then P·V; its gradients come from torch autograd in float64.
"""

import torch


def sparse_from_dense(D, mask, layout, index_dtype, dtype):
    """The values D (anything outside `mask` is ignored) as a sparse tensor that stores exactly the positions of `mask`
    ([n, m], shared by the items of a batched D), explicit zeros and infinities included."""
    D = D.to(dtype)
    batched = D.dim() == 3
    if layout in ("coo", "coo_uncoalesced"):
        idx = mask.nonzero().t()
        if batched:
            b, nnz = D.size(0), idx.size(1)
            idx = torch.cat([torch.arange(b).repeat_interleave(nnz).unsqueeze(0), idx.repeat(1, b)])
            val = torch.cat([Di[mask] for Di in D])
        else:
            val = D[mask]
        if layout == "coo":
            return torch.sparse_coo_tensor(idx, val, D.shape, is_coalesced=True)
        order = torch.randperm(val.numel(), generator=torch.Generator().manual_seed(1))
        half = val[order] / 2           # every entry twice, shuffled: coalescing sums them back (exact: a power of two)
        A = torch.sparse_coo_tensor(torch.cat([idx[:, order], idx[:, order.flip(0)]], 1), torch.cat([half, half.flip(0)]), D.shape)
        assert not A.is_coalesced()
        return A
    n, m = mask.shape
    if layout == "csr":
        comp = torch.zeros(n + 1, dtype=torch.int64)
        comp[1:] = mask.sum(1).cumsum(0)
        plain = mask.nonzero()[:, 1]
        pick = (lambda Di: Di[mask])
        make = torch.sparse_csr_tensor
    else:
        comp = torch.zeros(m + 1, dtype=torch.int64)
        comp[1:] = mask.sum(0).cumsum(0)
        plain = mask.t().nonzero()[:, 1]
        pick = (lambda Di: Di.t()[mask.t()])
        make = torch.sparse_csc_tensor
    comp, plain = comp.to(index_dtype), plain.to(index_dtype)
    if batched:
        b = D.size(0)
        return make(comp.repeat(b, 1), plain.repeat(b, 1), torch.stack([pick(Di) for Di in D]), D.shape)
    return make(comp, plain, pick(D), D.shape)


def stored_order(W, A):
    """The dense W ([n, m] or [b, n, m]) at the stored positions of the sparse A, shaped like A's value array."""
    if A.layout == torch.sparse_coo:
        return W[tuple(A._indices())]
    csr = A.layout == torch.sparse_csr
    comp, plain = (A.crow_indices(), A.col_indices()) if csr else (A.ccol_indices(), A.row_indices())

    def one(c, p, Wi):
        major = torch.repeat_interleave(torch.arange(c.numel() - 1, device=c.device), (c[1:] - c[:-1]).to(torch.int64))
        return Wi[major, p.to(torch.int64)] if csr else Wi[p.to(torch.int64), major]

    if A.dim() == 2:
        return one(comp, plain, W)
    return torch.stack([one(comp[i], plain[i], W[i]) for i in range(A.size(0))])


def values_of(A):
    return A._values() if A.layout == torch.sparse_coo else A.values()


def index_tensors(A):
    if A.layout == torch.sparse_csr:
        return A.crow_indices(), A.col_indices()
    if A.layout == torch.sparse_csc:
        return A.ccol_indices(), A.row_indices()
    return (A._indices(),)


def heads_view(X, multi):
    """[..., rows, d] -> [..., rows, 1, d] for operands without a head axis."""
    return X if multi else X.unsqueeze(-2)


def dense_oracle(mask, B, Q, K, V, dO, scale, use_bias=True):
    """Float64 (O, dQ, dK, dV, dB, P) of the dense masked computation.  mask: bool [n, m] (shared by batch items); B: the bias
    [.., n, m]; Q, dO: [.., n, H, d]; K, V: [.., m, H, d].  dB is dense (meaningful at the stored positions); P is [.., H, n, m]."""
    Q, K, V, B = (x.detach().double().requires_grad_(True) for x in (Q, K, V, B))
    logits = torch.einsum("...ihd,...jhd->...hij", Q, K) * scale
    if use_bias:
        logits = logits + B.unsqueeze(-3)
    has = mask.any(1).view(-1, 1)
    logits = logits.masked_fill(~mask, float("-inf")).masked_fill(~has, 0.0)
    P = torch.softmax(logits, -1) * has
    O = torch.einsum("...hij,...jhd->...ihd", P, V)
    dQ, dK, dV, dB = torch.autograd.grad(O, (Q, K, V, B), dO.double(), allow_unused=True)
    return O.detach(), dQ, dK, dV, dB, P.detach()


@torch.no_grad()
def error_bounds(mask, B, Q, K, V, dO, scale, use_bias, u, tiny, P, O):
    """First-order bounds on |computed − exact| of (O, dQ, dK, dV, dA) and max ρ, for one item (Q, dO: [n, H, d]; K, V: [m, H, d];
    B, mask: [n, m]; P: [H, n, m] and O: [n, H, d] from :func:`dense_oracle`) in an arithmetic of unit roundoff `u` whose exp
    loses at most `tiny` absolutely when it underflows.  Per row i and head, L the row's length, L'_j the column's:

      a_j = |scale| Σ_c |q_c||k_jc| + |b_j|          e_j = (d + 2) u a_j          (the logit: a dot of d terms, scale, bias)
      ρ_j = e_j + Σ_l p_l e_l + (3L + |t_j − max t| + C) u                        (relative error of p_j; C = 8, 16 for gradients)
      |O_c − ·|  <= Σ_j p_j ρ_j |v_jc| + tiny Σ_j |v_jc|
      dP̄_j = Σ_c |dO_c||v_jc|      δ̄ = Σ_j p_j dP̄_j + d u Σ_c |dO_c||O_c|      dS̄_j = p_j (dP̄_j + δ̄)
      |dQ − ·|   <= |scale| Σ_j (ρ_j + d u) dS̄_j |k_j|
      |dK_j − ·| <= |scale| Σ_i (ρ_ij + (L'_j + d) u) dS̄_ij |q_i|
      |dV_j − ·| <= Σ_i (ρ_ij + L'_j u) p_ij |dO_i|
      |dA_ij − ·| <= Σ_h (ρ + H u) dS̄_ij,h
    The gradient bounds carry the forward's underflow term too — what exp(t − lse) can lose absolutely, tiny per stored entry,
    without a relative factor: δ̄' = tiny Σ_j dP̄_j, dS̄'_j = p_j δ̄' + tiny (dP̄_j + δ̄ + δ̄') beside every dS̄_j, tiny beside p_ij in dV."""
    Q, K, V, dO, B, O = (x.double() for x in (Q, K, V, dO, B, O))
    n, H, d = Q.shape
    M = mask.unsqueeze(0).double()
    s = abs(scale)
    t = torch.einsum("ihd,jhd->hij", Q, K) * scale + (B.unsqueeze(0) if use_bias else 0.0)
    a = s * torch.einsum("ihd,jhd->hij", Q.abs(), K.abs()) + (B.abs().unsqueeze(0) if use_bias else 0.0)
    a = torch.where(mask.unsqueeze(0), a, torch.zeros_like(a))              # (absent positions may hold anything, inf included)
    tm = t.masked_fill(~mask, float("-inf"))
    top = tm.amax(-1, keepdim=True)
    dist = torch.where(mask.unsqueeze(0) & tm.isfinite(), (tm - top).abs(), torch.zeros_like(tm)).nan_to_num(0.0, 0.0, 0.0)
    L = mask.sum(1).double().view(1, n, 1)
    Lc = mask.sum(0).double().view(1, 1, -1)
    e = (d + 2) * u * a
    pe = (P * e).sum(-1, keepdim=True)

    def rho(C):
        return (e + pe + (3 * L + dist + C) * u) * M

    r8, r16 = rho(8), rho(16)
    Va, Ka, Qa, Ga = V.abs(), K.abs(), Q.abs(), dO.abs()
    bO = torch.einsum("hij,jhd->ihd", P * r8, Va) + tiny * torch.einsum("hij,jhd->ihd", M.expand(H, -1, -1), Va)
    dPb = torch.einsum("ihd,jhd->hij", Ga, Va)
    tail = d * u * (Ga * O.abs()).sum(-1).t().unsqueeze(-1)                  # [H, n, 1]

    db = (P * dPb).sum(-1, keepdim=True) + tail
    db_under = tiny * (dPb * M).sum(-1, keepdim=True)
    dSb = P * (dPb + db)
    dSb_under = P * db_under + tiny * M * (dPb + db + db_under)
    bQ = s * torch.einsum("hij,jhd->ihd", (r16 + d * u) * dSb + dSb_under, Ka)
    bK = s * torch.einsum("hij,ihd->jhd", (r16 + (Lc + d) * u) * dSb + dSb_under, Qa)
    bV = torch.einsum("hij,ihd->jhd", (r16 + Lc * u) * P + tiny * M, Ga)
    bA = ((r16 + H * u) * dSb + dSb_under).sum(0)
    return bO, bQ, bK, bV, bA, float(r16.max()) if r16.numel() else 0.0
