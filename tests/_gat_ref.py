"""Shared by the sparse_gat_attention / sparse_gatv2_attention tests: the dense float64 oracle of both kinds and the error bounds.

The oracle is the masked dense computation with torch.nn.functional.leaky_relu: logits lrelu(s_dst[i] + s_src[j]) ("gat") or
Σ_k att_k·lrelu(X_dst[i,k] + X_src[j,k]) ("gatv2") plus the bias, −inf at absent positions, torch.softmax over each row, zero rows
where nothing is stored, then P·messages; its gradients come from torch autograd in float64.  The logits are formed row by row (a
GATv2 row is an [m, H, d] tensor), which is the same arithmetic.

Operands `(a, b, c)`: "gat" (s_dst [n, H], s_src [m, H], V [m, H, d]); "gatv2" (X_dst [n, H, d], X_src [m, H, d], att [H, d]).
"""

import torch
import torch.nn.functional as F

from _attention_ref import index_tensors, sparse_from_dense, stored_order, values_of  # noqa: F401  (shared with the tests)
from _mm_reduce_ref import same_bits  # noqa: F401

KINDS = ("gat", "gatv2")


def grid(shape, gen, lim=4):
    """Multiples of 1/32 of magnitude below `lim`: exact in bfloat16, and so are their pairwise sums."""
    return torch.randint(-32 * lim + 1, 32 * lim, shape, generator=gen).double() / 32


def _logits(kind, a, b, c, slope):
    """(logits without the bias, their magnitude Σ|terms|), both [H, n, m]."""
    ts, mags = [], []
    for i in range(a.size(0)):
        z = a[i].unsqueeze(0) + b
        if kind == "gat":
            ts.append(F.leaky_relu(z, slope))
            mags.append((a[i].abs().unsqueeze(0) + b.abs()).detach())
        else:
            ts.append((c * F.leaky_relu(z, slope)).sum(-1))
            mags.append((c.abs() * z.abs()).sum(-1).detach())
    n, m, H = a.size(0), b.size(0), b.size(1)
    stack = (lambda xs: torch.stack(xs).permute(2, 0, 1) if xs else torch.zeros((H, n, m), dtype=torch.float64))
    return stack(ts), stack(mags)


def dense_oracle(kind, mask, B, a, b, c, dO, slope, use_bias=True):
    """Float64 results of one item as a dict: O [n, H, d], the gradients (da, db, dc, dB — dB dense, meaningful at the stored
    positions), P and the logits t [H, n, m] and their magnitudes `mag`."""
    a, b, c, B = (x.detach().double().requires_grad_(True) for x in (a, b, c, B))
    t, mag = _logits(kind, a, b, c, slope)
    if use_bias:
        t = t + B.unsqueeze(0)
    has = mask.any(1).view(-1, 1)
    tm = t.masked_fill(~mask, float("-inf")).masked_fill(~has, 0.0)
    P = torch.softmax(tm, -1) * has
    O = torch.einsum("hij,jhd->ihd", P, c if kind == "gat" else b)
    da, db, dc, dB = torch.autograd.grad(O, (a, b, c, B), dO.double(), allow_unused=True)
    return dict(O=O.detach(), da=da, db=db, dc=dc, dB=torch.zeros_like(B) if dB is None else dB, P=P.detach(), t=t.detach(), mag=mag)


@torch.no_grad()
def error_bounds(kind, mask, B, a, b, c, dO, slope, use_bias, u, tiny, ref, grads=True):
    """First-order bounds on |computed − exact| for one item, in the form of _attention_ref.error_bounds with its constants (C = 8
    forward, 16 gradients, `tiny` per stored entry for an underflowing exp); `ref` from :func:`dense_oracle`.  Per row i and head,
    L the row's length, L'_j the column's, v the messages (V or X_src):

      e_j = 3u (|s_dst| + |s_src| + |b_j|)   ("gat": an addition, the LeakyReLU's product, the bias)
      e_j = (d + 3) u (Σ_k |att_k||z_k| + |b_j|)   ("gatv2": z, the selected coefficient, a dot of d terms, the bias)
      ρ_j = e_j + Σ_l p_l e_l + (3L + |t_j − max t| + C) u
      |O − ·| <= Σ_j p_j ρ_j |v_j| + tiny Σ_j |v_j|
      dP̄_j = Σ_c |dO_c||v_jc|     δ̄ = Σ_j p_j dP̄_j + d u Σ_c |dO_c||O_c|     dS̄_j = p_j (dP̄_j + δ̄)
      E_j = (ρ_j + d u) dS̄_j + the underflow terms of _attention_ref      (the error of dS_j)
    A sum of N terms in a fixed order adds N u Σ|terms|, a rounded coefficient (att·slope, slope·z) one more u:
      "gat"    |ds_dst − ·| <= Σ_j (E_j + L u dS̄_j) |lrelu'|        |ds_src_j − ·| <= Σ_i (E_ij + L'_j u dS̄_ij) |lrelu'|
               |dV_j − ·| <= Σ_i ((ρ_ij + L'_j u) p_ij + tiny) |dO_i|
      "gatv2"  |dX_dst_k − ·| <= Σ_j (E_j + (L + 1) u dS̄_j) |c_jk|   with c_jk = att_k or att_k·slope
               |dX_src_jk − ·| <= Σ_i (E_ij + (L'_j + 1) u dS̄_ij) |c_ik| + Σ_i ((ρ_ij + 2 L'_j u) p_ij + tiny) |dO_ik|
               |datt_k − ·| <= Σ_ij (E_ij + (nnz + 1) u dS̄_ij) |lrelu(z_ijk)|
      |dA_ij − ·| <= Σ_h (E_ij,h + H u dS̄_ij,h)
    Returns a dict with the keys of dense_oracle's results (O, da, db, dc, dB); grads=False: O only."""
    a, b, c, dO, B = (x.double() for x in (a, b, c, dO, B))
    P, O, t = ref["P"], ref["O"], ref["t"]
    v = c if kind == "gat" else b
    n, (m, H, d) = mask.size(0), v.shape
    M = mask.unsqueeze(0).double()
    mag = ref["mag"] + (B.abs().unsqueeze(0) if use_bias else 0.0)
    mag = torch.where(mask.unsqueeze(0), mag, torch.zeros_like(mag))
    tm = t.masked_fill(~mask, float("-inf"))
    top = tm.amax(-1, keepdim=True)
    dist = torch.where(mask.unsqueeze(0) & tm.isfinite(), (tm - top).abs(), torch.zeros_like(tm)).nan_to_num(0.0, 0.0, 0.0)
    L = mask.sum(1).double().view(1, n, 1)
    Lc = mask.sum(0).double().view(1, 1, m)
    e = (3 if kind == "gat" else d + 3) * u * mag
    pe = (P * e).sum(-1, keepdim=True)
    rho = (lambda C: (e + pe + (3 * L + dist + C) * u) * M)
    r8, r16 = rho(8), rho(16)
    Va, Ga = v.abs(), dO.abs()
    out = dict(O=torch.einsum("hij,jhd->ihd", P * r8, Va) + tiny * torch.einsum("hij,jhd->ihd", M.expand(H, -1, -1), Va))
    if not grads:
        return out
    dPb = torch.einsum("ihd,jhd->hij", Ga, Va)
    tail = d * u * (Ga * O.abs()).sum(-1).t().unsqueeze(-1)
    db_ = (P * dPb).sum(-1, keepdim=True) + tail
    db_under = tiny * (dPb * M).sum(-1, keepdim=True)
    dSb = P * (dPb + db_)
    dSb_under = P * db_under + tiny * M * (dPb + db_ + db_under)
    E = (r16 + d * u) * dSb + dSb_under
    msg = torch.einsum("hij,ihd->jhd", (r16 + (1 if kind == "gat" else 2) * Lc * u) * P + tiny * M, Ga)
    out["dB"] = (E + H * u * dSb).sum(0)
    z = a.unsqueeze(1) + b.unsqueeze(0)                                   # [n, m, H] or [n, m, H, d]
    if kind == "gat":
        sl = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, abs(slope)))
        out["da"] = torch.einsum("hij,ijh->ih", E + L * u * dSb, sl)
        out["db"] = torch.einsum("hij,ijh->jh", E + Lc * u * dSb, sl)
        out["dc"] = msg
    else:
        coef = torch.where(z > 0, c.expand_as(z), (c * slope).expand_as(z)).abs()
        out["da"] = torch.einsum("hij,ijhk->ihk", E + (L + 1) * u * dSb, coef)
        out["db"] = torch.einsum("hij,ijhk->jhk", E + (Lc + 1) * u * dSb, coef) + msg
        out["dc"] = torch.einsum("hij,ijhk->hk", E + (float(mask.sum()) + 1) * u * dSb, F.leaky_relu(z, slope).abs())
    return out
