"""Operands and float64 truths shared by the density tests of the sparse multivariate normal (CPU and GPU files).

The inputs are those of tests/golden/encoder_mvn.npz (the encoder's strictly-lower factor, ``Lfull`` with a stored diagonal,
``diagonal``, ``loc``, the reference's samples as ``value``; batched B = 2).  The truth is ``torch.distributions.MultivariateNormal``
built DENSELY in float64 (``covariance_matrix=`` / ``precision_matrix=``), and float64 autograd through those dense formulas for the
gradients of ``Σ_c w_c · log_prob_c``.
"""

import numpy as np
import torch
from torch.distributions import MultivariateNormal

import _golden as G

SHAPE, RADIUS, N = (2, 5, 4, 6), 1.5, 240
FORMS = ("scale_llt", "scale_ldlt", "prec_llt", "prec_ldlt")
TOL = {torch.float32: 1e-5, torch.float64: 1e-12}      # the project's own (tests/test_gpu_next_rows.py, rsample on the same inputs)


def rel(got, want):
    """max|got − want| / max|want|."""
    return G.rel_err(_np(got), _np(want))


def rel_norm(got, want):
    """‖got − want‖₂ / ‖want‖₂."""
    a, b = _np(got).astype(np.float64).ravel(), _np(want).astype(np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def weights(shape, dtype=torch.float64):
    k = int(np.prod(shape)) if len(shape) else 1
    return torch.linspace(0.5, 1.5, k, dtype=dtype).reshape(shape)


def as_layout(A, layout, itype):
    """CSR tensor `A` in `layout` with index dtype `itype` (same entries, same order)."""
    if layout == "csr":
        return torch.sparse_csr_tensor(A.crow_indices().to(itype), A.col_indices().to(itype), A.values(), A.shape)
    C = A.to_sparse_coo().coalesce()
    return torch.sparse_coo_tensor(C.indices().to(itype), C.values(), C.shape, is_coalesced=True)


def operands(vn, batched, device="cpu"):
    """dict(Ls, Lfull, diag, loc, value): CSR int64 factors (strictly lower; lower with stored diagonal) of encoder_mvn.npz.  The
    batched stored diagonal (the file has none) is ``0.5 + diagb``, in [1, 2) like the unbatched one."""
    from torchsparsegradutils_amd.encoders import PairwiseEncoder

    z = G.load("encoder_mvn.npz")
    enc = PairwiseEncoder(RADIUS, SHAPE, diag=False, upper=False, channel_voxel_relation="intra", layout=torch.sparse_csr)
    if not batched:
        Ls = enc(G.t(z[vn + "_w"]))
        Lfull = torch.sparse_csr_tensor(G.t(z[vn + "_Lfull_crow"]), G.t(z[vn + "_Lfull_col"]), G.t(z[vn + "_Lfull_val"]), (N, N))
        diag, loc = G.t(z[vn + "_diag"]), G.t(z[vn + "_loc"])
        value = {f: G.t(z[f"{vn}_{f}_x"]) for f in FORMS}
    else:
        Ls = enc(G.t(z[vn + "_wb"]))
        diag, loc = G.t(z[vn + "_diagb"]), G.t(z[vn + "_locb"])
        Lfull = (Ls.to_dense() + torch.diag_embed(0.5 + diag)).to_sparse_csr()       # (every item has the encoder's pattern + the diagonal)
        value = {f: G.t(z[vn + "_prec_ldlt_batched_x"]) for f in FORMS}
    Ls = torch.sparse_csr_tensor(Ls.crow_indices().to(torch.int64), Ls.col_indices().to(torch.int64), Ls.values(), Ls.shape)
    out = dict(Ls=Ls, Lfull=Lfull, diag=diag, loc=loc, value=value)
    return {k: ({f: x.to(device) for f, x in v.items()} if isinstance(v, dict) else v.to(device)) for k, v in out.items()}


def dense_truth(form, factor, diag, loc, value, w=None):
    """float64: (log_prob, entropy, variance or None, dict of gradients of Σ w·log_prob w.r.t. factor (dense, masked to the stored
    entries), diag, loc, value) from MultivariateNormal on the dense matrices."""
    Ld = factor.detach().cpu().to_dense().double()
    mask = torch.zeros_like(Ld, dtype=torch.bool)
    C = factor.detach().cpu()
    C = C.to_sparse_coo() if C.layout != torch.sparse_coo else C
    idx = C.coalesce().indices().long()
    mask[tuple(idx)] = True
    Ld = Ld.requires_grad_(True)
    ldlt = form.endswith("ldlt")
    D = diag.detach().cpu().double().requires_grad_(True) if ldlt else None
    locd = loc.detach().cpu().double().requires_grad_(True)
    x = value.detach().cpu().double().requires_grad_(True)
    if ldlt:
        LI = Ld + torch.eye(Ld.size(-1), dtype=torch.float64)
        M = LI @ torch.diag_embed(D) @ LI.transpose(-1, -2)
    else:
        M = Ld @ Ld.transpose(-1, -2)
    ref = MultivariateNormal(locd, covariance_matrix=M) if form.startswith("scale") else MultivariateNormal(locd, precision_matrix=M)
    lp = ref.log_prob(x)
    w = weights(lp.shape) if w is None else w.detach().cpu().double()
    leaves = [Ld, locd, x] + ([D] if ldlt else [])
    grads = torch.autograd.grad((lp * w).sum(), leaves)
    g = dict(factor=grads[0] * mask, loc=grads[1], value=grads[2], diag=grads[3] if ldlt else None)
    var = ref.variance.detach() if form.startswith("scale") else None
    return lp.detach(), ref.entropy().detach(), var, g


def distribution(form, factor, diag, loc, validate_args=None):
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormal

    kw = {"scale_tril" if form.startswith("scale") else "precision_tril": factor}
    if form.endswith("ldlt"):
        kw["diagonal"] = diag
    return SparseMultivariateNormal(loc, validate_args=validate_args, **kw)


def dense64(sparse):
    """A sparse tensor (a factor's gradient) as a dense float64 array on the CPU."""
    return sparse.detach().cpu().to_dense().double()


# ---- the encoder's real shape: float64 truth with torch's CPU sparse ops, closed-form gradients ----------------------------------
def stencil_factor(form, n_side=64, seed=0, device="cpu", dtype=torch.float32):
    """The truncated 27-point lower factor on an n_side³ lattice: strictly lower for the LDLᵀ forms, with a stored diagonal for the
    LLᵀ forms; off-diagonals 0.03·randn, stored diagonal 1 + rand, D = 0.5 + rand, loc = randn, 8 values loc + 1.5·randn.
    Returns (crow, col, val, D, loc, value) on `device` (int32 indices)."""
    from torchsparsegradutils_amd.utils import synthetic

    part = "strict_lower" if form.endswith("ldlt") else "lower"
    crow, col = synthetic.box_stencil(n_side, n_side, n_side, periodic=(False,) * 3, part=part)
    n = n_side ** 3
    g = torch.Generator().manual_seed(seed)
    val = 0.03 * torch.randn(col.numel(), generator=g, dtype=dtype)
    rows = torch.repeat_interleave(torch.arange(n), (crow[1:] - crow[:-1]).long())
    on_diag = col.long() == rows
    val[on_diag] = 1.0 + torch.rand(int(on_diag.sum()), generator=g, dtype=dtype)
    D = 0.5 + torch.rand(n, generator=g, dtype=dtype)
    loc = torch.randn(n, generator=g, dtype=dtype)
    value = loc + 1.5 * torch.randn(8, n, generator=g, dtype=dtype)
    return tuple(t.to(device) for t in (crow, col, val, D, loc, value))


def sparse_truth(form, crow, col, val, D, loc, value, w):
    """float64 on the CPU, sparse throughout: (log_prob, entropy, gradients of Σ_c w_c·log_prob_c w.r.t. the stored values, D and
    value) by the closed forms — per sample, with d = value − loc:

        scale LLᵀ    z = L⁻¹d, u = L⁻ᵀz                      ∂value = −u,           ∂L_ij = u_i z_j − [i=j]/L_ii
        scale LDLᵀ   z = (L+I)⁻¹d, q = z/D, u = (L+I)⁻ᵀq      ∂value = −u,           ∂L_ij = u_i z_j,        ∂D_i = ½q_i² − ½/D_i
        prec LLᵀ     y = Lᵀd                                 ∂value = −L y,         ∂L_ij = −d_i y_j + [i=j]/L_ii
        prec LDLᵀ    y = Lᵀd + d                             ∂value = −(L+I)(D∘y),  ∂L_ij = −d_i D_j y_j,   ∂D_i = −½y_i² + ½/D_i
    """
    f64 = torch.float64
    crow, col = crow.cpu().long(), col.cpu().long()
    val, D, loc, value, w = (t.detach().cpu().to(f64) for t in (val, D, loc, value, w))
    n = loc.numel()
    rows = torch.repeat_interleave(torch.arange(n), crow[1:] - crow[:-1])
    L = torch.sparse_csr_tensor(crow, col, val, (n, n))
    LT = torch.sparse_coo_tensor(torch.stack([col, rows]), val, (n, n)).coalesce()
    ldlt = form.endswith("ldlt")
    d = (value - loc).t().contiguous()                      # (n, k)
    on_diag = col == rows
    wsum = w.sum()

    def solve(rhs, transpose):
        return torch.triangular_solve(rhs.contiguous(), L, upper=False, transpose=transpose, unitriangular=ldlt).solution

    gD = None
    if form.startswith("scale"):
        z = solve(d, False)
        q = z / D[:, None] if ldlt else z
        u = solve(q, True)
        M = (z * q).sum(0)
        gval = -(u * w).t()
        gL = ((u * w)[rows] * z[col]).sum(1)
        if ldlt:
            half = 0.5 * D.log().sum()
            gD = (0.5 * q * q * w).sum(1) - 0.5 * wsum / D
        else:
            half = val[on_diag].log().sum()
            gL[on_diag] -= wsum / val[on_diag]
    else:
        y = torch.sparse.mm(LT, d) + (d if ldlt else 0)
        s = y * D[:, None] if ldlt else y
        M = (y * s).sum(0)
        gval = -((torch.sparse.mm(L, s) + (s if ldlt else 0)) * w).t()
        gL = -((d * w)[rows] * s[col]).sum(1)
        if ldlt:
            half = -0.5 * D.log().sum()
            gD = -(0.5 * y * y * w).sum(1) + 0.5 * wsum / D
        else:
            half = -val[on_diag].log().sum()
            gL[on_diag] += wsum / val[on_diag]
    lp = -0.5 * (n * np.log(2 * np.pi) + M) - half
    ent = 0.5 * n * (1 + np.log(2 * np.pi)) + half
    return lp, ent, dict(factor=gL, diag=gD, value=gval)
