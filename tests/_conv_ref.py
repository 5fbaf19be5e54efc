"""The float64 reference of neighbor_mm on the CPU: a loop over the stencil slots with index_select, and the shared test data."""
import torch


def reference(x, w, nbr, bias=None, g=None):
    """dict with "out" and, given g, "grad_x", "grad_w", "grad_bias"; and under "<name>_mag" the Σ|terms| of every element."""
    x64, w64, nbr = x.double().cpu(), w.double().cpu(), nbr.cpu().long()
    n_in, (n_out, K) = x64.size(0), nbr.shape
    ok = ((nbr >= 0) & (nbr < n_in)).double()
    at = nbr.clamp(0, max(n_in - 1, 0))
    res = {}
    for tag, f in (("", lambda t: t), ("_mag", torch.abs)):
        b = torch.zeros(w64.size(2), dtype=torch.float64) if bias is None else f(bias.double().cpu())
        out = b.repeat(n_out, 1)
        if g is not None:
            g64 = f(g.double().cpu())
            gx, gw = torch.zeros_like(x64), torch.zeros_like(w64)
        for k in range(K if n_in else 0):
            xk = f(x64).index_select(0, at[:, k]) * ok[:, k, None]
            out += xk @ f(w64[k])
            if g is not None:
                gx.index_add_(0, at[:, k], (g64 @ f(w64[k]).t()) * ok[:, k, None])
                gw[k] = xk.t() @ g64
        res["out" + tag] = out
        if g is not None:
            res.update({"grad_x" + tag: gx, "grad_w" + tag: gw, "grad_bias" + tag: g64.sum(0)})
    return res


def table(n_in, n_out, K, gen, dtype=torch.int64):
    """Every column a random partial injection with about half its entries absent; column 0 all absent (K > 2), the last column
    the identity on min(n_in, n_out) rows (K > 1), row n_out // 2 all absent (n_out > 2), and rows [128, 256) absent but for one entry."""
    nbr = torch.full((n_out, K), -1, dtype=torch.int64)
    for k in range(K):
        rows = torch.randperm(n_out, generator=gen)[:min(n_in, n_out)]
        nbr[rows, k] = torch.randperm(n_in, generator=gen)[:rows.numel()]
    nbr[torch.rand((n_out, K), generator=gen) < 0.5] = -1
    if K > 1:
        m = min(n_in, n_out)
        nbr[:, K - 1] = -1
        nbr[:m, K - 1] = torch.arange(m)
    if K > 2:
        nbr[:, 0] = -1
    if n_out > 2:
        nbr[n_out // 2] = -1
    if n_out > 128:
        nbr[128:256] = -1
        free = sorted(set(range(n_in)) - set(nbr[:, K // 2].tolist()))
        nbr[min(130, n_out - 1), K // 2] = free[0]
    return nbr.to(dtype)


def integers(n_in, n_out, K, d1, d2, gen):
    """x, g in [-3, 3], bias in [-2, 2] and w an asymmetric ramp in (k, c1, c2) with |w| <= 3: every sum stays far below 2^24
    (forward: K * d1 * 9 <= 27 * 130 * 9 < 2^15)."""
    x = torch.randint(-3, 4, (n_in, d1), generator=gen).double()
    g = torch.randint(-3, 4, (n_out, d2), generator=gen).double()
    k, c1, c2 = torch.meshgrid(torch.arange(K), torch.arange(d1), torch.arange(d2), indexing="ij")
    w = ((3 * k + 2 * c1 + 5 * c2) % 7 - 3).double()
    bias = torch.randint(-2, 3, (d2,), generator=gen).double()
    return x, w, g, bias
