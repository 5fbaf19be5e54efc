#!/usr/bin/env python3
"""sparse_sinkhorn against the composition that existed before it, on one GPU: one JSON line.

    python tools/sinkhornbench.py [--iters 20] [--reps 5] [--cases million,c2,topk]

The fused loop is `tsgu.sparse_sinkhorn(S, log_a, log_b, T)`.  The composition is what a user wrote without it: per half step
`values + v[col]` (or `+ u[row]`) as the values of a CSR tensor on S's pattern, `tsgu.sparse_logsumexp(..., include_zeros=False)`
along the direction, and `log_marginal − lse`; its backward is torch autograd through the 2T calls, which keeps their nnz-sized
values.  (The values enter the CSR tensor through a two-line autograd function, because torch's own backward of the
`sparse_csr_tensor` constructor goes through a dense n × m tensor.)

Cases, all CSR int32 fp32 with T iterations: the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22 uniformly random),
the C2 pattern (27-point periodic stencil, N = 10^6), and the pattern `sparse_topk_mm` selects at n = m = 16384, k = 16, d = 64.
Both sides run in the same process and take turns: `reps` rounds of (fused, composed), device-event time of one call of T
iterations each after a warm-up of both; the medians are reported per iteration, with the ratio composed / fused, for the forward
(no gradient) and for forward + backward (cotangents of all three outputs; gradients to S, log_a and log_b).  `peak_bytes` is
`torch.cuda.max_memory_allocated` over one forward + backward, less what was allocated before it.  The two results are compared
before anything is timed (`max_diff`).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


class _OnPattern(torch.autograd.Function):
    """values -> CSR tensor on fixed index tensors; the gradient is the cotangent's value array."""

    @staticmethod
    def forward(ctx, values, crow, col, shape):
        return torch.sparse_csr_tensor(crow, col, values, shape)

    @staticmethod
    def backward(ctx, g):
        return g.values(), None, None, None


def composed(crow, col, row, values, shape, la, lb, T):
    """(log_P values, u, v) by 2T sparse_logsumexp calls; `row`: the expanded row index."""
    col64 = col.long()
    v = torch.zeros(shape[1], dtype=values.dtype, device=values.device)
    for _ in range(T):
        u = la - tsgu.sparse_logsumexp(_OnPattern.apply(values + v[col64], crow, col, shape), 1, include_zeros=False)
        v = lb - tsgu.sparse_logsumexp(_OnPattern.apply(values + u[row], crow, col, shape), 0, include_zeros=False)
    return values + u[row] + v[col64], u, v


def event_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def run_case(name, crow, col, values, shape, T, reps):
    dev = values.device
    n, m = shape
    row = torch.repeat_interleave(torch.arange(n, device=dev), (crow[1:] - crow[:-1]).long(), output_size=col.numel())
    g = torch.Generator(device=dev).manual_seed(1)
    la, lb = torch.randn(n, device=dev, generator=g), torch.randn(m, device=dev, generator=g)
    cot = (torch.randn(values.numel(), device=dev, generator=g), torch.randn(n, device=dev, generator=g),
           torch.randn(m, device=dev, generator=g))
    S = torch.sparse_csr_tensor(crow, col, values, shape)
    gP = torch.sparse_csr_tensor(crow, col, cot[0], shape)

    def fused_fwd():
        with torch.no_grad():
            return tsgu.sparse_sinkhorn(S, la, lb, T)

    def composed_fwd():
        with torch.no_grad():
            return composed(crow, col, row, values, shape, la, lb, T)

    def fused_fwdbwd():
        L, a, b = S.detach().requires_grad_(True), la.clone().requires_grad_(True), lb.clone().requires_grad_(True)
        lp, u, v = tsgu.sparse_sinkhorn(L, a, b, T)
        return torch.autograd.grad((lp, u, v), (L, a, b), (gP, cot[1], cot[2]))

    def composed_fwdbwd():
        x, a, b = values.clone().requires_grad_(True), la.clone().requires_grad_(True), lb.clone().requires_grad_(True)
        lp, u, v = composed(crow, col, row, x, shape, a, b, T)
        return torch.autograd.grad((lp, u, v), (x, a, b), cot)

    # the same result first (columns or rows without entries have infinite potentials on both sides)
    f, c = fused_fwd(), composed_fwd()
    fin = lambda t: torch.where(t.isfinite(), t, torch.zeros_like(t))  # noqa: E731
    diff = max(float((fin(f[0].values()) - fin(c[0])).abs().max()), float((fin(f[1]) - fin(c[1])).abs().max()),
               float((fin(f[2]) - fin(c[2])).abs().max()))
    gf, gc = fused_fwdbwd(), composed_fwdbwd()
    gdiff = max(float((gf[0].values() - gc[0]).abs().max()), float((gf[1] - gc[1]).abs().max()), float((gf[2] - gc[2]).abs().max()))
    del f, c, gf, gc
    for fn in (fused_fwd, composed_fwd, fused_fwdbwd, composed_fwdbwd):
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in ("fused_fwd", "composed_fwd", "fused_fwdbwd", "composed_fwdbwd")}
    for _ in range(reps):
        for k, fn in (("fused_fwd", fused_fwd), ("composed_fwd", composed_fwd), ("fused_fwdbwd", fused_fwdbwd),
                      ("composed_fwdbwd", composed_fwdbwd)):
            ts[k].append(event_time(fn))
    med = {k: median(v) for k, v in ts.items()}
    return {
        "case": name, "n": n, "m": m, "nnz": int(values.numel()), "T": T,
        "max_diff": diff, "max_grad_diff": gdiff,
        "fused_fwd_us_per_iter": round(med["fused_fwd"] / T, 2), "composed_fwd_us_per_iter": round(med["composed_fwd"] / T, 2),
        "fwd_ratio": round(med["composed_fwd"] / med["fused_fwd"], 2),
        "fused_fwdbwd_us_per_iter": round(med["fused_fwdbwd"] / T, 2), "composed_fwdbwd_us_per_iter": round(med["composed_fwdbwd"] / T, 2),
        "fwdbwd_ratio": round(med["composed_fwdbwd"] / med["fused_fwdbwd"], 2),
        "fused_peak_bytes": peak_of(fused_fwdbwd), "composed_peak_bytes": peak_of(composed_fwdbwd),
        "spread_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in ts.items()},
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="million,c2,topk")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sinkhornbench: no GPU: timings are taken on the device only")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"tool": "sinkhornbench", "device": torch.cuda.get_device_name(0), "dtype": "float32", "index": "int32", "cases": []}
    want = args.cases.split(",")
    if "million" in want:
        n = 1 << 20
        keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
        crow = torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True)
        res["cases"].append(run_case("million", crow, (keys % n).int(), torch.randn(keys.numel(), device=dev), (n, n), args.iters, args.reps))
        del keys, crow
    if "c2" in want:
        crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
        nc = crow.numel() - 1
        res["cases"].append(run_case("C2", crow.to(dev), col.to(dev), torch.randn(col.numel(), device=dev), (nc, nc), args.iters, args.reps))
    if "topk" in want:
        n, d, k = 16384, 64, 16
        Q, K = torch.randn(n, d, device=dev), torch.randn(n, d, device=dev)
        S = tsgu.sparse_topk_mm(Q, K, k, scale=d ** -0.5, index_dtype=torch.int32)
        res["cases"].append(run_case("topk n=m=16384 k=16", S.crow_indices(), S.col_indices(), S.values().detach(), (n, n), args.iters,
                                     args.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
