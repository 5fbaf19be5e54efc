#!/usr/bin/env python3
"""Density of the sparse multivariate normal on one GPU: one JSON line.

    python tools/mvnbench.py [--loops 10] [--reps 5] [--side 64]

The encoder's real shape: the truncated 27-point lower factor on a side³ lattice (N = 262 144 at the default; strictly lower for
the LDLᵀ forms, with a stored diagonal for the LLᵀ forms), CSR int32 fp32, 8 values.  For each of the four parameterisations:
`log_prob` forward and forward + backward (gradients of the factor, `value` and `diagonal`), and beside each, ON THE SAME OPERANDS,
the bare existing call it is built on — `sparse_triangular_solve` (covariance forms) or the transposed product (precision forms),
forward and forward + backward.  `ratio_*` = log_prob / bare call: what the reductions of csrc/mvn.hip and the autograd plumbing
add.  `entropy` and `variance` are timed alone.  Times are device-event medians over `reps` blocks of `loops` calls after warm-up,
in microseconds.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd.distributions import SparseMultivariateNormal  # noqa: E402
from torchsparsegradutils_amd.distributions.sparse_multivariate_normal import _sparse_tmm  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402

FORMS = ("scale_llt", "scale_ldlt", "prec_llt", "prec_ldlt")


def timed(fn, loops, reps):
    for _ in range(4):      # (the pattern's plans and the sweep width settle during its first calls)
        fn()
        tsgu.wait_for_plans()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(loops):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / loops)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


def factor(form, side, dev):
    part = "strict_lower" if form.endswith("ldlt") else "lower"
    crow, col = synthetic.box_stencil(side, side, side, periodic=(False,) * 3, part=part)
    n = side ** 3
    val = 0.03 * torch.randn(col.numel())
    rows = torch.repeat_interleave(torch.arange(n), (crow[1:] - crow[:-1]).long())
    on_diag = col.long() == rows
    val[on_diag] = 1.0 + torch.rand(int(on_diag.sum()))
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n, n)), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--values", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mvnbench measures on the GPU only"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "side": args.side, "values": args.values, "cases": []}
    for form in FORMS:
        A, n = factor(form, args.side, dev)
        A = A.requires_grad_(True)
        ldlt, covariance = form.endswith("ldlt"), form.startswith("scale")
        D = (0.5 + torch.rand(n, device=dev)).requires_grad_(True)
        loc = torch.randn(n, device=dev)
        value = (loc + 1.5 * torch.randn(args.values, n, device=dev)).requires_grad_(True)
        kw = {"scale_tril" if covariance else "precision_tril": A}
        if ldlt:
            kw["diagonal"] = D
        dist = SparseMultivariateNormal(loc, validate_args=False, **kw)
        leaves = [A, value] + ([D] if ldlt else [])
        d = (value.detach() - loc).requires_grad_(True)
        ones = torch.ones(args.values, n, device=dev)

        def bare():
            if covariance:
                return tsgu.sparse_triangular_solve(A, d.t(), upper=False, unitriangular=ldlt).t()
            return _sparse_tmm(A, d.t()).t()

        def lp_fwd():
            with torch.no_grad():
                dist.log_prob(value)

        def lp_fwdbwd():
            torch.autograd.grad(dist.log_prob(value).sum(), leaves)

        def bare_fwd():
            with torch.no_grad():
                bare()

        def bare_fwdbwd():
            torch.autograd.grad(bare(), (A, d), ones)

        def entropy():
            with torch.no_grad():
                dist.entropy()

        case = {"form": form, "n": n, "nnz": A.values().numel(),
                "log_prob_fwd_us": timed(lp_fwd, args.loops, args.reps), "bare_fwd_us": timed(bare_fwd, args.loops, args.reps),
                "log_prob_fwdbwd_us": timed(lp_fwdbwd, args.loops, args.reps),
                "bare_fwdbwd_us": timed(bare_fwdbwd, args.loops, args.reps), "entropy_us": timed(entropy, args.loops, args.reps)}
        case["ratio_fwd"] = round(case["log_prob_fwd_us"] / case["bare_fwd_us"], 3)
        case["ratio_fwdbwd"] = round(case["log_prob_fwdbwd_us"] / case["bare_fwdbwd_us"], 3)
        if covariance:
            def variance():
                with torch.no_grad():
                    dist.variance
            case["variance_us"] = timed(variance, args.loops, args.reps)
        res["cases"].append(case)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
