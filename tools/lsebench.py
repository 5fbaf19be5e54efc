#!/usr/bin/env python3
"""sparse_logsumexp / sparse_bidir_logsumexp timings on one GPU: one JSON line.

    python tools/lsebench.py [--loops 20] [--reps 5]

Cases: the reference benchmark's "million" shape (N = M = 2^20, nnz = 2^22 uniformly random, CSR int32 fp32, dim=1) and the
C2 pattern (27-point periodic stencil, N = 10^6, CSR int32 fp32: dim=1, dim=0, bidir), each forward and forward + backward.
Times are device-event medians over `reps` blocks of `loops` calls after warm-up.  `bytes` is the algorithmic traffic of the
call (index arrays read once, values read once per direction, outputs / gradient written once) and `frac_8tbs` its rate as
a fraction of 8 TB/s.  Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


def timed(fn, loops, reps):
    for _ in range(3):
        fn()
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
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "cases": []}

    # "million": N = M = 2^20, nnz = 2^22
    n = 1 << 20
    nnz = 1 << 22
    keys = torch.unique(torch.randint(0, n * n, (nnz,), device=dev, dtype=torch.int64))     # sorted, distinct cells
    mrow = torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True)
    M = torch.sparse_csr_tensor(mrow, (keys % n).int(), torch.randn(keys.numel(), device=dev), (n, n))
    crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
    nc = crow.numel() - 1
    C2 = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), torch.randn(col.numel(), device=dev), (nc, nc))

    def add(name, A, call, bytes_fwd, bytes_bwd):
        # (a sparse leaf: torch's own backward of the sparse_csr_tensor constructor goes through a dense n x n tensor)
        L = A.detach().requires_grad_(True)

        def fwd():
            with torch.no_grad():
                call(L)

        def fwdbwd():
            out = call(L)
            out = out if isinstance(out, tuple) else (out,)
            torch.autograd.grad(out, L, [torch.ones_like(o) for o in out])

        tf, tb = timed(fwd, args.loops, args.reps), timed(fwdbwd, args.loops, args.reps)
        res["cases"].append({
            "case": name, "fwd_us": round(tf, 2), "fwd_bytes": bytes_fwd, "fwd_frac_8tbs": round(bytes_fwd / (tf * 1e-6) / 8e12, 3),
            "fwdbwd_us": round(tb, 2), "bwd_bytes": bytes_bwd,
        })

    def sizes(A):
        r = A.size(0)
        k = A.values().numel()
        return r, k

    r, k = sizes(M)
    add("million dim=1", M, lambda L: tsgu.sparse_logsumexp(L, 1), 4 * (r + 1) + 4 * k + 4 * r,
        4 * (r + 1) + 4 * k + 4 * k + 8 * r)
    r, k = sizes(C2)
    b_row = 4 * (r + 1) + 4 * k + 4 * r
    b_col = 4 * (r + 1) + 4 * k + 4 * k + 4 * r
    add("C2 dim=1", C2, lambda L: tsgu.sparse_logsumexp(L, 1), b_row, 4 * (r + 1) + 8 * k + 8 * r)
    add("C2 dim=0", C2, lambda L: tsgu.sparse_logsumexp(L, 0), b_col, 8 * k + 4 * k + 8 * r)
    add("C2 bidir", C2, lambda L: tsgu.sparse_bidir_logsumexp(L), b_row + b_col,
        4 * (r + 1) + 4 * k + 4 * k + 4 * k + 16 * r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
