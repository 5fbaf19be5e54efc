#!/usr/bin/env python3
"""gather_mm / segment_mm timings on one GPU: one JSON line.

    python tools/immbench.py [--loops 20] [--reps 5] [--quick]

Cases: N = 2^20 rows, R in {16, 256}, D1 = D2 = D in {64, 128}, fp32 and bf16; gather_mm with uniformly random idx_b
(int64) and segment_mm with equal lengths; forward and forward + backward (grad_a and grad_b).  Times are device-event medians
over `reps` blocks of `loops` calls after warm-up.  `bytes` / `flops` are the algorithmic traffic and work of the call,
computed from shapes (operands read once, results written once, the index read once per pass); `bound_us` is the larger of
bytes / 8 TB/s and flops / peak (157.3 TF fp32, 2516.8 TF bf16 MFMA), `bound_by` which of the two, and `frac` bound_us / time.
Yardsticks on the same GPU: torch.mm of the whole (N, D) x (D, D) product (R = 1, the dense ceiling) and a torch-op
segmented product (stable argsort + one torch.mm per segment + scatter back).  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402

HBM = 8e12
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 16 * 157.3e12}


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


def roof(t_us, nbytes, flops, dtype):
    tb, tf = nbytes / HBM * 1e6, flops / PEAK[dtype] * 1e6
    bound = max(tb, tf)
    return {"us": round(t_us, 2), "bytes": nbytes, "flops": flops, "bound_us": round(bound, 2),
            "bound_by": "bytes" if tb >= tf else "flops", "frac": round(bound / t_us, 3)}


def torch_segmented(a, b, idx, R):
    """The torch-op baseline: stable argsort, one torch.mm per segment, scatter back (lengths read on the host)."""
    order = torch.argsort(idx, stable=True)
    counts = torch.bincount(idx, minlength=R).tolist()
    ap = a.index_select(0, order)
    res = torch.empty((a.size(0), b.size(2)), dtype=a.dtype, device=a.device)
    lo = 0
    for r, c in enumerate(counts):
        if c:
            torch.mm(ap[lo:lo + c], b[r], out=res[lo:lo + c])
        lo += c
    out = torch.empty_like(res)
    out[order] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="R = 16 only")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n = 1 << 20
    res = {"device": torch.cuda.get_device_name(0), "N": n, "cases": [], "dense_mm": []}
    for dtype in (torch.float32, torch.bfloat16):
        s = torch.tensor([], dtype=dtype).element_size()
        for d in (64, 128):
            a = torch.randn(n, d, device=dev, dtype=dtype)
            w = torch.randn(d, d, device=dev, dtype=dtype)
            t = timed(lambda: torch.mm(a, w), args.loops, args.reps)
            res["dense_mm"].append({"dtype": str(dtype)[6:], "D": d,
                                    **roof(t, s * (2 * n * d + d * d), 2 * n * d * d, dtype)})
            g = torch.randn(n, d, device=dev, dtype=dtype)
            for R in ((16,) if args.quick else (16, 256)):
                b = torch.randn(R, d, d, device=dev, dtype=dtype)
                idx = torch.randint(0, R, (n,), device=dev)
                seglen = torch.full((R,), n // R, dtype=torch.int64)
                base_us = timed(lambda: torch_segmented(a, b, idx, R), 3, 3)
                for fn, call, ib in (("gather_mm", lambda x, y: tsgu.gather_mm(x, y, idx), 4 * n),
                                     ("segment_mm", lambda x, y: tsgu.segment_mm(x, y, seglen), 0)):
                    xa, xb = a.detach().requires_grad_(True), b.detach().requires_grad_(True)

                    def fwd():
                        with torch.no_grad():
                            call(xa, xb)

                    def fwdbwd():
                        out = call(xa, xb)
                        torch.autograd.grad(out, (xa, xb), g)

                    tf, tb = timed(fwd, args.loops, args.reps), timed(fwdbwd, args.loops, args.reps)
                    fb = s * (2 * n * d + R * d * d) + ib                       # a, b, out; the int32 perm read
                    bb = fb + s * (2 * n * d + R * d * d) + s * (2 * n * d + R * d * d) + 2 * ib   # + grad_a, grad_b
                    fl = 2 * n * d * d
                    res["cases"].append({"fn": fn, "dtype": str(dtype)[6:], "R": R, "D": d,
                                         "fwd": roof(tf, fb, fl, dtype), "fwdbwd": roof(tb, bb, 3 * fl, dtype),
                                         "fwdbwd_over_fwd": round(tb / tf, 2), "torch_segmented_fwd_us": round(base_us, 1)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
