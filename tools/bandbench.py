#!/usr/bin/env python3
"""Banded triangular solves on one GPU: `sparse_triangular_solve` (the sync-free sweep) and `sparse_banded_triangular_solve` (the
log-depth chunk solve) in one process on the same operands, one JSON line per case.

    python tools/bandbench.py [--widths 1 2 4 8] [--rows 65536 1048576] [--columns 1 8 64] [--out profiles/band/tool_lines.jsonl]

A case is a lower band of width w with n rows (every row full: w sub-diagonal entries in (−1, 1) scaled to an absolute sum of at
most 0.5, a diagonal in ±[1, 2]), CSR int32 fp32, and p right-hand sides.  Timed: the forward solve under no_grad and forward +
backward (two solves and the SDDMM) of both functions.  Times are device-event medians over `reps` blocks of `loops` calls after
warm-up, in microseconds; a path whose call takes over 20 ms is timed one call per block, three blocks (the sweep at n = 2²⁰ takes
most of a second per solve).  `ratio_*` is sweep time / banded time in the same run.  `max_abs_diff` is between the two solutions.
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import torch

if not os.environ.get("PYTHONPATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, warmup=5):
    for _ in range(warmup):      # (the pattern's plans and the sync-free sweep's width settle during the first calls)
        fn()
        tsgu.wait_for_plans()
    torch.cuda.synchronize()
    ms = once(fn)
    loops, reps = (1, 3) if ms > 20.0 else (max(1, min(20, int(20.0 / max(ms, 1e-3)))), 7)
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


def band(n, w, dev):
    """Full lower band of width w as a CSR tensor (rows 0 … w−1 are shorter)."""
    g = torch.Generator().manual_seed(n + w)
    rows = torch.arange(n).repeat_interleave(w + 1)
    cols = rows - torch.arange(w, -1, -1).repeat(n)
    keep = cols >= 0
    off = torch.rand(n, w, generator=g) * 2 - 1
    off = off * (0.25 + 0.25 * torch.rand(n, 1, generator=g)) / off.abs().sum(1, keepdim=True)
    diag = (1 + torch.rand(n, 1, generator=g)) * torch.where(torch.rand(n, 1, generator=g) < 0.5, -1.0, 1.0)
    val = torch.cat((off, diag), 1).reshape(-1)[keep]
    crow = torch.zeros(n + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(keep.view(n, w + 1).sum(1), 0)
    return torch.sparse_csr_tensor(crow.to(torch.int32).to(dev), cols[keep].to(torch.int32).to(dev), val.to(dev), (n, n))


def measure(n, w, p, dev):
    A = band(n, w, dev)
    B = torch.randn(n, p, device=dev)
    ones = torch.ones(n, p, device=dev)
    Ag, Bg = A.detach().requires_grad_(True), B.clone().requires_grad_(True)
    out = {"n": n, "w": w, "columns": p, "nnz": A.values().numel(), "dtype": "float32"}
    sol = {}
    for name, fn in (("sweep", tsgu.sparse_triangular_solve), ("banded", tsgu.sparse_banded_triangular_solve)):
        def fwd():
            with torch.no_grad():
                return fn(A, B, upper=False)

        def fwdbwd():
            torch.autograd.grad(fn(Ag, Bg, upper=False), (Ag, Bg), ones)

        sol[name] = fwd()
        out[f"{name}_forward_us"] = timed(fwd)
        out[f"{name}_fwdbwd_us"] = timed(fwdbwd)
    out["ratio_forward"] = round(out["sweep_forward_us"] / out["banded_forward_us"], 2)
    out["ratio_fwdbwd"] = round(out["sweep_fwdbwd_us"] / out["banded_fwdbwd_us"], 2)
    out["max_abs_diff"] = float((sol["sweep"] - sol["banded"]).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--rows", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--columns", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default=None, help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bandbench measures on the GPU only"
    dev = torch.device("cuda:0")
    for n in args.rows:
        for w in args.widths:
            for p in args.columns:
                line = json.dumps(dict(measure(n, w, p, dev), device=torch.cuda.get_device_name(0)))
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
