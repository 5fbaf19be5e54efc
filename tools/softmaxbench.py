#!/usr/bin/env python3
"""Segmented softmax timings on one GPU, beside the best form available without the fused kernels: one JSON line per case.

    python tools/softmaxbench.py [--loops 200] [--reps 7] [--out profiles/softmax/tool_lines.jsonl]

Cases: the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22 uniformly random) and the C2 pattern (27-point
periodic stencil, N = 10^6), CSR int32 fp32, each along dim=-1 (the pattern's own direction) and dim=-2 (through the cached
transpose and its perm), forward and forward + backward.

`fused`: tsgu_segment_softmax (and tsgu_segment_softmax_backward).  `composed`: the same softmax from the log-sum-exp entries —
tsgu_segment_logsumexp with include_zeros = 0, then tsgu_segment_logsumexp_backward with a gradient of ones, which is
exp(v - lse) per entry.  There is no segmented sum among the older entries, so the backward of `composed` is the fused one:
its forward + backward differs from `fused` by the forward alone.  Both are called through the ctypes binding with
the same allocation of their result, alternately, in the same process; the results are compared first.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up, with the least and the greatest block
beside them: differences inside that spread are noise.  `bytes_per_entry` is the algorithmic traffic of the value-sized arrays
(and of perm / the column index where they are read), per entry; the row pointer adds 4 (n + 1) bytes per launch.
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import _backend as be  # noqa: E402
from torchsparsegradutils_amd import _pattern  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in us per call; the functions take turns block by block."""
    for fn in fns.values():
        for _i in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _r in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(loops):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / loops)
    return {k: (round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("profiles", "softmax", "tool_lines.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    softmax_mod = importlib.import_module("torchsparsegradutils_amd.sparse_softmax")

    n = 1 << 20
    keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
    mrow = torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True)
    million = torch.sparse_csr_tensor(mrow, (keys % n).int(), torch.randn(keys.numel(), device=dev), (n, n))
    crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
    nc = crow.numel() - 1
    c2 = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), torch.randn(col.numel(), device=dev), (nc, nc))

    lines = []
    for shape, A in (("million", million), ("C2", c2)):
        plan = _pattern.from_csr(A)
        val = A.values().contiguous()
        nnz = val.numel()
        g = torch.randn_like(val)
        for dim in (-1, -2):
            own = dim == -1
            h = plan if own else plan.transposed
            ng = h.n_rows
            crossing = softmax_mod._crossing(h.crow, be.segment_softmax_range(val.dtype))
            lse = torch.empty(ng, dtype=val.dtype, device=dev)
            ws = torch.empty(be.segment_logsumexp_workspace_bytes(val.dtype, nnz), dtype=torch.uint8, device=dev)
            ones = torch.ones(ng, dtype=val.dtype, device=dev)

            def fused_fwd():          # (every form allocates its result, as the operators do)
                return be.segment_softmax(h.crow, h.perm, val, ng, False, crossing)

            def fused_bwd():
                return be.segment_softmax_backward(h.crow, h.perm, y, g, ng, False, crossing)

            def composed_fwd():
                be.segment_logsumexp(h.crow, h.perm, val, lse, ng, nnz, False, 0, ng, ng, ws)
                if own:
                    return be.segment_logsumexp_backward(val, plan.crow, ones, lse, None, None, None, ng)
                return be.segment_logsumexp_backward(val, None, None, None, plan.col, ones, lse, 0)

            y = fused_fwd()
            ref = composed_fwd()
            torch.cuda.synchronize()
            err = float(((y - ref).abs() / ref.abs().clamp(min=1e-30)).max())
            t = blocks({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd,
                        "fused_fwdbwd": lambda: (fused_fwd(), fused_bwd()),
                        "composed_fwdbwd": lambda: (composed_fwd(), fused_bwd())}, args.loops, args.reps)
            # value-sized arrays per entry (4 bytes each): fused forward val + y (+ perm, read once for both); composed val + val +
            # grad (+ perm, + the column index in the other direction); backward y + g + gin (+ perm)
            p = 0 if own else 4
            bpe = {"fused_fwd": 8 + p, "composed_fwd": 12 + p + (0 if own else 4), "bwd": 12 + p}
            line = {"shape": shape, "dim": dim, "n_groups": ng, "nnz": nnz, "crossing": crossing, "dtype": "float32", "index": "int32",
                    "max_rel_diff_fused_vs_composed": err, "bytes_per_entry": bpe,
                    "us_median_min_max": {k: list(v) for k, v in t.items()},
                    "fwd_speedup": round(t["composed_fwd"][0] / t["fused_fwd"][0], 3),
                    "fwdbwd_speedup": round(t["composed_fwdbwd"][0] / t["fused_fwdbwd"][0], 3),
                    "fused_fwd_GBps": round(bpe["fused_fwd"] * nnz / t["fused_fwd"][0] / 1e3, 1),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
