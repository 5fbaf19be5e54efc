#!/usr/bin/env python3
"""sparse_mm_reduce (amax) timings on one GPU beside sparse_mm on the plan-free kernels: one JSON line per case.

    python tools/mmreducebench.py [--loops 30] [--reps 5] [--out profiles/mm_reduce/tool_lines.jsonl]

Cases: the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22 uniformly random) and the C2 pattern (27-point
periodic stencil, N = 10^6), CSR int32; fp32 with p = 32 and 64 columns, bf16 with p = 64; forward (no graph), and forward +
backward with both operands requiring a gradient, through the public functions.

Yardstick, timing: `sparse_mm` in the same process with every planned kernel family switched off (the environment below), i.e.
on the plan-free gather kernels the max / min kernels are modelled on — the same bytes except for the `arg` array.  Yardstick,
bytes: the compulsory traffic of the forward, nnz·(index + value) + (n_cols + n)·p·sizeof(value) + n·p·4, over its time.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up, the functions taking turns block by
block, with the least and the greatest block beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys

for _k in ("TSGU_ENABLE_LATTICE", "TSGU_ENABLE_MARCH", "TSGU_ENABLE_PACK", "TSGU_ENABLE_TILE"):
    os.environ[_k] = "0"          # read when the package is imported: sparse_mm stays on the plan-free kernels

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import sparse_mm, sparse_mm_reduce  # noqa: E402
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
    ap.add_argument("--loops", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mm_reduce", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mmreducebench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    n = 1 << 20
    keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
    mrow = torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True)
    million = (mrow, (keys % n).int(), n)
    crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
    c2 = (crow.to(dev), col.to(dev), crow.numel() - 1)

    lines = []
    for shape, (ptr, idx, rows) in (("million", million), ("C2", c2)):
        nnz = idx.numel()
        for dtype, p in ((torch.float32, 32), (torch.float32, 64), (torch.bfloat16, 64)):
            val = torch.randn(nnz, device=dev).to(dtype)
            A = torch.sparse_csr_tensor(ptr, idx, val, (rows, rows))
            B = torch.randn(rows, p, device=dev).to(dtype)
            G = torch.randn(rows, p, device=dev).to(dtype)
            Ag, Bg = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)

            def fwd(f):
                with torch.no_grad():
                    return f(A, B)

            def fwdbwd(f):
                Ag.grad = Bg.grad = None
                f(Ag, Bg).backward(G)

            amax = lambda a, b: sparse_mm_reduce(a, b, "amax")      # noqa: E731
            first, again = fwd(amax), fwd(amax)
            torch.cuda.synchronize()
            assert torch.equal(first, again), "two runs of the forward differ"
            t = blocks({"amax_fwd": lambda: fwd(amax), "sum_fwd": lambda: fwd(sparse_mm),
                        "amax_fwdbwd": lambda: fwdbwd(amax), "sum_fwdbwd": lambda: fwdbwd(sparse_mm)}, args.loops, args.reps)
            eb = val.element_size()
            compulsory = nnz * (4 + eb) + 2 * rows * p * eb + rows * p * 4
            line = {"shape": shape, "n": rows, "nnz": nnz, "p": p, "dtype": str(dtype).replace("torch.", ""), "index": "int32",
                    "us_median_min_max": {k: list(v) for k, v in t.items()},
                    "fwd_amax_over_sum": round(t["amax_fwd"][0] / t["sum_fwd"][0], 3),
                    "fwdbwd_amax_over_sum": round(t["amax_fwdbwd"][0] / t["sum_fwdbwd"][0], 3),
                    "compulsory_bytes_fwd": compulsory, "arg_bytes": rows * p * 4,
                    "amax_fwd_TBps_compulsory": round(compulsory / t["amax_fwd"][0] / 1e6, 3),
                    "sum_fwd_TBps_compulsory": round((compulsory - rows * p * 4) / t["sum_fwd"][0] / 1e6, 3),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
