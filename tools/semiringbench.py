#!/usr/bin/env python3
"""sparse_semiring_mm timings on one GPU beside its composition from torch ops and beside sparse_mm: one JSON line per case.

    python tools/semiringbench.py [--loops 20] [--reps 5] [--out profiles/semiring/tool_lines.jsonl]

Cases: the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22 uniformly random) and the C2 pattern (27-point periodic
stencil, N = 10^6), CSR int32, fp32 with p = 32 and 64 columns; the log and max_plus semirings; forward (no graph), and forward +
backward with both operands requiring a gradient.

Beside the fused op, in the same run and taking turns block by block:
  * the composition a user writes today — `val[:, None] + B[col]` (nnz × p), a segmented reduction over it (`scatter_reduce` amax;
    for log also exp, `index_add` and log), torch autograd through it — with the peak memory of both;
  * `sparse_mm` with every planned kernel family switched off (the environment below), i.e. on the plan-free gather kernels the
    semiring kernels are modelled on: the floor of the gathers.
`exp_per_us` is nnz·p over the fused log forward's time: the rate of exp evaluations the kernel sustains, to hold against its
bytes (`fwd_TBps_compulsory`: nnz·(index + value) + (n_cols + n)·p·sizeof(value) over the time).

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up (the composition: a fifth of the loops), with
the least and the greatest block beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys

for _k in ("TSGU_ENABLE_LATTICE", "TSGU_ENABLE_MARCH", "TSGU_ENABLE_PACK", "TSGU_ENABLE_TILE"):
    os.environ[_k] = "0"          # read when the package is imported: sparse_mm stays on the plan-free kernels

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import sparse_mm, sparse_semiring_mm  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in us per call; the functions take turns block by block.  fns: name -> (fn, loops divisor)."""
    for fn, _ in fns.values():
        for _i in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _r in range(reps):
        for k, (fn, div) in fns.items():
            n = max(1, loops // div)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(n):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / n)
    return {k: (round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)) for k, v in ts.items()}


def composed(rows_of, col, n, semiring):
    """The op from torch ops: an nnz × p gather + add, a segmented reduction, autograd through both."""
    def f(A, B):
        T = A.values().unsqueeze(1) + B.index_select(0, col)
        idx = rows_of.unsqueeze(1).expand_as(T)
        M = torch.full((n, B.size(1)), float("-inf"), device=B.device, dtype=B.dtype).scatter_reduce(0, idx, T, "amax", include_self=True)
        if semiring != "log":
            return M
        Md = M.detach()
        S = torch.zeros_like(Md).index_add_(0, rows_of, torch.exp(T - Md.index_select(0, rows_of)))
        return torch.log(S) + Md
    return f


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "semiring", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "semiringbench needs an MI355X"
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
        rows_of = torch.repeat_interleave(torch.arange(rows, device=dev), (ptr[1:] - ptr[:-1]).long())
        col64 = idx.long()
        for p in (32, 64):
            val = torch.randn(nnz, device=dev)
            A = torch.sparse_csr_tensor(ptr, idx, val, (rows, rows))
            B, G = torch.randn(rows, p, device=dev), torch.randn(rows, p, device=dev)
            Ag, Bg = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)

            def fwd(f):
                with torch.no_grad():
                    return f(A, B)

            def fwdbwd(f):
                Ag.grad = Bg.grad = None
                f(Ag, Bg).backward(G)

            for semiring in ("log", "max_plus"):
                fused = lambda a, b: sparse_semiring_mm(a, b, semiring)      # noqa: E731
                comp = composed(rows_of, col64, rows, semiring)
                first, again = fwd(fused), fwd(fused)
                torch.cuda.synchronize()
                assert torch.equal(first, again), "two runs of the forward differ"
                err = float((first - fwd(comp)).abs().max())
                t = blocks({"fused_fwd": (lambda: fwd(fused), 1), "composed_fwd": (lambda: fwd(comp), 5),
                            "sum_fwd": (lambda: fwd(sparse_mm), 1), "fused_fwdbwd": (lambda: fwdbwd(fused), 1),
                            "composed_fwdbwd": (lambda: fwdbwd(comp), 5), "sum_fwdbwd": (lambda: fwdbwd(sparse_mm), 1)},
                           args.loops, args.reps)
                mem = {k: peak(f) for k, f in (("fused_fwdbwd", lambda: fwdbwd(fused)), ("composed_fwdbwd", lambda: fwdbwd(comp)))}
                compulsory = nnz * 8 + 2 * rows * p * 4
                line = {"shape": shape, "n": rows, "nnz": nnz, "p": p, "dtype": "float32", "index": "int32", "semiring": semiring,
                        "us_median_min_max": {k: list(v) for k, v in t.items()},
                        "fwd_composed_over_fused": round(t["composed_fwd"][0] / t["fused_fwd"][0], 2),
                        "fwdbwd_composed_over_fused": round(t["composed_fwdbwd"][0] / t["fused_fwdbwd"][0], 2),
                        "fwd_fused_over_sum": round(t["fused_fwd"][0] / t["sum_fwd"][0], 3),
                        "fwdbwd_fused_over_sum": round(t["fused_fwdbwd"][0] / t["sum_fwdbwd"][0], 3),
                        "peak_bytes_fwdbwd": mem, "compulsory_bytes_fwd": compulsory,
                        "fwd_TBps_compulsory": round(compulsory / t["fused_fwd"][0] / 1e6, 3),
                        "exp_per_us": round(nnz * p / t["fused_fwd"][0]) if semiring == "log" else None,
                        "max_abs_diff_fused_composed": err, "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
