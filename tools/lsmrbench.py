#!/usr/bin/env python3
"""`lsmr` on the fused kernels beside the host-driven loop (`ENABLE_FUSED = False`), on one GPU: one JSON line per case.

    python tools/lsmrbench.py [--reps 5] [--small] [--out profiles/lsmr/tool_lines.jsonl]

Problems, fp32, k = 1 and 16 right-hand sides:
  stencil   [A; I] with A the 7-point stencil of tools/factorbench.py on 64^3 (singular values in [1, 12.05]: well conditioned)
  random    a (3n, n) pattern with 8 random entries per row, n = 100 000
Per line: a solve to the default tolerances (time to solution, iterations, ms per iteration) and a run of exactly 50 iterations
(atol = btol = conlim = 0: no test can stop it; ms per iteration without the set-up's share), both paths in the same run taking
turns, host-timed around a synchronise, medians of `reps` blocks after a warm-up of each; and `sparse_generic_lstsq` forward +
backward (three LSMR runs) the same way.  There are no thresholds."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from factorbench import stencil7  # noqa: E402
from torchsparsegradutils_amd import sparse_generic_lstsq  # noqa: E402
from torchsparsegradutils_amd.utils import _graph, last_solve_info, lsmr  # noqa: E402

lsmr_mod = sys.modules[lsmr.__module__]
FIXED = 50


def stencil_tall(n1, dev):
    A = stencil7(n1, (1.0, 1.0, 1.0), dev=dev).to_sparse_coo().coalesce()
    n = A.shape[0]
    eye = torch.arange(n, device=dev)
    idx = torch.cat([A.indices(), torch.stack([eye + n, eye])], dim=1)
    return torch.sparse_coo_tensor(idx, torch.cat([A.values(), torch.ones(n, device=dev)]), (2 * n, n)).coalesce().to_sparse_csr()


def random_tall(n, per_row, dev):
    m = 3 * n
    rows = torch.arange(m, device=dev).repeat_interleave(per_row)
    cols = torch.randint(0, n, (m * per_row,), device=dev)
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.randn(m * per_row, device=dev), (m, n)).coalesce().to_sparse_csr()


def turns(fns, reps):
    """Median ms of each of `fns`, called in turn `reps` times after one warm-up each."""
    times = [[] for _ in fns]
    for r in range(reps + 1):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                times[i].append((time.perf_counter() - t0) * 1e3)
    return [round(sorted(t)[len(t) // 2], 3) for t in times]


def path(fused, fn):
    def run():
        lsmr_mod.ENABLE_FUSED = fused
        try:
            return fn()
        finally:
            lsmr_mod.ENABLE_FUSED = True
    return run


def lines_for(problem, A, k, reps):
    dev = A.device
    b = torch.randn(A.shape[0], k, device=dev)
    its = {}
    for fused in (True, False):
        path(fused, lambda: lsmr(A, b))()
        its[fused] = last_solve_info("lsmr")["iterations"]
    solve = turns([path(True, lambda: lsmr(A, b)), path(False, lambda: lsmr(A, b))], reps)
    fixed_kw = dict(atol=0.0, btol=0.0, conlim=0.0, maxiter=FIXED)
    fixed = turns([path(True, lambda: lsmr(A, b, **fixed_kw)), path(False, lambda: lsmr(A, b, **fixed_kw))], reps)
    yield ({"case": "lsmr", "problem": problem, "shape": list(A.shape), "nnz": int(A.values().numel()), "k": k, "dtype": "float32",
                "iterations": {"fused": its[True], "host_loop": its[False]},
                "solve_ms": {"fused": solve[0], "host_loop": solve[1]},
                "solve_ms_per_iteration": {"fused": round(solve[0] / max(its[True], 1), 4), "host_loop": round(solve[1] / max(its[False], 1), 4)},
                f"fixed_{FIXED}_iterations_ms_per_iteration": {"fused": round(fixed[0] / FIXED, 4), "host_loop": round(fixed[1] / FIXED, 4)},
                "speedup_time_to_solution": round(solve[1] / solve[0], 3), "speedup_per_iteration": round(fixed[1] / fixed[0], 3),
                "graph_min_iters": _graph.MIN_ITERS, "reps": reps, "device": torch.cuda.get_device_name(0)})

    def train():
        Ag = A.detach().clone().requires_grad_(True)      # a leaf: its gradient arrives on A's pattern
        bg = b.clone().requires_grad_(True)
        sparse_generic_lstsq(Ag, bg).square().sum().backward()
    step = turns([path(True, train), path(False, train)], reps)
    yield ({"case": "sparse_generic_lstsq forward + backward", "problem": problem, "k": k, "ms": {"fused": step[0], "host_loop": step[1]},
                "speedup": round(step[1] / step[0], 3), "reps": reps, "device": torch.cuda.get_device_name(0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 12^3 lattice and n = 2000: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "lsmr", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lsmrbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n1, n = (12, 2000) if args.small else (64, 100_000)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    lines = []
    for problem, A in ((f"[stencil7; I] on {n1}^3", stencil_tall(n1, dev)), (f"random (3n, n), 8 per row, n = {n}", random_tall(n, 8, dev))):
        for k in (1, 16):
            for line in lines_for(problem, A, k, args.reps):
                lines.append(line)
                print(json.dumps(line), flush=True)
                with open(args.out, "w") as f:  # rewritten after every case: a run that is cut short leaves what it measured
                    for done in lines:
                        f.write(json.dumps(done) + "\n")


if __name__ == "__main__":
    main()
