#!/usr/bin/env python3
"""sparse_lobpcg on one GPU beside torch.lobpcg: one JSON line per step.

    python tools/lobpcgbench.py [--k 4 16 32] [--niter 200] [--small] [--no-torch] [--out profiles/lobpcg/tool_lines.jsonl]

Problems: the 7-point Laplacian on 126³ with Dirichlet faces (C4) and the C3 pattern (27-point stencil on 64³, truncated at the
faces, diagonally dominant values), fp32 / int32 CSR.  For every k, for the smallest and the largest pairs, with no preconditioner
and (smallest pairs only: FSAI approximates A⁻¹) with `sparse_fsai(A)`: iterations to the default tolerance sqrt(eps)·‖A‖_est or the
`--niter` cap, wall time of the solve after a warm-up solve of a few iterations, ms per iteration, and its split into the sparse
product A·W (device-event median of the product alone at the same width) and the rest — the dense part on the tall-skinny
kernels, the preconditioner and the host's Rayleigh–Ritz step.  The same initial block then goes to `torch.lobpcg` on the COO
operand (method "ortho", the same tolerance and cap) as the comparison.  Nothing here is asserted anywhere.

Every step is a child process of its own under a time limit, one after the other (one process has the GPU open at a time); the
first step that fails ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"c4": 900, "c3": 900}      # step -> time limit in seconds


def product_ms(torch, A, k, reps=7):
    from torchsparsegradutils_amd import sparse_mm

    W = torch.randn(A.size(0), k, device=A.device)
    for _i in range(6):
        sparse_mm(A, W)
    torch.cuda.synchronize()
    ts = []
    for _r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _i in range(5):
            sparse_mm(A, W)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / 5)
    return sorted(ts)[len(ts) // 2]


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def problem_lines(torch, name, A, ks, niter, with_torch):
    from torchsparsegradutils_amd import sparse_fsai, sparse_lobpcg
    from torchsparsegradutils_amd.utils import last_solve_info

    n = A.size(0)
    coo = A.to_sparse_coo().coalesce() if with_torch else None
    fsai, fsai_ms = timed(torch, lambda: sparse_fsai(A))
    lines = []
    for k in ks:
        X = torch.randn(n, k, device=A.device)
        spmm = product_ms(torch, A, k)
        for largest in (False, True):
            res = {}
            for tag, pre in (("none", None), ("fsai", fsai)):
                if largest and pre is not None:
                    continue
                run = lambda it: sparse_lobpcg(A, k, X=X, preconditioner=pre, niter=it, largest=largest)     # noqa: E731,B023
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    run(4)                                                                  # warm-up: plans, pinned buffers
                    (lam, V), ms = timed(torch, lambda: run(niter))
                info = last_solve_info("lobpcg")
                its = max(1, int(info["iterations"]))
                r = torch.sparse.mm(A, V) - V * lam
                res[tag] = {"iterations": int(info["iterations"]), "converged": bool(info["converged"]), "restarts": int(info["restarts"]),
                            "ms": round(ms, 2), "ms_per_iteration": round(ms / its, 4), "ms_product": round(spmm, 4),
                            "ms_rest": round(ms / its - spmm, 4), "max_residual_over_a_norm": float(r.norm(dim=0).max() / info["a_norm"]),
                            "eigenvalues": [float(x) for x in lam[: min(k, 4)]]}
            if with_torch:
                tol = float(torch.finfo(torch.float32).eps) ** 0.5
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    torch.lobpcg(coo, k=k, X=X, niter=4, tol=tol, largest=largest, method="ortho")
                    count = {}
                    (tl, tv), ms = timed(torch, lambda: torch.lobpcg(coo, k=k, X=X, niter=niter, tol=tol, largest=largest, method="ortho",
                                                                     tracker=lambda w: count.__setitem__("it", int(w.ivars["istep"]))))
                its = max(1, count.get("it", niter))
                r = torch.sparse.mm(A, tv) - tv * tl
                res["torch_lobpcg"] = {"iterations": its, "ms": round(ms, 2), "ms_per_iteration": round(ms / its, 4),
                                       "max_residual_over_a_norm": float(r.norm(dim=0).max() / info["a_norm"]),
                                       "eigenvalues": [float(x) for x in tl[: min(k, 4)]]}
            lines.append({"case": "lobpcg", "problem": name, "n": n, "k": k, "largest": largest, "niter_cap": niter, "dtype": "float32",
                          "index": "int32", "fsai_build_ms_with_plan": round(fsai_ms, 2), **res, "device": torch.cuda.get_device_name(0)})
    return lines


def step(name, args):
    import torch

    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from fsaibench import stencil7
    from torchsparsegradutils_amd.utils import synthetic

    assert torch.cuda.is_available(), "lobpcgbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n27, n7 = (12, 20) if args.small else (64, 126)
    if name == "c4":
        A = stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev)
        return problem_lines(torch, f"C4 Laplacian {n7}^3", A, args.k, args.niter, not args.no_torch)
    if name == "c3":
        crow, col = synthetic.box_stencil(n27, n27, n27, (False, False, False), 27, None, torch.int32)
        rows = torch.repeat_interleave(torch.arange(n27 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
        val = torch.where(col == rows, torch.tensor(30.0), torch.tensor(-1.0))             # symmetric, diagonally dominant
        A = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n27 ** 3, n27 ** 3))
        return problem_lines(torch, f"C3: 27-point on {n27}^3", A, args.k, args.niter, not args.no_torch)
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[4, 16, 32])
    ap.add_argument("--niter", type=int, default=200, help="iteration cap of every solve")
    ap.add_argument("--small", action="store_true", help="12³ / 20³ lattices: a check of the tool, not a measurement")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch.lobpcg comparison out")
    ap.add_argument("--problems", nargs="+", choices=sorted(STEPS), default=sorted(STEPS, reverse=True))
    ap.add_argument("--out", default=os.path.join("profiles", "lobpcg", "tool_lines.jsonl"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its lines")
    args = ap.parse_args()
    if args.step:
        for line in step(args.step, args):
            print("LINE " + json.dumps(line), flush=True)
        return 0
    lines = []
    for name in args.problems:
        limit = STEPS[name]
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--niter", str(args.niter), "--k", *map(str, args.k)]
        cmd += (["--small"] if args.small else []) + (["--no-torch"] if args.no_torch else [])
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"lobpcgbench: step {name} exceeded its {limit} s: stopping", file=sys.stderr)
            return 124
        got = [ln[5:] for ln in done.stdout.splitlines() if ln.startswith("LINE ")]
        if done.returncode != 0 or not got:
            print(f"lobpcgbench: step {name} ended with status {done.returncode}: stopping\n{done.stdout[-2000:]}", file=sys.stderr)
            return done.returncode or 1
        lines += got
        print("\n".join(got), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
