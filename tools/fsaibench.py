#!/usr/bin/env python3
"""sparse_fsai on one GPU beside sparse_ic0 and the un-preconditioned CG: one JSON line per step.

    python tools/fsaibench.py [--loops 5] [--reps 5] [--small] [--out profiles/fsai/tool_lines.jsonl]

Build time: FSAI on tril(A) and on tril(A²) on the C3 pattern (27-point stencil on 64³, truncated at the faces) and on the 7-point
Laplacian on 126³ (C4), fp32 / int32, at the backend level (`_backend.csr_fsai`: the plan is cached, the numeric build is what a
rebuild for new values costs), beside `tsgu_csr_ic0` on the same matrix in the same process, and the time of one application
M(r) = Gᵀ(G·r) with one right-hand side.

Solve time: `linear_cg` to a relative residual of 1e-4 on the C4 Laplacian and on its anisotropic variant (coefficients
1 : 1 : 1000): plain, IC(0), FSAI(A) and FSAI(A²) — iterations and host-timed wall time of one solve after a warm-up solve.  The time
of building each preconditioner (plan included, first call) is reported beside the solves, not hidden in them.

Every step is a child process of its own under a time limit, one after the other (one process has the GPU open at a time); the
first step that fails ends the run.  Build times are device-event medians (ms) over `reps` blocks of `loops` calls after warm-up
with the least and the greatest block beside them.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"build_c3": 300, "build_c4": 300, "solve_c4": 600, "solve_aniso": 600}      # step -> time limit in seconds


def blocks(torch, fn, loops, reps):
    """(median, min, max) in ms per call."""
    for _i in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _r in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _i in range(loops):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / loops)
    return [round(sorted(ts)[len(ts) // 2], 4), round(min(ts), 4), round(max(ts), 4)]


def stencil7(torch, synthetic, n1, coeff, dev):
    """−∇·(diag(coeff)∇u) on an n1³ lattice with Dirichlet faces: CSR float32 / int32."""
    crow, col = synthetic.box_stencil(n1, n1, n1, (False, False, False), 7, None, torch.int32)
    crow, col = crow.to(dev), col.to(dev)
    n = n1 ** 3
    rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    d = (col - rows).abs()
    cx, cy, cz = coeff
    val = torch.zeros(col.numel(), device=dev)
    val[d == n1 * n1] = -cx
    val[d == n1] = -cy
    val[d == 1] = -cz
    val[d == 0] = 2.0 * (cx + cy + cz)
    return torch.sparse_csr_tensor(crow, col, val, (n, n))


def build_line(torch, name, A, loops, reps):
    from torchsparsegradutils_amd import _backend, _pattern, sparse_fsai, sparse_spgemm

    n = A.size(0)
    g = _pattern.from_csr(A)
    plan = _pattern.factor_plan(g)
    lg, lpos, ldp = plan.lower()
    lval = plan.canonical_values(A.values()).index_select(0, lpos)
    cap = _backend.fsai_geometry(torch.float32)[0]
    rhs = torch.randn(n, 1, device=A.device)
    t, shape = {}, {}
    ic = lambda: _backend.csr_factor("ic0", lg.crow, lg.col, ldp, lval, n)                 # noqa: E731
    assert int(ic()[1].item()) == 0
    t["ic0"] = blocks(torch, ic, loops, reps)
    for tag, carrier in (("fsai_A", None), ("fsai_A2", sparse_spgemm(A, A))):
        M = sparse_fsai(A, pattern=carrier)                                                # (builds and caches the plan)
        sg, order = _pattern.fsai_plan(g if carrier is None else _pattern.from_csr(carrier), cap).view(lg.crow.dtype)
        run = lambda: _backend.csr_fsai(lg.crow, lg.col, lval, sg.crow, sg.col, n, order=order)      # noqa: E731
        out, info = run()
        assert int(info.item()) == 0 and torch.equal(out, M.values) and torch.equal(run()[0], out)
        t[tag] = blocks(torch, run, loops, reps)
        t[tag + "_apply_1rhs"] = blocks(torch, lambda: M(rhs), loops, reps)
        shape[tag] = {"nnz_S": int(sg.nnz), "longest_row": int((sg.crow[1:] - sg.crow[:-1]).max()), "ordered": order is not None}
    return {"case": "build", "pattern": name, "n": n, "nnz": int(g.nnz), "nnz_lower": int(lg.nnz), "dtype": "float32", "index": "int32",
            "S": shape, "ms_median_min_max": t, "fsai_A_over_ic0": round(t["fsai_A"][0] / t["ic0"][0], 4),
            "fsai_A2_over_ic0": round(t["fsai_A2"][0] / t["ic0"][0], 4), "device": torch.cuda.get_device_name(0)}


def solve_line(torch, name, A, tol, max_iter):
    from torchsparsegradutils_amd import sparse_fsai, sparse_ic0, sparse_spgemm
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    n = A.size(0)
    b = torch.randn(n, 1, device=A.device)
    res = {}
    for tag, make in (("plain", lambda: None), ("ic0", lambda: sparse_ic0(A)), ("fsai_A", lambda: sparse_fsai(A)),
                      ("fsai_A2", lambda: sparse_fsai(A, pattern=sparse_spgemm(A, A)))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pre = make()
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        run = lambda: linear_cg(A, b, tolerance=tol, eps=1e-30, stop_updating_after=1e-30, max_iter=max_iter, max_tridiag_iter=0,       # noqa: E731
                                preconditioner=pre)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run()                                                                          # warm-up solve
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = run()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        info = last_solve_info("linear_cg")
        r = torch.sparse.mm(A, x) - b
        res[tag] = {"iterations": int(info["iterations"]), "ms": round(ms, 2), "ms_per_iteration": round(ms / max(1, int(info["iterations"])), 4),
                    "true_relative_residual": float(r.norm() / b.norm()), "first_build_ms_with_plan": round(first_ms, 2)}
    for tag in ("ic0", "fsai_A", "fsai_A2"):
        res[tag]["speedup_over_plain"] = round(res["plain"]["ms"] / res[tag]["ms"], 4)
    return {"case": "solve", "problem": name, "solver": "linear_cg", "n": n, "tolerance": tol, **res, "device": torch.cuda.get_device_name(0)}


def step(name, args):
    import torch

    sys.path.insert(0, ROOT)
    from torchsparsegradutils_amd.utils import synthetic

    assert torch.cuda.is_available(), "fsaibench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n27, n7 = (12, 20) if args.small else (64, 126)
    if name == "build_c3":
        crow, col = synthetic.box_stencil(n27, n27, n27, (False, False, False), 27, None, torch.int32)
        rows = torch.repeat_interleave(torch.arange(n27 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
        val = torch.where(col == rows, torch.tensor(30.0), -torch.rand(col.numel()))    # diagonally dominant; only the lower triangle is read
        A = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n27 ** 3, n27 ** 3))
        return build_line(torch, f"C3: 27-point on {n27}^3", A, args.loops, args.reps)
    if name == "build_c4":
        return build_line(torch, f"C4: 7-point on {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev), args.loops, args.reps)
    if name == "solve_c4":
        return solve_line(torch, f"C4 Laplacian {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev), 1e-4, 2000)
    if name == "solve_aniso":
        return solve_line(torch, f"anisotropic 1:1:1000 {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1000.0), dev), 1e-4, 2000)
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="12³ / 20³ lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "fsai", "tool_lines.jsonl"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one step in this process and print its line")
    args = ap.parse_args()
    if args.step:
        print("LINE " + json.dumps(step(args.step, args)), flush=True)
        return 0
    lines = []
    for name, limit in STEPS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--loops", str(args.loops), "--reps", str(args.reps)]
        try:
            done = subprocess.run(cmd + (["--small"] if args.small else []), stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"fsaibench: step {name} exceeded its {limit} s: stopping", file=sys.stderr)
            return 124
        got = [ln[5:] for ln in done.stdout.splitlines() if ln.startswith("LINE ")]
        if done.returncode != 0 or len(got) != 1:
            print(f"fsaibench: step {name} ended with status {done.returncode}: stopping\n{done.stdout[-2000:]}", file=sys.stderr)
            return done.returncode or 1
        lines.append(got[0])
        print(got[0], flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
