#!/usr/bin/env python3
"""sparse_amg on one GPU beside sparse_fsai and the un-preconditioned CG: one JSON line per step.

    python tools/amgbench.py [--loops 5] [--reps 5] [--small] [--out profiles/amg/tool_lines.jsonl]

Setup time: the first call (plans, aggregation, the three products per level; host-timed, it reads the device) and `refresh` (new
values on the same pattern; device events) on the 7-point Laplacian on 126³ (C4) and on the C3 pattern (27-point stencil on 64³,
truncated at the faces), fp32 / int32, with the level sizes and the complexities.

Cycle time: one V(1, 1) cycle with one right-hand side on C4, and the share of every level (the level's own launches, timed alone
on its buffers).  Beside it the finest level's sweep x + w∘(b − A·x) done as `sparse_mm` (the stencil kernels) plus torch
elementwise ops against the one fused launch: what decides whether the finest level should go through the stencil kernels.

Solve time: `linear_cg` to a relative residual of 1e-4 on the C4 Laplacian and on its anisotropic variant (coefficients
1 : 1 : 1000, theta = 0.08): plain, FSAI(A) and AMG in the same process — iterations and host-timed wall time of one solve after a
warm-up solve; the time of building each preconditioner is reported beside the solves, not hidden in them.

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
STEPS = {"setup_c4": 300, "setup_c3": 300, "cycle_c4": 300, "solve_c4": 600, "solve_aniso": 600}      # step -> time limit in seconds


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


def stencil27(torch, synthetic, n1, dev):
    crow, col = synthetic.box_stencil(n1, n1, n1, (False, False, False), 27, None, torch.int32)
    rows = torch.repeat_interleave(torch.arange(n1 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    val = torch.where(col == rows, torch.tensor(26.0), torch.tensor(-1.0))
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n1 ** 3, n1 ** 3))


def first_build(torch, make):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M = make()
    torch.cuda.synchronize()
    return M, round((time.perf_counter() - t0) * 1e3, 2)


def setup_line(torch, name, A, theta, loops, reps):
    from torchsparsegradutils_amd import sparse_amg

    M, first_ms = first_build(torch, lambda: sparse_amg(A, theta=theta))
    again = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values() * 1.5, A.shape)
    refresh = blocks(torch, lambda: M.refresh(again), max(1, loops // 2), reps)
    return {"case": "setup", "pattern": name, "n": A.size(0), "nnz": int(A.values().numel()), "dtype": "float32", "index": "int32",
            "theta": theta, "levels": list(M.levels), "operator_complexity": round(M.operator_complexity, 4),
            "grid_complexity": round(M.grid_complexity, 4), "first_call_ms_with_plans": first_ms, "refresh_ms_median_min_max": refresh,
            "device": torch.cuda.get_device_name(0)}


def level_ops(torch, M, l, bufs, affine):
    """The launches of level l of one cycle, without the levels below, on the level's own buffers."""
    lv = M._levels[l]
    xa, xb, r, b = bufs[l]
    s = M._sweeps
    if l == len(M._levels) - 1:
        if lv.solver == "dense":
            return lambda: torch.mm(lv.inv, b, out=xa)

        def coarse():
            torch.mul(lv.w.unsqueeze(1), b, out=xa)
            M._smooth(lv, b, xa, xb, 2 * s - 1, affine)
        return coarse
    rc, e = bufs[l + 1][3], bufs[l + 1][0]

    def ops():
        torch.mul(lv.w.unsqueeze(1), b, out=xa)
        x, y = M._smooth(lv, b, xa, xb, s - 1, affine)
        affine(lv.ptr, lv.idx, lv.val, x, lv.n, lv.n, B=b, out=r)
        affine(lv.p_t.crow, lv.p_t.col, lv.pt_val, r, lv.n_c, lv.n, alpha=-1.0, out=rc)
        affine(lv.p_ptr, lv.p_idx, lv.p_val, e, lv.n, lv.n_c, C=x, alpha=-1.0, out=x)
        M._smooth(lv, b, x, y, s, affine)
    return ops


def cycle_line(torch, name, A, loops, reps):
    from torchsparsegradutils_amd import _backend, sparse_amg, sparse_mm

    M = sparse_amg(A)
    n = A.size(0)
    rhs = torch.randn(n, 1, device=A.device)
    whole = blocks(torch, lambda: M(rhs), loops, reps)
    bufs = M._work(1, rhs.dtype)
    for level in bufs:
        for t in level:
            t.normal_()
    per_level = [blocks(torch, level_ops(torch, M, l, bufs, _backend.csr_affine_spmm), loops, reps) for l in range(len(M.levels))]
    total = sum(t[0] for t in per_level)
    lv = M._levels[0]
    x, b, out = (torch.randn(n, 1, device=A.device) for _ in range(3))
    w = lv.w.unsqueeze(1)
    fused = blocks(torch, lambda: _backend.csr_affine_spmm(lv.ptr, lv.idx, lv.val, x, n, n, C=x, B=b, w=lv.w, out=out), loops, reps)
    composed = blocks(torch, lambda: torch.addcmul(x, w, b - sparse_mm(A, x), out=out), loops, reps)
    product = blocks(torch, lambda: sparse_mm(A, x), loops, reps)
    s = M._sweeps
    launches = [1 if l == len(M.levels) - 1 else 3 + 2 * s for l in range(len(M.levels))]
    return {"case": "cycle", "pattern": name, "n": n, "rhs": 1, "sweeps": s, "levels": [lv["n"] for lv in M.levels],
            "cycle_ms_median_min_max": whole, "per_level_ms_median_min_max": per_level,
            "per_level_share": [round(t[0] / total, 4) for t in per_level], "launches_per_level": launches,
            "fine_sweep_fused_ms": fused, "fine_sweep_sparse_mm_plus_torch_ms": composed, "fine_sparse_mm_alone_ms": product,
            "device": torch.cuda.get_device_name(0)}


def solve_line(torch, name, A, theta, tol, max_iter):
    from torchsparsegradutils_amd import sparse_amg, sparse_fsai
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    n = A.size(0)
    b = torch.randn(n, 1, device=A.device)
    res = {}
    for tag, make in (("plain", lambda: None), ("fsai_A", lambda: sparse_fsai(A)), ("amg", lambda: sparse_amg(A, theta=theta))):
        pre, first_ms = first_build(torch, make)
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
                    "true_relative_residual": float(r.norm() / b.norm()), "first_build_ms_with_plan": first_ms}
        if tag == "amg":
            again = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values() * 1.5, A.shape)
            res[tag]["refresh_ms_median_min_max"] = blocks(torch, lambda: pre.refresh(again), 2, 3)
            res[tag]["levels"] = [lv["n"] for lv in pre.levels]
            res[tag]["operator_complexity"] = round(pre.operator_complexity, 4)
    for tag in ("fsai_A", "amg"):
        res[tag]["speedup_over_plain"] = round(res["plain"]["ms"] / res[tag]["ms"], 4)
    return {"case": "solve", "problem": name, "solver": "linear_cg", "n": n, "tolerance": tol, "theta": theta, **res,
            "device": torch.cuda.get_device_name(0)}


def step(name, args):
    import torch

    sys.path.insert(0, ROOT)
    from torchsparsegradutils_amd.utils import synthetic

    assert torch.cuda.is_available(), "amgbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n27, n7 = (12, 20) if args.small else (64, 126)
    if name == "setup_c4":
        return setup_line(torch, f"C4: 7-point on {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev), 0.0, args.loops, args.reps)
    if name == "setup_c3":
        return setup_line(torch, f"C3: 27-point on {n27}^3", stencil27(torch, synthetic, n27, dev), 0.0, args.loops, args.reps)
    if name == "cycle_c4":
        return cycle_line(torch, f"C4: 7-point on {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev), args.loops, args.reps)
    if name == "solve_c4":
        return solve_line(torch, f"C4 Laplacian {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1.0), dev), 0.0, 1e-4, 2000)
    if name == "solve_aniso":
        return solve_line(torch, f"anisotropic 1:1:1000 {n7}^3", stencil7(torch, synthetic, n7, (1.0, 1.0, 1000.0), dev), 0.08, 1e-4, 2000)
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="12³ / 20³ lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "amg", "tool_lines.jsonl"))
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
            print(f"amgbench: step {name} exceeded its {limit} s: stopping", file=sys.stderr)
            return 124
        got = [ln[5:] for ln in done.stdout.splitlines() if ln.startswith("LINE ")]
        if done.returncode != 0 or len(got) != 1:
            print(f"amgbench: step {name} ended with status {done.returncode}: stopping\n{done.stdout[-2000:]}", file=sys.stderr)
            return done.returncode or 1
        lines.append(got[0])
        print(got[0], flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
