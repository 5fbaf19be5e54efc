#!/usr/bin/env python3
"""sparse_coloring, the coloured sparse_ilu0 / sparse_ic0 and sparse_sgs on one GPU beside the natural ordering and the package's
other preconditioners: one JSON line per case.

    python tools/colorbench.py [--loops 5] [--reps 5] [--small] [--out profiles/coloring/tool_lines.jsonl]

Colouring: the time of the greedy colouring (rounds of `tsgu_csr_color_round` with their host polls; the plan's torch ops are
reported beside it) and the number of colours on C3 (27-point stencil on 64³, truncated at the faces) and C4 (7-point Laplacian on
126³), fp32 / int32.

Factor and application, on both shapes and in ONE run: ILU(0) and IC(0) at the backend level (`_backend.csr_factor`) on the natural
and on the permuted pattern — the kernel is the same, only the dependency graph differs — and one application (one right-hand
side) of the natural factors (two sync-free sweeps, each followed by the host's look at the error word), of the coloured factors
and of SGS (2 · n_colors wait-free launches).

Krylov: `linear_cg` to 1e-4 on the C4 Laplacian and on its 1:1:1000 variant with no preconditioner, `sparse_fsai`, `sparse_amg`,
natural IC(0), coloured IC(0) with the greedy colours, coloured IC(0) with red-black colours given through `colors=`, and SGS;
`gmres(30)` and `bicgstab` on convection–diffusion (7-point, first-order upwind along z) at cell Péclet numbers 2 and 20 with no
preconditioner, natural ILU(0) and coloured ILU(0).  Every line names the fastest entry of its problem: where the coloured
preconditioners lose to the plain loop, to FSAI or to AMG, the line says so.

Times are device-event medians (ms) over `reps` blocks of `loops` calls after warm-up with the least and the greatest block beside
them; the Krylov solves are host-timed once each after a warm-up solve.
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import (_backend, _pattern, sparse_amg, sparse_coloring, sparse_fsai, sparse_ic0, sparse_ilu0,  # noqa: E402
                                      sparse_sgs)
from torchsparsegradutils_amd.utils import (BICGSTABSettings, GMRESSettings, bicgstab, gmres, last_solve_info, linear_cg,  # noqa: E402
                                            synthetic)
from tools.factorbench import blocks, stencil7  # noqa: E402


def device_name():
    return torch.cuda.get_device_name(0)


def coloring_and_application_lines(name, A, loops, reps):
    dev, n = A.device, A.size(0)
    g = _pattern.from_csr(A)
    colour = blocks(lambda: _pattern.greedy_colors(g), 1, reps)

    def plan_from_scratch():
        g.core.own.pop("coloring", None)
        return _pattern.coloring_plan(g)

    plan_ms = blocks(plan_from_scratch, 1, reps)
    plan = _pattern.coloring_plan(g)
    sizes = [plan.offsets[c + 1] - plan.offsets[c] for c in range(plan.n_colors)]
    lines = [{"case": "colouring", "pattern": name, "n": n, "nnz": int(g.nnz), "n_colors": plan.n_colors,
              "class_rows_min_max": [min(sizes), max(sizes)], "colouring_ms_median_min_max": colour,
              "whole_plan_ms_median_min_max": plan_ms, "index": "int32", "device": device_name()}]

    nat = _pattern.factor_plan(g)
    val = nat.canonical_values(A.values())
    lg, lpos, ldp = nat.lower()
    col = plan.factor
    pval = A.values().index_select(0, plan.pos)
    plg, plpos, pldp = col.lower()
    t = {"ilu0_natural": blocks(lambda: _backend.csr_factor("ilu0", g.crow, g.col, nat.diag_pos, val, n), loops, reps),
         "ilu0_coloured": blocks(lambda: _backend.csr_factor("ilu0", col.gather.crow, col.gather.col, col.diag_pos, pval, n), loops, reps),
         "ic0_natural": blocks(lambda: _backend.csr_factor("ic0", lg.crow, lg.col, ldp, val.index_select(0, lpos), n), loops, reps),
         "ic0_coloured": blocks(lambda: _backend.csr_factor("ic0", plg.crow, plg.col, pldp, pval.index_select(0, plpos), n), loops, reps)}
    lines.append({"case": "factor", "pattern": name, "n": n, "n_colors": plan.n_colors, "dtype": "float32", "index": "int32",
                  "ms_median_min_max": t, "ilu0_coloured_over_natural": round(t["ilu0_coloured"][0] / t["ilu0_natural"][0], 3),
                  "ic0_coloured_over_natural": round(t["ic0_coloured"][0] / t["ic0_natural"][0], 3), "device": device_name()})

    r = torch.randn(n, 1, device=dev)
    objects = {"ilu0_natural": sparse_ilu0(A), "ilu0_coloured": sparse_ilu0(A, ordering="multicolor"), "ic0_natural": sparse_ic0(A),
               "ic0_coloured": sparse_ic0(A, ordering="multicolor"), "sgs": sparse_sgs(A)}
    t = {k: blocks(lambda M=M: M(r), loops, reps) for k, M in objects.items()}
    t["sparse_mm_1rhs"] = blocks(lambda: torch.sparse.mm(A, r), loops, reps)
    lines.append({"case": "application", "pattern": name, "n": n, "n_colors": plan.n_colors, "launches_per_coloured_application": 2 * plan.n_colors,
                  "right_hand_sides": 1, "dtype": "float32", "index": "int32", "ms_median_min_max": t,
                  "ilu0_natural_over_coloured": round(t["ilu0_natural"][0] / t["ilu0_coloured"][0], 1),
                  "ic0_natural_over_coloured": round(t["ic0_natural"][0] / t["ic0_coloured"][0], 1),
                  "coloured_ic0_in_products": round(t["ic0_coloured"][0] / t["sparse_mm_1rhs"][0], 2),
                  "sgs_in_products": round(t["sgs"][0] / t["sparse_mm_1rhs"][0], 2), "device": device_name()})
    return lines


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = fn()
    torch.cuda.synchronize()
    return x, (time.perf_counter() - t0) * 1e3


def first_build(make):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    M = make()
    torch.cuda.synchronize()
    return M, round((time.perf_counter() - t0) * 1e3, 2)


def verdict(res):
    best = min(res, key=lambda k: res[k]["ms"])
    coloured = [k for k in res if k.startswith("coloured") or k == "sgs"]
    best_coloured = min(coloured, key=lambda k: res[k]["ms"])
    return {"fastest": best, "fastest_coloured": best_coloured,
            "fastest_coloured_over_fastest": round(res[best_coloured]["ms"] / res[best]["ms"], 3),
            "coloured_wins": best == best_coloured}


def cg_line(name, A, n1, theta, tol, max_iter):
    n = A.size(0)
    b = torch.randn(n, 1, device=A.device)
    i = torch.arange(n, device=A.device)
    red_black = ((i // (n1 * n1)) + (i // n1) % n1 + i % n1) % 2
    makers = (("plain", lambda: None), ("fsai", lambda: sparse_fsai(A)), ("amg", lambda: sparse_amg(A, theta=theta)),
              ("natural_ic0", lambda: sparse_ic0(A)), ("coloured_ic0_greedy", lambda: sparse_ic0(A, ordering="multicolor")),
              ("coloured_ic0_red_black", lambda: sparse_ic0(A, ordering=sparse_coloring(A, colors=red_black))),
              ("sgs", lambda: sparse_sgs(A)))
    res = {}
    for tag, make in makers:
        M, build_ms = first_build(make)
        run = lambda: linear_cg(A, b, tolerance=tol, eps=1e-30, stop_updating_after=1e-30, max_iter=max_iter, max_tridiag_iter=0,       # noqa: E731
                                preconditioner=M)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, ms = timed(run)
        its = int(last_solve_info("linear_cg")["iterations"])
        res[tag] = {"iterations": its, "ms": round(ms, 2), "ms_per_iteration": round(ms / max(its, 1), 4), "first_build_ms_with_plan": build_ms,
                    "true_relative_residual": float((torch.sparse.mm(A, x) - b).norm() / b.norm())}
        if hasattr(M, "coloring"):
            res[tag]["n_colors"] = M.coloring.n_colors
    return {"case": "krylov", "problem": name, "solver": "linear_cg", "n": n, "tolerance": tol, **res, **verdict(res), "device": device_name()}


def nonsymmetric_lines(name, A, tol, max_iter):
    n = A.size(0)
    b = torch.randn(n, 1, device=A.device)
    built = {"plain": (None, 0.0)}
    built["natural_ilu0"] = first_build(lambda: sparse_ilu0(A))
    built["coloured_ilu0"] = first_build(lambda: sparse_ilu0(A, ordering="multicolor"))
    lines = []
    for solver in ("gmres(30)", "bicgstab"):
        res = {}
        for tag, (M, build_ms) in built.items():
            if solver == "bicgstab":
                run = lambda: bicgstab(A, b, settings=BICGSTABSettings(reltol=tol, abstol=0.0, matvec_max=2 * max_iter, precon=M))      # noqa: E731
                its = lambda: 2 * int(last_solve_info("bicgstab")["iterations_enqueued"])                                             # noqa: E731
            else:
                run = lambda: gmres(A, b, settings=GMRESSettings(restart=30, reltol=tol, abstol=0.0, maxiter=max_iter, precon=M))       # noqa: E731
                its = lambda: int(last_solve_info("gmres")["iterations"].max())                                                       # noqa: E731
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                x, ms = timed(run)
            k = its()
            res[tag] = {"products_with_A": k, "ms": round(ms, 2), "ms_per_product": round(ms / max(k, 1), 4), "first_build_ms_with_plan": build_ms,
                        "true_relative_residual": float((torch.sparse.mm(A, x) - b).norm() / b.norm())}
        res["coloured_ilu0"]["n_colors"] = built["coloured_ilu0"][0].coloring.n_colors
        lines.append({"case": "krylov", "problem": name, "solver": solver, "n": n, "tolerance": tol, **res, **verdict(res),
                      "natural_over_coloured_ms": round(res["natural_ilu0"]["ms"] / res["coloured_ilu0"]["ms"], 2), "device": device_name()})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="12³ / 20³ lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "coloring", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "colorbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n27, n7 = (12, 20) if args.small else (64, 126)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    out = open(args.out, "w")

    def emit(lines):
        for line in lines if isinstance(lines, list) else [lines]:
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
            out.flush()

    crow, col = synthetic.box_stencil(n27, n27, n27, (False, False, False), 27, None, torch.int32)
    rows = torch.repeat_interleave(torch.arange(n27 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    val = torch.where(col == rows, torch.tensor(30.0), -torch.rand(col.numel()))        # diagonally dominant, symmetric in its pattern
    C3 = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n27 ** 3, n27 ** 3))
    emit(coloring_and_application_lines(f"C3: 27-point on {n27}^3", C3, args.loops, args.reps))
    del C3
    lap = stencil7(n7, (1.0, 1.0, 1.0), dev=dev)
    emit(coloring_and_application_lines(f"C4: 7-point on {n7}^3", lap, args.loops, args.reps))
    emit(cg_line(f"C4 Laplacian {n7}^3", lap, n7, 0.0, 1e-4, 2000))
    del lap
    emit(cg_line(f"anisotropic 1:1:1000 {n7}^3", stencil7(n7, (1.0, 1.0, 1000.0), dev=dev), n7, 0.08, 1e-4, 2000))
    for peclet in (2.0, 20.0):
        emit(nonsymmetric_lines(f"convection-diffusion {n7}^3, cell Peclet {peclet:g}",
                                stencil7(n7, (1.0, 1.0, 1.0), convection=peclet, dev=dev), 1e-4, 2000))
    out.close()


if __name__ == "__main__":
    main()
