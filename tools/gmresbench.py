#!/usr/bin/env python3
"""`gmres` beside `bicgstab` on one GPU, and what the Arnoldi kernels cost: one JSON line per case.

    python tools/gmresbench.py [--loops 5] [--reps 5] [--small] [--out profiles/gmres/tool_lines.jsonl]

Problems: the convection-diffusion stencil of tools/factorbench.py (7-point on 126^3, first-order upwind convection along z with
cell Peclet number 2) and its Peclet-20 variant, fp32 / int32, one right-hand side, to a relative residual of 1e-4.  Solvers, all
in the same run: `bicgstab`, `gmres(30)`, `gmres(30)` with `sparse_fsai(A)`, with `sparse_ilu0(A)`, and flexible `gmres(30)` with
`sparse_amg(A)` where it builds.  Per line: iterations (inner steps = products with A), ms per solve (host-timed once after a
warm-up solve, as factorbench does: the loops synchronise per chunk anyway), ms per inner step, and the true relative residual.

Kernel lines: one restart cycle's worth of orthogonalisation launches (for k = 1 ... 30: two projections and two subtractions) as
device-event medians over `reps` blocks of `loops` cycles, the bytes they move (a projection reads k + 1 blocks, a subtraction
reads k + 1 and writes one) against the copy rate of the library's own streaming copy measured in the same run, and the share of
an un-preconditioned inner step they are.  There are no thresholds.
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from factorbench import blocks, stencil7  # noqa: E402
from torchsparsegradutils_amd import _backend, sparse_amg, sparse_fsai, sparse_ilu0  # noqa: E402
from torchsparsegradutils_amd.utils import BICGSTABSettings, GMRESSettings, bicgstab, gmres, last_solve_info  # noqa: E402

RESTART = 30


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = fn()
    torch.cuda.synchronize()
    return x, (time.perf_counter() - t0) * 1e3


def solve_line(problem, A, b, name, run, iterations):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, ms = timed(run)
    its = int(iterations())
    r = torch.sparse.mm(A, x) - b
    return {"case": "solve", "problem": problem, "solver": name, "n": A.size(0), "tolerance": 1e-4, "iterations": its,
            "ms": round(ms, 2), "ms_per_inner_step": round(ms / max(its, 1), 4),
            "true_relative_residual": float(r.norm() / b.norm()), "device": torch.cuda.get_device_name(0)}


def solve_lines(problem, A, max_iter):
    n = A.size(0)
    b = torch.randn(n, 1, device=A.device)
    g_its = lambda: last_solve_info("gmres")["iterations"].max()                     # noqa: E731
    base = GMRESSettings(restart=RESTART, reltol=1e-4, abstol=0.0, maxiter=max_iter)
    lines = [solve_line(problem, A, b, "bicgstab",
                        lambda: bicgstab(A, b, settings=BICGSTABSettings(reltol=1e-4, abstol=0.0, matvec_max=2 * max_iter)),
                        lambda: 2 * last_solve_info("bicgstab")["iterations_enqueued"]),
             solve_line(problem, A, b, f"gmres({RESTART})", lambda: gmres(A, b, settings=base), g_its)]
    for label, make, flexible in (("sparse_fsai", sparse_fsai, False), ("sparse_ilu0", sparse_ilu0, False), ("sparse_amg", sparse_amg, True)):
        t0 = time.perf_counter()
        try:
            M = make(A)
        except Exception as exc:  # noqa: BLE001  (a preconditioner that does not build on this matrix is a result, not an error)
            lines.append({"case": "solve", "problem": problem, "solver": f"gmres({RESTART}) + {label}", "built": False, "why": repr(exc)[:200]})
            continue
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        st = base._replace(precon=M, flexible=flexible)
        line = solve_line(problem, A, b, f"{'flexible ' if flexible else ''}gmres({RESTART}) + {label}", lambda: gmres(A, b, settings=st), g_its)
        line["first_build_ms"] = round(build_ms, 2)
        lines.append(line)
    t_b = lines[0]["ms"]
    for line in lines[1:]:
        if "ms" in line:
            line["speedup_over_bicgstab"] = round(t_b / line["ms"], 3)
    return lines


def kernel_line(n, p, loops, reps, step_ms):
    dev = torch.device("cuda:0")
    td = torch.float32
    m = RESTART
    vt = _backend.vtype_of(torch.empty(0, dtype=td))
    _, group, rows, nb = _backend.gmres_geometry(td, n, p)
    slab = -(-n * p // 4) * 4
    V = torch.randn((m + 1, slab), dtype=td, device=dev)
    w = torch.randn((n, p), dtype=td, device=dev)
    out = torch.empty_like(w)
    coef = torch.full((m, p), 1e-3, dtype=td, device=dev)
    part = torch.empty((nb, m + 1, p), dtype=td, device=dev)
    flags = torch.zeros(4 + 4 * p, dtype=torch.int32, device=dev)

    def project_cycle():
        for k in range(1, m + 1):
            for _ in range(2):
                _backend.launch("tsgu_gmres_project", dev, vt, n, p, k, w, V, slab, part, flags, 1)

    def subtract_cycle():
        for k in range(1, m + 1):
            for _ in range(2):
                _backend.launch("tsgu_gmres_subtract", dev, vt, n, p, k, w, V, slab, coef, out, part, flags, 1)

    src, dst = torch.randn(1 << 27, dtype=td, device=dev), torch.empty(1 << 27, dtype=td, device=dev)
    t_copy = blocks(lambda: _backend.device_copy(src, dst), loops, reps)
    copy_gbs = 2 * src.numel() * 4 / (t_copy[0] * 1e-3) / 1e9
    t_p, t_s = blocks(project_cycle, loops, reps), blocks(subtract_cycle, loops, reps)
    block_bytes = n * p * 4
    bytes_p = sum(2 * (k + 1) for k in range(1, m + 1)) * block_bytes
    bytes_s = sum(2 * (k + 2) for k in range(1, m + 1)) * block_bytes
    gbs_p, gbs_s = bytes_p / (t_p[0] * 1e-3) / 1e9, bytes_s / (t_s[0] * 1e-3) / 1e9
    per_step = (t_p[0] + t_s[0]) / m
    return {"case": "kernels", "n": n, "p": p, "restart": m, "group": group, "rows_per_workgroup": rows, "partial_rows": nb,
            "ms_per_cycle_median_min_max": {"project": t_p, "subtract": t_s}, "GBps": {"project": round(gbs_p, 1), "subtract": round(gbs_s, 1),
                                                                                     "copy": round(copy_gbs, 1)},
            "fraction_of_copy_rate": {"project": round(gbs_p / copy_gbs, 3), "subtract": round(gbs_s / copy_gbs, 3)},
            "orthogonalisation_ms_per_inner_step": round(per_step, 4), "gmres_ms_per_inner_step": step_ms,
            "share_of_inner_step": round(per_step / step_ms, 3) if step_ms else None, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a 20^3 lattice: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "gmres", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gmresbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n1 = 20 if args.small else 126
    lines = []
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)

    def emit(new):
        for line in new:
            lines.append(line)
            print(json.dumps(line), flush=True)
        with open(args.out, "w") as f:          # rewritten after every case: a run that is cut short leaves what it measured
            for line in lines:
                f.write(json.dumps(line) + "\n")

    step_ms = None
    for problem, conv in ((f"convection-diffusion Pe 2 on {n1}^3", 2.0), (f"convection-diffusion Pe 20 on {n1}^3", 20.0)):
        A = stencil7(n1, (1.0, 1.0, 1.0), convection=conv, dev=dev)
        got = solve_lines(problem, A, 2000)
        step_ms = step_ms or got[1]["ms_per_inner_step"]
        emit(got)
    emit([kernel_line(n1 ** 3, 1, args.loops, args.reps, step_ms)])


if __name__ == "__main__":
    main()
