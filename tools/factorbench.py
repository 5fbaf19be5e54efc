#!/usr/bin/env python3
"""sparse_ilu0 / sparse_ic0 timings on one GPU beside their floor and the un-preconditioned solvers: one JSON line per case.

    python tools/factorbench.py [--loops 5] [--reps 5] [--small] [--out profiles/factor/tool_lines.jsonl]

Factor time: ILU(0) and IC(0) on the C3 pattern (27-point stencil on 64³, truncated at the faces; IC on its lower part) and on
the 7-point Laplacian on 126³ (C4), fp32 / int32, at the backend level (`_backend.csr_factor`: the plan is cached, the numeric
factorisation is what a refactorisation costs).  Floor: ONE lower triangular solve with one right-hand side on the same pattern
in the same run — it has the same dependency chain and does a fraction of the arithmetic per row.

Krylov: iterations and wall time to a fixed relative residual for `linear_cg` with and without IC(0) on C4 and on its anisotropic
variant (coefficients 1 : 1 : 1000), and for `bicgstab` with and without ILU(0) on a convection–diffusion stencil (7-point,
upwind convection of cell Péclet number 2 along z).  The time of the factorisation is reported beside the solves, not hidden in
them.  Where preconditioning loses in wall time although it wins in iterations, the line says so (`speedup` < 1).

Times are device-event medians (ms) over `reps` blocks of `loops` calls after warm-up with the least and the greatest block beside
them; the Krylov solves are host-timed once each after a warm-up solve (they synchronise per iteration anyway).
"""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import _backend, _pattern, sparse_ic0, sparse_ilu0  # noqa: E402
from torchsparsegradutils_amd.utils import BICGSTABSettings, bicgstab, last_solve_info, linear_cg, synthetic  # noqa: E402


def blocks(fn, loops, reps):
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


def stencil7(n1, coeff, convection=0.0, dev="cpu"):
    """−∇·(diag(coeff)∇u) + convection·∂u/∂z (first-order upwind) on an n1³ lattice with Dirichlet faces: CSR float32 / int32."""
    crow, col = synthetic.box_stencil(n1, n1, n1, (False, False, False), 7, None, torch.int32)
    crow, col = crow.to(dev), col.to(dev)
    n = n1 ** 3
    rows = torch.repeat_interleave(torch.arange(n, device=dev, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    d = col - rows
    cx, cy, cz = coeff
    val = torch.zeros(col.numel(), device=dev)
    val[d.abs() == n1 * n1] = -cx
    val[d.abs() == n1] = -cy
    val[d == 1] = -cz
    val[d == -1] = -cz - convection          # upwind: the flow goes up z
    val[d == 0] = 2.0 * (cx + cy + cz) + convection
    return torch.sparse_csr_tensor(crow, col, val, (n, n))


def factor_lines(name, A, loops, reps):
    dev = A.device
    n = A.size(0)
    g = _pattern.from_csr(A)
    plan = _pattern.factor_plan(g)
    val = plan.canonical_values(A.values())
    lg, lpos, ldp = plan.lower()
    lval = val.index_select(0, lpos)
    rhs = torch.randn(n, 1, device=dev)
    ilu = lambda: _backend.csr_factor("ilu0", g.crow, g.col, plan.diag_pos, val, n)       # noqa: E731
    ic = lambda: _backend.csr_factor("ic0", lg.crow, lg.col, ldp, lval, n)                 # noqa: E731
    out, info = ic()
    trsm = lambda: _backend.csr_sptrsm(lg.crow, lg.col, out, rhs, n, lower=True, unit=False)    # noqa: E731
    first, again = ilu()[0], ilu()[0]
    assert torch.equal(first, again) and int(info.item()) == 0
    t = {"ilu0": blocks(ilu, loops, reps), "ic0": blocks(ic, loops, reps), "lower_solve_1rhs": blocks(trsm, loops, reps)}
    return {"case": "factor", "pattern": name, "n": n, "nnz": int(g.nnz), "nnz_lower": int(lg.nnz), "dtype": "float32", "index": "int32",
            "ms_median_min_max": t, "ilu0_over_solve": round(t["ilu0"][0] / t["lower_solve_1rhs"][0], 2),
            "ic0_over_solve": round(t["ic0"][0] / t["lower_solve_1rhs"][0], 2), "device": torch.cuda.get_device_name(0)}


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = fn()
    torch.cuda.synchronize()
    return x, (time.perf_counter() - t0) * 1e3


def krylov_line(name, A, solver, tol, max_iter):
    dev = A.device
    n = A.size(0)
    b = torch.randn(n, 1, device=dev)
    t0 = time.perf_counter()
    M = (sparse_ic0 if solver == "linear_cg" else sparse_ilu0)(A)
    torch.cuda.synchronize()
    first_factor_ms = (time.perf_counter() - t0) * 1e3
    res = {}
    for tag, pre in (("plain", None), ("preconditioned", M)):
        if solver == "linear_cg":
            run = lambda: linear_cg(A, b, tolerance=tol, eps=1e-30, stop_updating_after=1e-30, max_iter=max_iter, max_tridiag_iter=0,       # noqa: E731
                                    preconditioner=pre)
        else:
            run = lambda: bicgstab(A, b, settings=BICGSTABSettings(reltol=tol, abstol=0.0, matvec_max=2 * max_iter, precon=pre))          # noqa: E731
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x, ms = timed(run)
        info = last_solve_info(solver)
        r = torch.sparse.mm(A, x) - b
        res[tag] = {"iterations": int(info["iterations"] if solver == "linear_cg" else info["iterations_enqueued"]), "ms": round(ms, 2),
                    "true_relative_residual": float(r.norm() / b.norm())}
    return {"case": "krylov", "problem": name, "solver": solver, "preconditioner": "ic0" if solver == "linear_cg" else "ilu0", "n": n,
            "tolerance": tol, "first_factorisation_ms_with_plan": round(first_factor_ms, 2), **res,
            "speedup": round(res["plain"]["ms"] / res["preconditioned"]["ms"], 3), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="16³ / 20³ lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "factor", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "factorbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n27, n7 = (16, 20) if args.small else (64, 126)

    crow, col = synthetic.box_stencil(n27, n27, n27, (False, False, False), 27, None, torch.int32)
    rows = torch.repeat_interleave(torch.arange(n27 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    val = torch.where(col == rows, torch.tensor(30.0), -torch.rand(col.numel()))        # diagonally dominant, symmetric in its pattern
    C3 = torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n27 ** 3, n27 ** 3))
    lines = [factor_lines(f"C3: 27-point on {n27}^3", C3, args.loops, args.reps)]
    print(json.dumps(lines[-1]), flush=True)
    lap = stencil7(n7, (1.0, 1.0, 1.0), dev=dev)
    lines.append(factor_lines(f"C4: 7-point on {n7}^3", lap, args.loops, args.reps))
    print(json.dumps(lines[-1]), flush=True)
    for name, A, solver in ((f"C4 Laplacian {n7}^3", lap, "linear_cg"),
                            (f"anisotropic 1:1:1000 {n7}^3", stencil7(n7, (1.0, 1.0, 1000.0), dev=dev), "linear_cg"),
                            (f"convection-diffusion {n7}^3", stencil7(n7, (1.0, 1.0, 1.0), convection=2.0, dev=dev), "bicgstab")):
        lines.append(krylov_line(name, A, solver, 1e-4, 2000))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
