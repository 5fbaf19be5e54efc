#!/usr/bin/env python3
"""`sparse_inv_sqrt_mm` on one GPU beside the composition it replaces: one JSON line per case.

    python tools/ciqbench.py [--loops 5] [--reps 5] [--small] [--out profiles/ciq/tool_lines.jsonl]

Problems, fp32 / int32: C4 (the 7-point Laplacian on 126^3 of tools/factorbench.py plus 0.1 I) and the C3 pattern (27-point stencil on
64^3, truncated at the faces) with symmetric, strictly diagonally dominant values.  p = 16, N = 12, tolerance 1e-4, bounds estimated.

"forward" lines: iterations, the forward and forward + backward time of the public call (host-timed around a synchronise, median of
`reps` after a warm-up call, the bounds estimate included and also given alone), the fused loop alone between device events (per
iteration, without and with `keep`), and — in the same run, at the same iteration count — the composition that exists without
the new kernels: `minres(A, B, shifts=σ)` with its stopping test switched off, followed by the weighted sum; and what the stop
launch costs inside the loop (20 iterations that cannot stop, the launch on every iteration against every 10th).

"kernel" lines: `tsgu_ciq_update` alone (without / with `keep`) and `tsgu_minres_vector_ms(which = 1)` alone on the same state,
device-event medians over `reps` blocks of `loops` launches, with the bytes of the plane models (3 S + 5, 5 S + 5, 6 S + 2 planes of
n·p values) over the time; `tsgu_ciq_stop` alone, as a share of one fused iteration.  There are no thresholds.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from factorbench import blocks  # noqa: E402
from logdetbench import dominant27, host_ms, shifted_laplacian  # noqa: E402
from torchsparsegradutils_amd import _backend, sparse_inv_sqrt_mm  # noqa: E402
from torchsparsegradutils_amd import sparse_sqrt as ss  # noqa: E402
from torchsparsegradutils_amd.utils._operator import SparseOperator  # noqa: E402
from torchsparsegradutils_amd.utils.minres import MINRESSettings, minres  # noqa: E402


def event_ms(fn, reps):
    """Median over `reps` of the device time of one call of fn (after a warm-up call); returns (ms, last result)."""
    out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], out


def forward_line(problem, A, p, num_quad, tol, reps):
    n, dev = A.size(0), A.device
    B = torch.randn(n, p, device=dev)
    kw = dict(num_quad=num_quad, tolerance=tol)
    _, info = sparse_inv_sqrt_mm(A, B, return_info=True, **kw)
    lo, hi = info["bounds"]
    iters = info["iterations"]
    t_f = host_ms(lambda: sparse_inv_sqrt_mm(A, B, **kw), reps)
    t_f_given = host_ms(lambda: sparse_inv_sqrt_mm(A, B, bounds=(lo, hi), **kw), reps)
    Ag = A.detach().clone().requires_grad_(True)
    Bg = B.clone().requires_grad_(True)
    G = torch.randn(n, p, device=dev)

    def fwd_bwd():
        Ag.grad = Bg.grad = None
        sparse_inv_sqrt_mm(Ag, Bg, bounds=(lo, hi), **kw).backward(G)

    t_fb = host_ms(fwd_bwd, reps)
    sigma, omega = ss._ciq_rule(lo, hi, num_quad)
    sig_t = torch.as_tensor(sigma, dtype=A.dtype).to(dev)
    om_t = torch.as_tensor(omega, dtype=A.dtype).to(dev)
    op = SparseOperator(A)
    with torch.no_grad():
        loop_ms, res = event_ms(lambda: ss._ciq_fused(op, B, sig_t, om_t, tol, 1000, False), reps)
        loop_keep_ms, res_k = event_ms(lambda: ss._ciq_fused(op, B, sig_t, om_t, tol, 1000, True), reps)
        assert res[3] == iters == res_k[3]
        # the composition at the same iteration count: minres runs max_iter + 2 iterations when its own test never fires
        never = MINRESSettings(max_cg_iterations=1000, minres_tolerance=-1.0)

        def composed():
            sols = minres(A, B, shifts=sig_t, max_iter=iters - 2, settings=never)
            return torch.einsum("q,qnc->nc", om_t, sols.reshape(num_quad, n, p))

        comp_ms, comp = event_ms(composed, reps)
        # what the stop launch costs INSIDE the loop: 20 iterations that cannot stop, the launch on every iteration against every 10th
        every_ms = event_ms(lambda: ss._ciq_fused(op, B, sig_t, om_t, 1e-30, 20, False, stop_every=1), 3 * reps)[0]
        tenth_ms = event_ms(lambda: ss._ciq_fused(op, B, sig_t, om_t, 1e-30, 20, False, stop_every=10), 3 * reps)[0]
    diff = float((comp - res[0]).norm() / res[0].norm())
    return {"case": "forward", "problem": problem, "n": n, "nnz": A.values().numel(), "p": p, "num_quad": num_quad, "tolerance": tol,
            "bounds": [lo, hi], "iterations": iters, "converged": info["converged"],
            "forward_ms": t_f, "forward_given_bounds_ms": t_f_given, "forward_backward_given_bounds_ms": t_fb,
            "fused_loop_ms": round(loop_ms, 3), "fused_ms_per_iteration": round(loop_ms / iters, 4),
            "fused_keep_loop_ms": round(loop_keep_ms, 3), "fused_keep_ms_per_iteration": round(loop_keep_ms / iters, 4),
            "composition_ms": round(comp_ms, 3), "composition_ms_per_iteration": round(comp_ms / iters, 4),
            "fused_over_composition": round(loop_ms / comp_ms, 4), "composition_vs_fused_rel_diff": diff,
            "loop20_stop_every_iteration_ms": round(every_ms, 4), "loop20_stop_every_10th_ms": round(tenth_ms, 4),
            "stop_launch_share_in_loop": round((every_ms - tenth_ms) / 18.0 / (every_ms / 20.0), 4),
            "max_residual_estimate": float(info["residual_estimates"].max()), "device": torch.cuda.get_device_name(0)}


def kernel_lines(problem, n, p, S, iteration_ms, loops, reps):
    dev = torch.device("cuda:0")
    dtype = torch.float32
    align = _backend.ciq_geometry(dtype, n, p)[1]
    plane = -(-n * p // align) * align
    z = [torch.randn(n, p, device=dev), torch.randn(n, p, device=dev)]
    w = [torch.randn(S, plane, device=dev), torch.randn(S, plane, device=dev)]
    acc = torch.zeros(n, p, device=dev)
    sol = torch.zeros(S, plane, device=dev)
    keep = torch.zeros(n, S, p, device=dev)
    scal = torch.rand(S, 12, p, device=dev) * 0.5 + 0.5                # beta = 1 would leave z alone; any finite values time alike
    scal[0, 1] = 1.0
    omega = torch.rand(S, device=dev)
    done = torch.zeros(p, dtype=torch.int32, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    est = torch.zeros(p, device=dev)
    part = torch.empty(1, device=dev)
    size = n * p * 4
    out = []
    for name, planes, fn in (
        ("tsgu_ciq_update", 3 * S + 5, lambda: _backend.ciq_update(z[0], z[1], w[0], w[1], plane, acc, None, scal, omega, done, flags)),
        ("tsgu_ciq_update + keep", 5 * S + 5, lambda: _backend.ciq_update(z[0], z[1], w[0], w[1], plane, acc, keep, scal, omega, done, flags)),
        ("tsgu_minres_vector_ms(which=1)", 6 * S + 2,
         lambda: _backend.launch("tsgu_minres_vector_ms", dev, 0, 1, n, p, z[0], z[1], w[0], w[1], sol, None, scal, flags, part, 0, 0, S,
                                 plane, 1.0)),
    ):
        t = blocks(fn, loops, reps)
        out.append({"case": "kernel", "problem": problem, "kernel": name, "n": n, "p": p, "S": S, "planes": planes,
                    "ms_median_min_max": t, "model_GB_per_s": round(planes * size / (t[0] * 1e-3) / 1e9, 1),
                    "device": torch.cuda.get_device_name(0)})
    scal[:, 6] = 1.0                                                    # never done: the launch does all its work
    t = blocks(lambda: _backend.ciq_stop(scal, 1e-4, est, done, flags), loops, reps)
    out.append({"case": "kernel", "problem": problem, "kernel": "tsgu_ciq_stop", "p": p, "S": S, "ms_median_min_max": t,
                "share_of_a_fused_iteration": round(t[0] / iteration_ms, 4), "device": torch.cuda.get_device_name(0)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="20^3 / 16^3 lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "ciq", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ciqbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    n7, n27 = (20, 16) if args.small else (126, 64)
    lines = []
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(args.out, "w") as f:          # rewritten after every case: a run that is cut short leaves what it measured
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    t0 = time.perf_counter()
    for problem, A in ((f"C4: 7-point on {n7}^3 + 0.1 I", shifted_laplacian(n7, 0.1, dev)),
                       (f"C3 pattern: 27-point on {n27}^3, diagonally dominant", dominant27(n27, dev))):
        fwd = forward_line(problem, A, 16, 12, 1e-4, args.reps)
        emit(fwd)
        for line in kernel_lines(problem, A.size(0), 16, 12, fwd["fused_ms_per_iteration"], args.loops, args.reps):
            emit(line)
    print(f"# {time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
