#!/usr/bin/env python3
"""`sparse_expm_mm` on one GPU beside the composition it replaces: one JSON line per case.

    python tools/expmbench.py [--loops 5] [--reps 5] [--small] [--out profiles/expm/tool_lines.jsonl]

Problems, fp32 / int32: C4 (the 7-point Laplacian on 126^3 of tools/factorbench.py) and the C3 pattern (27-point stencil on 64^3,
truncated at the faces, the symmetric values of tools/logdetbench.py).  exp(-t L) B with p = 16, tolerance 1e-6, Gershgorin bounds
(computed once and passed on), |t| rho in {10, 100} for the largest of T in {1, 8} times (the others are j / T of it).

"forward" lines: K, the chunk length, the forward and forward + backward time of the public call (host-timed around a synchronise,
median of `reps` after a warm-up call), the fused loop alone between device events (per step, without and with the kept chunks),
and — in the same run, at the same K and with the same coefficient table — the torch-op composition `_cpu.expm_apply` on the GPU
tensors with `sparse_mm` for the product.  Beside them the plane counts both are expected to move per step next to the matrix:
2 + 5 + (m + 2T)/m fused, 2 + 4 + 3T composed.

"kernel" lines: `tsgu_cheb_step` (with a chunk: 5 planes) and `tsgu_cheb_combine` (emit with accumulate: m + 2T planes; spread:
m + T planes) alone on the same shapes, device-event medians over `reps` blocks of `loops` launches, as TB/s of those planes.
There are no thresholds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ciqbench import event_ms  # noqa: E402
from factorbench import blocks, stencil7  # noqa: E402
from logdetbench import dominant27, host_ms  # noqa: E402
from torchsparsegradutils_amd import _backend, _cpu, sparse_expm_mm, sparse_mm  # noqa: E402
from torchsparsegradutils_amd import sparse_expm as se  # noqa: E402
from torchsparsegradutils_amd.utils._operator import SparseOperator  # noqa: E402

TOL = 1e-6


def forward_line(problem, A, bounds, p, z, T, reps):
    n, dev = A.size(0), A.device
    lo, hi = bounds
    rho = 0.5 * (hi - lo)
    times = [-(z / rho) * (j + 1) / T for j in range(T)]
    t = times[0] if T == 1 else torch.tensor(times, device=dev)
    B = torch.randn(n, p, device=dev)
    kw = dict(bounds=bounds, tolerance=TOL)
    _, info = sparse_expm_mm(A, B, t, return_info=True, **kw)
    K, m = info["terms"], info["chunk"]
    t_f = host_ms(lambda: sparse_expm_mm(A, B, t, **kw), reps)
    Ag = A.detach().clone().requires_grad_(True)
    Bg = B.clone().requires_grad_(True)
    G = torch.randn((n, p) if T == 1 else (T, n, p), device=dev)

    def fwd_bwd():
        Ag.grad = Bg.grad = None
        sparse_expm_mm(Ag, Bg, t, **kw).backward(G)

    t_fb = host_ms(fwd_bwd, reps)
    coef, a, b, K2 = se._coefficients("expmbench", np.asarray(times).reshape(T, 1), lo, hi, TOL, 4096)
    assert K2 == K
    table = torch.as_tensor(np.array(np.broadcast_to(coef, (K + 1, T, p)), order="C"), dtype=A.dtype).to(dev)
    op = SparseOperator(A)
    with torch.no_grad():
        loop_ms, res = event_ms(lambda: se._expm_fused(op, B, table, a, b, False), reps)
        keep_ms, _ = event_ms(lambda: se._expm_fused(op, B, table, a, b, True), reps)
        comp_ms, comp = event_ms(lambda: _cpu.expm_apply(lambda v: sparse_mm(A, v), B, table, a, b, False), reps)
    norm = float(res[0].norm())
    diff = float((comp[0] - res[0]).norm()) / norm if norm > 0 else None     # (an fp32 result that underflows to zero compares nothing)
    steps = max(K, 1)
    return {"case": "forward", "problem": problem, "n": n, "nnz": A.values().numel(), "p": p, "t_rho": z, "T": T, "tolerance": TOL,
            "bounds": [lo, hi], "terms": K, "chunk": m, "forward_ms": t_f, "forward_backward_ms": t_fb,
            "fused_loop_ms": round(loop_ms, 3), "fused_ms_per_step": round(loop_ms / steps, 4),
            "fused_keep_loop_ms": round(keep_ms, 3), "fused_keep_ms_per_step": round(keep_ms / steps, 4),
            "composition_ms": round(comp_ms, 3), "composition_ms_per_step": round(comp_ms / steps, 4),
            "fused_over_composition": round(loop_ms / comp_ms, 4), "composition_vs_fused_rel_diff": diff,
            "planes_per_step_fused": round(2 + 5 + (m + 2 * T) / m, 2), "planes_per_step_composition": 2 + 4 + 3 * T,
            "device": torch.cuda.get_device_name(0)}


def kernel_lines(problem, n, p, m, T, loops, reps):
    dev = torch.device("cuda:0")
    dtype = torch.float32
    align = _backend.expm_geometry(dtype, n, p)[2]
    plane = -(-n * p // align) * align
    prod, x, prev = (torch.randn(n, p, device=dev) for _ in range(3))
    chunk = torch.randn(n, m, p, device=dev)
    coef = torch.randn(m, T, p, device=dev)
    planes = torch.randn(T, plane, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    size = n * p * 4
    out = []
    for name, count, fn in (
        ("tsgu_cheb_step", 4, lambda: _backend.cheb_step(prod, x, prev, 0.5, 0.25, 1.0, flags)),
        ("tsgu_cheb_step + chunk", 5, lambda: _backend.cheb_step(prod, x, prev, 0.5, 0.25, 1.0, flags, chunk=chunk, slot=m // 2)),
        ("tsgu_cheb_step + src + chunk", 6, lambda: _backend.cheb_step(prod, x, prev, 0.5, 0.25, 1.0, flags, src=chunk, src_slot=m // 2,
                                                                       chunk=chunk, slot=m // 2)),
        ("tsgu_cheb_combine emit +=", m + 2 * T, lambda: _backend.cheb_combine(0, chunk, coef, planes, plane, flags, accumulate=True)),
        ("tsgu_cheb_combine spread", m + T, lambda: _backend.cheb_combine(1, chunk, coef, planes, plane, flags)),
    ):
        t = blocks(fn, loops, reps)
        out.append({"case": "kernel", "problem": problem, "kernel": name, "n": n, "p": p, "m": m, "T": T, "planes": count,
                    "ms_median_min_max": t, "model_TB_per_s": round(count * size / (t[0] * 1e-3) / 1e12, 3),
                    "device": torch.cuda.get_device_name(0)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="20^3 / 16^3 lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "expm", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "expmbench needs an MI355X"
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
    for problem, A in ((f"C4: 7-point Laplacian on {n7}^3", stencil7(n7, (1.0, 1.0, 1.0), dev=dev)),
                       (f"C3 pattern: 27-point on {n27}^3, symmetric values", dominant27(n27, dev))):
        bounds = se._gershgorin(A)
        for z in (10.0, 100.0):
            for T in (1, 8):
                fwd = forward_line(problem, A, bounds, 16, z, T, args.reps)
                emit(fwd)
                for line in kernel_lines(problem, A.size(0), 16, fwd["chunk"], T, args.loops, args.reps):
                    emit(line)
    print(f"# {time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
