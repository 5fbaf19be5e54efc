#!/usr/bin/env python3
"""`sparse_logdet` on one GPU, and what the quadrature launch costs beside the CG run that feeds it: one JSON line per case.

    python tools/logdetbench.py [--loops 5] [--reps 5] [--small] [--out profiles/logdet/tool_lines.jsonl]

Problems, fp32 / int32: C4 (the 7-point Laplacian on 126^3 of tools/factorbench.py plus 0.1 I) and the C3 pattern (27-point stencil on
64^3, truncated at the faces) with symmetric, strictly diagonally dominant values.  num_probes in {16, 32}, lanczos_steps in
{20, 30, 100}.  Per "forward" line: the forward and forward + backward time of the public call (host-timed around a synchronise,
median of `reps` after a warm-up call), and, from device events in one instrumented run of the same two steps
(`linear_cg._cg_with_history`, then `_backend.tridiag_quadrature`), the CG run's and the quadrature launch's share of their sum.

"quadrature" lines: the launch alone on full-length histories, r in {20, 30, 100, cap}, p in {16, 256}, device-event medians over
`reps` blocks of `loops` launches.  The "dense" line: at N = 4096 the value and the time against `torch.logdet` of the dense
matrix in the same run, and the observed `stderr` beside the true error.  There are no thresholds.
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
from torchsparsegradutils_amd import _backend, sparse_logdet  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402
from torchsparsegradutils_amd.utils._operator import LAST_SOLVE, SparseOperator  # noqa: E402
from torchsparsegradutils_amd.utils.linear_cg import _cg_with_history  # noqa: E402


def shifted_laplacian(n1, shift, dev):
    A = stencil7(n1, (1.0, 1.0, 1.0), dev=dev)
    crow, col, val = A.crow_indices(), A.col_indices(), A.values().clone()
    rows = torch.repeat_interleave(torch.arange(n1 ** 3, device=dev, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    val[col == rows] += shift
    return torch.sparse_csr_tensor(crow, col, val, A.shape)


def dominant27(n1, dev):
    """The C3 pattern with symmetric values: off-diagonals -(0.25 + ((i + j) mod 7) / 14), diagonal 30 (the row sums stay below 18)."""
    crow, col = synthetic.box_stencil(n1, n1, n1, (False, False, False), 27, None, torch.int32)
    rows = torch.repeat_interleave(torch.arange(n1 ** 3, dtype=torch.int32), (crow[1:] - crow[:-1]).long())
    val = torch.where(col == rows, torch.tensor(30.0), -(0.25 + ((col + rows) % 7).float() / 14.0))
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n1 ** 3, n1 ** 3))


def host_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(ts)[len(ts) // 2], 3)


def forward_line(problem, A, k, steps, reps):
    Ag = A.detach().clone().requires_grad_(True)
    kw = dict(num_probes=k, lanczos_steps=steps, seed=0)

    def fwd_bwd():
        Ag.grad = None
        sparse_logdet(Ag, **kw).backward()

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        value, info = sparse_logdet(A, return_info=True, **kw)
        solve = dict(LAST_SOLVE.info["sparse_logdet"])
        t_f = host_ms(lambda: sparse_logdet(A, **kw), reps)
        t_fb = host_ms(fwd_bwd, reps)
        # the two steps of the forward between events, in the same run
        n, dev = A.size(0), A.device
        Z = _backend.rademacher_fill(n, k, 0, A.dtype, dev)
        op = SparseOperator(A)
        cg_ms, q_ms = [], []
        for _ in range(reps + 1):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            _, hist, _, _, _, norm = _cg_with_history(op, Z, min(steps, n), 1e-4, 1000)[:6]
            e[1].record()
            _backend.tridiag_quadrature(hist, _backend.QUAD_CG, _backend.QUAD_LOG, scale=norm * norm)
            e[2].record()
            e[2].synchronize()
            cg_ms.append(e[0].elapsed_time(e[1]))
            q_ms.append(e[1].elapsed_time(e[2]))
    cg, q = sorted(cg_ms[1:])[reps // 2], sorted(q_ms[1:])[reps // 2]
    return {"case": "forward", "problem": problem, "n": A.size(0), "nnz": A.values().numel(), "num_probes": k, "lanczos_steps": steps,
            "forward_ms": t_f, "forward_backward_ms": t_fb, "cg_run_ms": round(cg, 4), "quadrature_launch_ms": round(q, 4),
            "quadrature_over_cg": round(q / cg, 5), "cg_iterations": solve["iterations"], "fused_cg": solve.get("fused"),
            "logdet": float(value), "stderr": float(info["stderr"]), "lengths_min_max": [int(info["lengths"].min()), int(info["lengths"].max())],
            "device": torch.cuda.get_device_name(0)}


def quadrature_line(r, p, loops, reps):
    dev = torch.device("cuda:0")
    hist = torch.empty((r, 2, p), device=dev)
    hist[:, 0] = 0.2 + 0.1 * torch.rand((r, p), device=dev)          # alpha and beta of a well-conditioned CG run: full length
    hist[:, 1] = 0.4 + 0.3 * torch.rand((r, p), device=dev)
    _, info = _backend.tridiag_quadrature(hist)
    assert int(info.min()) == r
    t = blocks(lambda: _backend.tridiag_quadrature(hist), loops, reps)
    return {"case": "quadrature", "r": r, "p": p, "dtype": "float32", "ms_median_min_max": t, "form": "LDS" if r <= 100 else "work buffer",
            "device": torch.cuda.get_device_name(0)}


def dense_line(reps):
    dev = torch.device("cuda:0")
    A = shifted_laplacian(16, 0.1, dev)
    D = A.to_dense().double()
    exact = float(torch.logdet(D))
    t_dense64 = host_ms(lambda: torch.logdet(D), reps)
    D32 = D.float()
    t_dense32 = host_ms(lambda: torch.logdet(D32), reps)
    out = {"case": "dense", "problem": "7-point on 16^3 + 0.1 I", "n": 4096, "torch_logdet_fp64": exact, "torch_logdet_fp64_ms": t_dense64,
           "torch_logdet_fp32": float(torch.logdet(D32)), "torch_logdet_fp32_ms": t_dense32, "estimates": []}
    for k, steps in ((16, 30), (64, 30), (64, 100)):
        est, info = sparse_logdet(A, num_probes=k, lanczos_steps=steps, seed=0, return_info=True)
        ms = host_ms(lambda: sparse_logdet(A, num_probes=k, lanczos_steps=steps, seed=0), reps)
        out["estimates"].append({"num_probes": k, "lanczos_steps": steps, "logdet": float(est), "ms": ms, "stderr": float(info["stderr"]),
                                 "true_error": float(est) - exact, "error_over_stderr": round(abs(float(est) - exact) / float(info["stderr"]), 3)})
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="20^3 / 16^3 lattices: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "logdet", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "logdetbench needs an MI355X"
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

    cap = _backend.quadrature_geometry()[0]
    for r in (20, 30, 100, cap):
        for p in (16, 256):
            emit(quadrature_line(r, p, args.loops, args.reps))
    emit(dense_line(args.reps))
    for problem, A in ((f"C4: 7-point on {n7}^3 + 0.1 I", shifted_laplacian(n7, 0.1, dev)),
                       (f"C3 pattern: 27-point on {n27}^3, diagonally dominant", dominant27(n27, dev))):
        for k in (16, 32):
            for steps in (20, 30, 100):
                emit(forward_line(problem, A, k, steps, args.reps))


if __name__ == "__main__":
    main()
