#!/usr/bin/env python3
"""Triangular solve with a stencil factor on one GPU: one JSON line.

    python tools/tribench.py [--loops 10] [--reps 7] [--side 64] [--columns 8]

The flagship caller's factor: the truncated 27-point lower factor on a side³ lattice (N = 262 144 at the default, values as
tools/mvnbench.py makes them), CSR int32 fp32, 8 columns.  Timed: the forward solve, the transposed solve (both under no_grad) and
`sparse_triangular_solve` forward + backward (two solves and the SDDMM).  Beside the cube one ELONGATED lattice of about the same size
(15 x 17 x side³/256 = 261 120 rows at the default: few, very long z-lines — a wave solves its line serially, so this is where the line sweep gains least).
Times are device-event medians over `reps` blocks of `loops` calls after warm-up, in microseconds; `levels` is the number of
dependency levels of THIS factor (the 27-point half: 4x + 2y + z over the lattice) and `us_per_level` the forward time divided by it.

Uses public names only, so the same file runs against an older tree of the package (PYTHONPATH): where the line sweep's switch
(`sparse_solve.ENABLE_TRSM_LATTICE`) exists every case is measured with it on and off, elsewhere once ("switch": null).
Per-kernel times: run this under `rocprofv3 --kernel-trace --stats`."""
import argparse
import importlib
import json
import os
import sys

import torch

if not os.environ.get("PYTHONPATH"):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402

ss = importlib.import_module("torchsparsegradutils_amd.sparse_solve")


def timed(fn, loops, reps):
    for _ in range(5):      # (the pattern's plans and the sync-free sweep's width settle during the first calls)
        fn()
        tsgu.wait_for_plans()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(loops):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / loops)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


def factor(shape, dev):
    crow, col = synthetic.box_stencil(*shape, periodic=(False,) * 3, part="lower")
    n = shape[0] * shape[1] * shape[2]
    val = 0.03 * torch.randn(col.numel())
    rows = torch.repeat_interleave(torch.arange(n), (crow[1:] - crow[:-1]).long())
    on_diag = col.long() == rows
    val[on_diag] = 1.0 + torch.rand(int(on_diag.sum()))
    return torch.sparse_csr_tensor(crow.to(dev), col.to(dev), val.to(dev), (n, n)), n


def measure(shape, columns, loops, reps, dev):
    A, n = factor(shape, dev)
    B = torch.randn(n, columns, device=dev)
    ones = torch.ones(n, columns, device=dev)
    Ag = A.detach().requires_grad_(True)
    Bg = B.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            tsgu.sparse_triangular_solve(A, B, upper=False)

    def transposed():
        with torch.no_grad():
            tsgu.sparse_triangular_solve(A, B, upper=False, transpose=True)

    def fwdbwd():
        torch.autograd.grad(tsgu.sparse_triangular_solve(Ag, Bg, upper=False), (Ag, Bg), ones)

    levels = 4 * (shape[0] - 1) + 2 * (shape[1] - 1) + shape[2]
    out = {"shape": list(shape), "n": n, "nnz": A.values().numel(), "columns": columns, "levels": levels,
           "forward_us": timed(fwd, loops, reps), "transposed_us": timed(transposed, loops, reps),
           "fwdbwd_us": timed(fwdbwd, loops, reps)}
    out["us_per_level"] = round(out["forward_us"] / levels, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--side", type=int, default=64)
    ap.add_argument("--columns", type=int, default=8)
    ap.add_argument("--quick", action="store_true", help="the cube with the tree's default only (launch-shape experiments)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tribench measures on the GPU only"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    has_switch = hasattr(ss, "ENABLE_TRSM_LATTICE")
    res = {"device": torch.cuda.get_device_name(0), "line_sweep_in_tree": has_switch, "cases": []}
    cube = (args.side,) * 3
    long_ = (15, 17, args.side ** 3 // 256)      # (odd: the lattice detector samples rows around the middle of the matrix and
                                                 # must not meet a y = 0 face there)
    # which kernel family a case's solves ran on, where the tree can tell (the line sweep's binding is counted, never required)
    be = importlib.import_module("torchsparsegradutils_amd._backend")
    sweeps = [0]
    if hasattr(be, "csr_sptrsm_lattice"):
        orig = be.csr_sptrsm_lattice

        def counted(*a, **kw):
            sweeps[0] += 1
            return orig(*a, **kw)

        be.csr_sptrsm_lattice = counted
    switches = (True, False) if has_switch else (None,)
    shapes = (("cube", cube), ("elongated", long_))
    if args.quick:
        switches, shapes = switches[:1], shapes[:1]
    for switch in switches:
        if has_switch:
            ss.ENABLE_TRSM_LATTICE = switch
        for name, shape in shapes:
            sweeps[0] = 0
            case = measure(shape, args.columns, args.loops, args.reps, dev)
            case["lattice"], case["switch"], case["on_line_sweep"] = name, switch, sweeps[0] > 0
            res["cases"].append(case)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
