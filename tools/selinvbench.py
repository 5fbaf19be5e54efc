#!/usr/bin/env python3
"""sparse_selected_inverse timings on one GPU beside the two ways to the same diagonal the package had: one JSON line per case.

    python tools/selinvbench.py [--loops 3] [--reps 5] [--small] [--out profiles/selinv/tool_lines.jsonl]

Operands: the exact Cholesky factors (`sparse_ic0(cholesky_pattern(Q))`, float64 / int32) of full-band precisions (diagonally
dominant, half-bandwidth 16) and of 2-D lattice precisions (5-point Laplacian + 0.5·I in the natural ordering: the factor is a
band of the lattice's width).  Timed at the level of the public call with `check=False` (the pattern plan is cached, the work
buffer is allocated per call).

Beside it, in the same run and taking turns block by block, where n allows (n <= 8192):
  dense      `torch.cholesky_inverse` of the dense factor (the whole inverse, n² memory)
  hutchinson a 64-probe Rademacher estimate of the diagonal, `mean(Z ⊙ L⁻ᵀL⁻¹Z)`, by two `sparse_triangular_solve` sweeps with 64
             right-hand sides: an ESTIMATE (its relative error is reported), not the same result
Times are device-event medians (ms) over `reps` blocks of `loops` calls after warm-up, with the least and the greatest block.
The accuracy of the selected inverse's diagonal against the dense one is reported where the dense one is computed.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import cholesky_pattern, sparse_ic0, sparse_selected_inverse, sparse_triangular_solve  # noqa: E402

DENSE_MAX = 8192


def turns(fns, loops, reps):
    """{name: (median, min, max)} in ms per call; the functions take turns, one block of `loops` calls each."""
    for fn in fns.values():
        for _i in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _r in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(loops):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / loops)
    return {k: [round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}


def band_precision(n, half, gen):
    """A symmetric, diagonally dominant matrix with a full band of half-bandwidth `half` (COO, float64)."""
    off = torch.arange(1, half + 1)
    rows = (torch.arange(n).unsqueeze(1) + off).reshape(-1)
    cols = torch.arange(n).repeat_interleave(half)
    keep = rows < n
    rows, cols = rows[keep], cols[keep]
    v = -torch.rand(rows.numel(), generator=gen, dtype=torch.float64)
    diag = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, -v).index_add_(0, cols, -v) + 1
    ar = torch.arange(n)
    return torch.sparse_coo_tensor(torch.stack((torch.cat((rows, cols, ar)), torch.cat((cols, rows, ar)))), torch.cat((v, v, diag)),
                                   (n, n)).coalesce()


def lattice_precision(nx, ny):
    g = torch.arange(nx * ny).view(nx, ny)
    low = torch.cat((torch.stack((g[1:].reshape(-1), g[:-1].reshape(-1))), torch.stack((g[:, 1:].reshape(-1), g[:, :-1].reshape(-1)))), 1)
    ar = torch.arange(nx * ny).expand(2, -1)
    val = torch.cat((-torch.ones(2 * low.size(1)), 4.5 * torch.ones(nx * ny))).double()
    return torch.sparse_coo_tensor(torch.cat((low, low.flip(0), ar), 1), val, (nx * ny, nx * ny)).coalesce()


def line(family, name, Q, loops, reps, dev):
    n = Q.size(0)
    P = cholesky_pattern(Q)
    P = torch.sparse_csr_tensor(P.crow_indices().int(), P.col_indices().int(), P.values(), P.shape).to(dev)
    L = sparse_ic0(P).L
    first, again = (sparse_selected_inverse(L, check=False) for _ in range(2))
    assert torch.equal(first.values(), again.values()) and first.selinv_info.tolist() == [0, 0]
    diag = first.values()[(first.crow_indices()[1:] - 1).long()]
    fns = {"selected_inverse": lambda: sparse_selected_inverse(L, check=False)}
    out = {"case": "selinv", "family": family, "pattern": name, "n": n, "nnz_factor": int(L.values().numel()), "dtype": "float64",
           "index": "int32"}
    if n <= DENSE_MAX:
        Ld = L.to_dense()
        Z = (torch.randint(0, 2, (n, 64), device=dev, generator=torch.Generator(device=dev).manual_seed(1)) * 2 - 1).double()
        hutch = lambda: (Z * sparse_triangular_solve(L, sparse_triangular_solve(L, Z, upper=False), upper=False, transpose=True)).mean(1)   # noqa: E731
        fns["dense_cholesky_inverse"] = lambda: torch.cholesky_inverse(Ld)
        fns["hutchinson_64"] = hutch
        want = torch.cholesky_inverse(Ld).diagonal()
        out["diag_rel_err_vs_dense"] = float(((diag - want) / want).abs().max())
        out["hutchinson_diag_rel_err"] = float(((hutch() - want) / want).abs().max())
    t = turns(fns, loops, reps)
    out["ms_median_min_max"] = t
    for k in t:
        if k != "selected_inverse":
            out[f"{k}_over_selected_inverse"] = round(t[k][0] / t["selected_inverse"][0], 3)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny operands: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "selinv", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "selinvbench needs an MI355X"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    bands = (256,) if args.small else (4096, 65536)
    lattices = ((12, 12),) if args.small else ((64, 64), (128, 128))
    lines = []
    for n in bands:
        lines.append(line("band", f"half-bandwidth 16, n = {n}", band_precision(n, 16, gen), args.loops, args.reps, dev))
        print(json.dumps(lines[-1]), flush=True)
    for nx, ny in lattices:
        lines.append(line("lattice", f"5-point + 0.5 I on {nx} x {ny}", lattice_precision(nx, ny), args.loops, args.reps, dev))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
