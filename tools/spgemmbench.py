#!/usr/bin/env python3
"""sparse_spgemm timings on one GPU beside torch.sparse.mm on the same operands: one JSON line per case.

    python tools/spgemmbench.py [--loops 10] [--reps 5] [--torch-loops 2] [--out profiles/spgemm/tool_lines.jsonl]

Cases, fp32 values and int32 indices, each matrix multiplied by itself: the 27-point periodic stencil on 64³ (125 entries per row
of the square) and the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22 uniformly random).

Per case: the first call (symbolic + numeric, wall clock around a synchronisation, pattern cache emptied before it), the steady
state forward, forward + backward with both operands requiring a gradient and the gradient on C's own index tensors, and
`torch.sparse.mm` on the same operands as COO tensors on the GPU when this torch build offers it (the line says so when it does
not).  Yardstick, bytes: the compulsory traffic of the steady-state forward — A's and B's index and value arrays once, C's
pattern once, C's values once — over its time.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up, with the least and the greatest block
beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import _pattern, sparse_spgemm  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


def blocks(fn, loops, reps):
    """(median, min, max) in us per call."""
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
        ts.append(a.elapsed_time(b) * 1e3 / loops)
    return [round(sorted(ts)[len(ts) // 2], 1), round(min(ts), 1), round(max(ts), 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-loops", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "spgemm", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "spgemmbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    crow, col = synthetic.stencil27_periodic(64, 64, 64, torch.int32)
    stencil = (crow.to(dev), col.to(dev), crow.numel() - 1)
    n = 1 << 20
    keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
    million = (torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True), (keys % n).int(), n)

    # one small product first: the library's load and the kernels' first launches are not what `first_call_ms` is about
    w = torch.eye(64, device=dev).to_sparse_csr()
    sparse_spgemm(w, w)
    torch.cuda.synchronize()

    lines = []
    for shape, (ptr, idx, rows) in (("stencil27_64", stencil), ("million", million)):
        nnz = idx.numel()
        val = torch.randn(nnz, device=dev)
        A = torch.sparse_csr_tensor(ptr, idx, val, (rows, rows))
        Ag = A.detach().clone().requires_grad_(True)
        Bg = torch.sparse_csr_tensor(Ag.crow_indices(), Ag.col_indices(), val.clone(), (rows, rows)).requires_grad_(True)

        _pattern.clear_cache()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            C = sparse_spgemm(A, A)
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        nnz_c = C.values().numel()
        with torch.no_grad():
            again = sparse_spgemm(A, A)
        assert again.col_indices().data_ptr() == C.col_indices().data_ptr() and torch.equal(again.values(), C.values())
        gvals = torch.randn(nnz_c, device=dev)

        def fwd():
            with torch.no_grad():
                return sparse_spgemm(A, A)

        def fwdbwd():
            Ag.grad = Bg.grad = None
            Cg = sparse_spgemm(Ag, Bg)
            Cg.backward(torch.sparse_csr_tensor(Cg.crow_indices(), Cg.col_indices(), gvals, Cg.shape))

        t_fwd = blocks(fwd, args.loops, args.reps)
        t_fb = blocks(fwdbwd, max(args.loops // 2, 1), args.reps)
        compulsory = 2 * (nnz * 8 + (rows + 1) * 4) + nnz_c * 4 + (rows + 1) * 4 + nnz_c * 4
        line = {"shape": shape, "n": rows, "nnz": nnz, "nnz_c": nnz_c, "dtype": "float32", "index": "int32",
                "first_call_ms": round(first_ms, 2), "fwd_us_median_min_max": t_fwd, "fwdbwd_us_median_min_max": t_fb,
                "compulsory_bytes_fwd": compulsory, "fwd_TBps_compulsory": round(compulsory / t_fwd[0] / 1e6, 3),
                "device": torch.cuda.get_device_name(0)}
        try:
            Ac = A.to_sparse_coo().coalesce()
            Ct = torch.sparse.mm(Ac, Ac)
            torch.cuda.synchronize()
            assert Ct._nnz() == nnz_c, "torch.sparse.mm stores another pattern"
            del Ct
            t_torch = blocks(lambda: torch.sparse.mm(Ac, Ac), args.torch_loops, args.reps)
            line["torch_sparse_mm_us_median_min_max"] = t_torch
            line["fwd_over_torch"] = round(t_fwd[0] / t_torch[0], 4)
        except (RuntimeError, NotImplementedError) as exc:
            line["torch_sparse_mm"] = f"not offered by this torch build: {str(exc).splitlines()[0][:160]}"
        print(json.dumps(line), flush=True)
        lines.append(line)
        del A, Ag, Bg, C, again
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
