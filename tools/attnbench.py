#!/usr/bin/env python3
"""sparse_attention timings on one GPU beside the composition of its parts: one JSON line per case.

    python tools/attnbench.py [--loops 10] [--reps 5] [--out profiles/attention/tool_lines.jsonl] [--shapes C2,million]

Shapes: the C2 pattern (27-point periodic stencil, N = 10^6) and the "million" shape of tools/lsebench.py (N = M = 2^20,
nnz = 2^22 uniformly random), CSR int32; fp32 with (H, d) = (1, 32), (1, 64), (4, 32) and bf16 with (4, 64).

  fused_fwd       sparse_attention, forward only (no graph is recorded)
  fused_fwdbwd    forward + backward for dA, dQ, dK, dV (the row pass and the column pass)
  composed_fwd    the same forward from the parts, per head: _backend.csr_sddmm -> + bias -> sparse_softmax -> sparse_mm, on
                  the strided head views of the same operands; compared with the fused result first

The three take turns block by block in one process.  Times are device-event medians (us) over `reps` blocks of `loops` calls
after warm-up (plans of the composition's sparse_mm built and waited for), with the least and the greatest block beside them:
differences inside that spread are noise.  Every form allocates its results, as the operators do; the operands are far larger
than the caches (>= 128 MB each), so every call finds them cold.

Bytes, from the shapes: `compulsory` is what the forward must move once — Q, K, V read, O and lse written, (idx, bias) per
entry, the row pointer; `gathered` is what the lanes load — a K row and a V row per entry instead of K and V once.  The
composition moves, per head, the SDDMM's gathers and logits, the bias addition (read 2, write 1 value per entry), the softmax
(read 1, write 1) and the SpMM (value + index + a V row per entry): `composed_compulsory` counts its value-sized arrays only.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd import _backend as be  # noqa: E402
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402

CONFIGS = [(torch.float32, 1, 32), (torch.float32, 1, 64), (torch.float32, 4, 32), (torch.bfloat16, 4, 64)]


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in us per call; the functions take turns block by block."""
    for fn in fns.values():
        for _i in range(3):
            fn()
    tsgu.wait_for_plans()
    for fn in fns.values():
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
            ts[k].append(a.elapsed_time(b) * 1e3 / loops)
    return {k: (round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)) for k, v in ts.items()}


def patterns(dev, which):
    if "C2" in which:
        crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
        yield "C2", crow.to(dev), col.to(dev), crow.numel() - 1
    if "million" in which:
        n = 1 << 20
        keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
        yield "million", torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True), (keys % n).int(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="C2,million")
    ap.add_argument("--out", default=os.path.join("profiles", "attention", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attnbench measures on an MI355X: there is nothing to report without one"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = []
    for shape, crow, col, n in patterns(dev, args.shapes.split(",")):
        nnz = col.numel()
        for dtype, heads, d in CONFIGS:
            es = torch.empty((), dtype=dtype).element_size()
            scale = d ** -0.5
            A = torch.sparse_csr_tensor(crow, col, torch.randn(nnz, device=dev).to(dtype), (n, n))
            Q, K, V, dO = (torch.randn((n, heads, d), device=dev).to(dtype) for _ in range(4))
            Ag = A.detach().requires_grad_(True)
            Qg, Kg, Vg = (x.detach().requires_grad_(True) for x in (Q, K, V))

            def fused_fwd():
                return tsgu.sparse_attention(A, Q, K, V, scale=scale)

            def fused_fwdbwd():
                return torch.autograd.grad(tsgu.sparse_attention(Ag, Qg, Kg, Vg, scale=scale), (Ag, Qg, Kg, Vg), dO)

            def composed_fwd():
                out = []
                for h in range(heads):
                    S = be.csr_sddmm(crow, col, Q[:, h], K[:, h], n, n, alpha=scale)
                    P = tsgu.sparse_softmax(torch.sparse_csr_tensor(crow, col, S + A.values(), (n, n)), -1)
                    out.append(tsgu.sparse_mm(P, V[:, h]))
                return torch.stack(out, 1)

            got, want = fused_fwd(), composed_fwd()
            torch.cuda.synchronize()
            diff = float((got.float() - want.float()).abs().max())
            del got, want
            t = blocks({"fused_fwd": fused_fwd, "composed_fwd": composed_fwd, "fused_fwdbwd": fused_fwdbwd}, args.loops, args.reps)
            acc = 4
            row = heads * d * es
            compulsory = 4 * n * row + n * heads * acc + nnz * (4 + es) + 4 * (n + 1)
            gathered = 2 * n * row + n * heads * acc + nnz * (4 + es + 2 * row) + 4 * (n + 1)
            # per head and entry: logits written, bias pass (2 reads + 1 write), softmax (1 + 1), SpMM value read: 7 values;
            # the index array is read by the SDDMM, the softmax's pointer walk aside, and the SpMM: 2 × 4 bytes
            composed = heads * (nnz * (7 * es + 8) + 4 * n * d * es + 3 * 4 * (n + 1))
            line = {"shape": shape, "n": n, "nnz": nnz, "dtype": str(dtype)[6:], "index": "int32", "heads": heads, "d": d,
                    "max_abs_diff_fused_vs_composed": diff,
                    "us_median_min_max": {k: list(v) for k, v in t.items()},
                    "fwd_speedup_over_composed": round(t["composed_fwd"][0] / t["fused_fwd"][0], 3),
                    "bytes": {"fused_compulsory": compulsory, "fused_gathered": gathered, "composed_compulsory": composed},
                    "fused_fwd_compulsory_GBps": round(compulsory / t["fused_fwd"][0] / 1e3, 1),
                    "fused_fwd_gathered_GBps": round(gathered / t["fused_fwd"][0] / 1e3, 1),
                    "composed_fwd_compulsory_GBps": round(composed / t["composed_fwd"][0] / 1e3, 1),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del A, Q, K, V, dO, Ag, Qg, Kg, Vg
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
