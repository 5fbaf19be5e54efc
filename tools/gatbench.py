#!/usr/bin/env python3
"""sparse_gat_attention / sparse_gatv2_attention timings on one GPU beside the composition they replace and beside
sparse_attention: one JSON line per case.

    python tools/gatbench.py [--loops 10] [--reps 5] [--shapes C2,million,topk] [--out profiles/gat/tool_lines.jsonl]

Cases: the C2 pattern (27-point periodic stencil, N = 10^6), the "million" shape of tools/lsebench.py (N = M = 2^20, nnz = 2^22
uniformly random) and a `sparse_topk_mm` pattern (n = 16384, k = 16 columns per row); CSR int32; float32 and bfloat16;
(H, d) = (1, 64), (4, 32), (8, 64); both kinds; forward (no graph), and forward + backward with every dense operand and A
requiring a gradient.

Beside the fused op, in the same run and taking turns block by block:
  * the composition a user writes today — torch ops for the nnz × H logits (GATv2: through an nnz × H × d tensor), then
    `sparse_softmax` and `sparse_mm` once per head, torch autograd through it — with the peak memory of both; it is skipped
    (null) where its nnz × H × d temporaries alone would pass 24 GB;
  * `sparse_attention` at the same (H, d): the per-lane-exp yardstick with the same gathers of V.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up (the composition: a fifth of the loops), with
the least and the greatest block beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import (sparse_attention, sparse_gat_attention, sparse_gatv2_attention, sparse_mm,  # noqa: E402
                                      sparse_softmax)
from torchsparsegradutils_amd.utils import synthetic  # noqa: E402


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in us per call; the functions take turns block by block.  fns: name -> (fn, loops divisor)."""
    for fn, _ in fns.values():
        for _i in range(2):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _r in range(reps):
        for k, (fn, div) in fns.items():
            n = max(1, loops // div)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _i in range(n):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3 / n)
    return {k: (round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)) for k, v in ts.items()}


def composed(kind, ptr, idx, rows_of, col, shape, heads, slope):
    """The layer from torch ops and the package's per-head ops, autograd through all of it.  The per-head logits go into a
    coalesced COO tensor: the constructor's backward takes the sparse gradient as it is (the CSR constructor's densifies it)."""
    coo = torch.stack([rows_of, col])

    def f(A, a, b, c):
        z = a.index_select(0, rows_of) + b.index_select(0, col)
        t = F.leaky_relu(z, slope) if kind == "gat" else (c * F.leaky_relu(z, slope)).sum(-1)
        t = t + A.values().unsqueeze(1)
        msg = c if kind == "gat" else b
        outs = []
        for h in range(heads):
            P = sparse_softmax(torch.sparse_coo_tensor(coo, t[:, h].contiguous(), shape, is_coalesced=True), -1)
            outs.append(sparse_mm(P, msg[:, h].contiguous()))
        return torch.stack(outs, 1)
    return f


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="C2,million,topk")
    ap.add_argument("--out", default=os.path.join("profiles", "gat", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gatbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def pattern(shape):
        if shape == "C2":
            crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
            return crow.to(dev), col.to(dev), crow.numel() - 1
        if shape == "million":
            n = 1 << 20
            keys = torch.unique(torch.randint(0, n * n, (1 << 22,), device=dev, dtype=torch.int64))
            return torch._convert_indices_from_coo_to_csr(keys // n, n, out_int32=True), (keys % n).int(), n
        n, k = 16384, 16
        cols = torch.rand((n, n), device=dev).topk(k, dim=1).indices.sort(1).values
        return torch.arange(0, n * k + 1, k, device=dev, dtype=torch.int32), cols.reshape(-1).int(), n

    slope = 0.2
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as out:
        for shape in args.shapes.split(","):
            ptr, idx, n = pattern(shape)
            nnz = idx.numel()
            rows_of = torch.repeat_interleave(torch.arange(n, device=dev), (ptr[1:] - ptr[:-1]).long())
            col64 = idx.long()
            for dtype in (torch.float32, torch.bfloat16):
                for heads, d in ((1, 64), (4, 32), (8, 64)):
                    A = torch.sparse_csr_tensor(ptr, idx, torch.randn(nnz, device=dev).to(dtype), (n, n))
                    X = torch.randn(n, heads, d, device=dev).to(dtype)
                    G = torch.randn(n, heads, d, device=dev).to(dtype)
                    for kind in ("gat", "gatv2"):
                        if kind == "gat":
                            ops = (torch.randn(n, heads, device=dev).to(dtype), torch.randn(n, heads, device=dev).to(dtype), X)
                            fused = lambda S, a, b, c: sparse_gat_attention(S, a, b, c, negative_slope=slope)      # noqa: E731
                            temp = nnz * heads * 4
                        else:
                            ops = (torch.randn(n, heads, d, device=dev).to(dtype), X, (torch.randn(heads, d, device=dev) / d ** 0.5).to(dtype))
                            fused = lambda S, a, b, c: sparse_gatv2_attention(S, a, b, c, negative_slope=slope)    # noqa: E731
                            temp = nnz * heads * d * 4
                        attn = lambda S, a, b, c: sparse_attention(S, X, X, X)                                       # noqa: E731
                        comp = composed(kind, ptr, idx, rows_of, col64, (n, n), heads, slope) if 3 * temp < 24e9 else None
                        Ag = A.detach().clone().requires_grad_(True)
                        gops = tuple(x.clone().requires_grad_(True) for x in ops)
                        Xg = X.clone().requires_grad_(True)

                        def fwd(f):
                            with torch.no_grad():
                                return f(A, *ops)

                        def fwdbwd(f):
                            Ag.grad = None
                            for x in gops:
                                x.grad = None
                            f(Ag, *gops).backward(G)

                        def attn_fwdbwd():
                            Ag.grad = Xg.grad = None
                            sparse_attention(Ag, Xg, Xg, Xg).backward(G)

                        fns = {"fused_fwd": (lambda: fwd(fused), 1), "attention_fwd": (lambda: fwd(attn), 1),
                               "fused_fwdbwd": (lambda: fwdbwd(fused), 1), "attention_fwdbwd": (attn_fwdbwd, 1)}
                        err = None
                        if comp is not None:
                            fns.update({"composed_fwd": (lambda: fwd(comp), 5), "composed_fwdbwd": (lambda: fwdbwd(comp), 5)})
                            err = float((fwd(fused).float() - fwd(comp).float()).abs().max())
                        t = blocks(fns, args.loops, args.reps)
                        mem = {"fused_fwdbwd": peak(lambda: fwdbwd(fused))}
                        if comp is not None:
                            mem["composed_fwdbwd"] = peak(lambda: fwdbwd(comp))
                        ratio = (lambda x, y: round(t[x][0] / t[y][0], 3) if x in t else None)
                        line = {"shape": shape, "n": n, "nnz": nnz, "kind": kind, "heads": heads, "d": d,
                                "dtype": str(dtype).replace("torch.", ""), "index": "int32",
                                "us_median_min_max": {k: list(v) for k, v in t.items()},
                                "fwd_composed_over_fused": ratio("composed_fwd", "fused_fwd"),
                                "fwdbwd_composed_over_fused": ratio("composed_fwdbwd", "fused_fwdbwd"),
                                "fwd_fused_over_attention": ratio("fused_fwd", "attention_fwd"),
                                "fwdbwd_fused_over_attention": ratio("fused_fwdbwd", "attention_fwdbwd"),
                                "peak_bytes_fwdbwd": mem, "max_abs_diff_fused_composed": err,
                                "device": torch.cuda.get_device_name(0)}
                        print(json.dumps(line), flush=True)
                        out.write(json.dumps(line) + "\n")
                        out.flush()
                        del comp, Ag, gops, Xg
                        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
