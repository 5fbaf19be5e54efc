#!/usr/bin/env python3
"""`sparse_topk_mm` on one GPU beside the torch composition it replaces: one JSON line per case.

    python tools/topkbench.py [--loops 3] [--reps 5] [--small] [--out profiles/topk/tool_lines.jsonl]

"forward" lines, n = m in {16384, 65536}, d in {64, 128}, k in {16, 128}, float32 and bfloat16, scale = d^-1/2, standard normal
operands: the fused call and, in the same run and taking turns block by block, the reference
`torch.topk(scale * Q @ K.T, k)` + the assembly of a CSR tensor from it (columns sorted per row, values gathered, crow = arange·k).
Medians (min, max) of `reps` blocks of `loops` calls between device events.  The reference is skipped where its n x m score matrix
does not fit ("reference": null).  Beside them: the achieved rate of the fused call counted as 2·n·m·d operations (a whole-call rate,
not a kernel's share of peak), and the share of (row, key tile) pairs whose pending list was not empty — the drains of
csrc/topk_impl.h — COMPUTED from the scores of 256 sampled rows by the kernel's own rule (a tile drains for a row when one of its
scores beats the k-th best of the tiles before it), not counted inside the kernel.

"backward" lines: forward + backward with a cotangent on the result's own pattern (fused: `torch.autograd.grad` with a sparse CSR
cotangent; reference: the same values through topk's and matmul's backward, a dense n x m cotangent).  The result's index tensors
are new on every call, so the two sparse products of the fused backward run on whatever `_ops` gives a first-seen pattern, and the
transposed pattern is built on every call: that cost is in the line.

"pipeline" line: `sparse_topk_mm -> sparse_attention(values_as_bias=False)` against scores -> topk -> boolean mask ->
`scaled_dot_product_attention` at n = m = 16384, d = 64, k = 16, float32.  There are no thresholds.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd import _backend, sparse_attention, sparse_topk_mm  # noqa: E402


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in ms per call; the functions take turns block by block."""
    for fn in fns.values():
        for _i in range(2):
            fn()
    tsgu.wait_for_plans()
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
    return {k: (round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)) for k, v in ts.items()}


def reference_csr(Q, K, k, scale):
    """torch.topk on the dense scores, assembled as the CSR tensor sparse_topk_mm returns (ties: whatever torch.topk picks)."""
    n, m = Q.size(0), K.size(0)
    val, idx = torch.topk(scale * (Q @ K.t()), k, dim=1)
    idx, order = torch.sort(idx, dim=1)
    val = val.gather(1, order)
    crow = torch.arange(0, n * k + 1, k, dtype=torch.int32, device=Q.device)
    return torch.sparse_csr_tensor(crow, idx.reshape(-1).to(torch.int32), val.reshape(-1), (n, m))


def drain_share(Q, K, k, scale, tile, rows=256):
    """Share of (row, key tile) pairs with a score above the k-th best of the earlier tiles (every pair of the first tiles, before
    k scores exist), for `rows` evenly spaced rows: the drains of the kernel's walk, from the scores."""
    n, m = Q.size(0), K.size(0)
    pick = torch.linspace(0, n - 1, min(rows, n), device=Q.device).long()
    S = scale * (Q[pick].float() @ K.float().t())
    hit = total = 0
    for j0 in range(0, m, tile):
        best = S[:, j0:j0 + tile].amax(1)
        if j0 < k:
            hit += best.numel()
        else:
            kth = torch.topk(S[:, :j0], k, dim=1).values[:, -1]
            hit += int((best > kth).sum())
        total += best.numel()
    return hit / total


def fits(n, m, dtype, copies):
    free, _ = torch.cuda.mem_get_info()
    return n * m * torch.empty((), dtype=dtype).element_size() * copies < 0.8 * free


def case_lines(n, d, k, dtype, loops, reps):
    dev = torch.device("cuda:0")
    m, scale = n, d ** -0.5
    Q, K = (torch.randn(n, d, device=dev).to(dtype) for _ in range(2))
    name = str(dtype).replace("torch.", "")
    tile = _backend.topk_geometry(dtype)[2]
    base = {"n": n, "m": m, "d": d, "k": k, "dtype": name, "device": torch.cuda.get_device_name(0)}
    out = []

    with torch.no_grad():
        fns = {"fused": lambda: sparse_topk_mm(Q, K, k, scale=scale)}
        ref_ok = fits(n, m, dtype, 3)                 # scores, topk's work space, the sort
        if ref_ok:
            fns["reference"] = lambda: reference_csr(Q, K, k, scale)
        t = blocks(fns, loops, reps)
        share = drain_share(Q, K, k, scale, tile)
    ops = 2.0 * n * m * d
    out.append({"case": "forward", **base, "fused_ms": t["fused"], "reference_ms": t.get("reference"),
                "fused_over_reference": round(t["fused"][0] / t["reference"][0], 4) if ref_ok else None,
                "fused_TFLOPs_whole_call": round(ops / (t["fused"][0] * 1e-3) / 1e12, 2), "score_matrix_GB": round(n * m * Q.element_size() / 1e9, 2),
                "drain_share_of_row_tiles_computed": round(share, 4), "keys_per_tile": tile})

    Qg, Kg = Q.clone().requires_grad_(True), K.clone().requires_grad_(True)
    g = torch.randn(n * k, device=dev).to(dtype)

    def fused_fb():
        A = sparse_topk_mm(Qg, Kg, k, scale=scale)
        return torch.autograd.grad(A, (Qg, Kg), torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), g, A.shape))

    def ref_fb():
        val, _ = torch.topk(scale * (Qg @ Kg.t()), k, dim=1)
        return torch.autograd.grad(val, (Qg, Kg), g.view(n, k))

    fns = {"fused": fused_fb}
    ref_ok = fits(n, m, dtype, 5)                     # the scores are kept for the backward, which makes two more dense arrays
    if ref_ok:
        fns["reference"] = ref_fb
    t = blocks(fns, loops, reps)
    out.append({"case": "backward", **base, "fused_fwd_bwd_ms": t["fused"], "reference_fwd_bwd_ms": t.get("reference"),
                "fused_over_reference": round(t["fused"][0] / t["reference"][0], 4) if ref_ok else None,
                "note": "fused backward: two sparse products on a first-seen pattern + its transpose, built per call"})
    return out


def pipeline_line(n, d, k, loops, reps):
    dev = torch.device("cuda:0")
    scale = d ** -0.5
    Q, K, V = (torch.randn(n, d, device=dev) for _ in range(3))

    def ours():
        return sparse_attention(sparse_topk_mm(Q, K, k, scale=scale), Q, K, V, scale=scale, values_as_bias=False)

    def dense():
        idx = torch.topk(scale * (Q @ K.t()), k, dim=1).indices
        mask = torch.zeros((n, n), dtype=torch.bool, device=dev).scatter_(1, idx, True)
        return torch.nn.functional.scaled_dot_product_attention(Q[None, None], K[None, None], V[None, None], attn_mask=mask[None, None],
                                                                scale=scale)[0, 0]

    with torch.no_grad():
        t = blocks({"fused": ours, "reference": dense}, loops, reps)
        diff = float((ours() - dense()).abs().max())
    return {"case": "pipeline", "n": n, "m": n, "d": d, "k": k, "dtype": "float32", "topk_then_sparse_attention_ms": t["fused"],
            "dense_topk_mask_sdpa_ms": t["reference"], "fused_over_reference": round(t["fused"][0] / t["reference"][0], 4),
            "max_abs_difference": diff, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="n = 1024 / 2048: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "topk", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "topkbench needs an MI355X"
    torch.manual_seed(0)
    sizes = (1024, 2048) if args.small else (16384, 65536)
    lines = []
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(args.out, "w") as f:          # rewritten after every case: a run that is cut short leaves what it measured
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    t0 = time.perf_counter()
    emit(pipeline_line(sizes[0], 64, 16, args.loops, args.reps))
    for n in sizes:
        for dtype in (torch.float32, torch.bfloat16):
            for d in (64, 128):
                for k in (16, 128):
                    for line in case_lines(n, d, k, dtype, args.loops if n == sizes[0] else 1, args.reps):
                        emit(line)
    print(f"# {time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
