#!/usr/bin/env python3
"""`sparse_semi_structured_linear` on one GPU beside the dense layer it prunes: one JSON line per case.

    python tools/semibench.py [--loops 3] [--reps 5] [--small] [--out profiles/semi/tool_lines.jsonl]

A pruned-weight layer `X·Aᵀ` in bfloat16 at layer shapes (out x in) 4096 x 4096 and 8192 x 28672 with 512 to 8192 tokens.  Three
contestants in the same process, taking turns block by block: `torch.nn.functional.linear` on the dense bfloat16 weight (the pruned
matrix with its zeros), this op on the expanding path (`TSGU_SEMI_SMFMAC=0`: a dense LDS image, `v_mfma`) and this op on the sparse
matrix instruction (`v_smfmac`).  "forward" lines time the product alone, "forward_backward" lines the product plus the gradients of
the weight (dense: the full out x in gradient; this op: the kept values only) and of the input.  Medians (min, max) of `reps` blocks
of `loops` calls between device events; rates count the DENSE 2·tokens·out·in operations of the forward, so a sparse path that
skips half of them can exceed the dense instruction's peak.  "prune" lines: `sparse_semi_structured_prune` per matrix, with the
bytes it reads and writes.  There are no thresholds."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import sparse_semi_structured as semi  # noqa: E402
from torchsparsegradutils_amd import sparse_semi_structured_linear, sparse_semi_structured_prune  # noqa: E402


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in ms per call; the functions take turns block by block."""
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
    return {k: (round(sorted(v)[len(v) // 2], 4), round(min(v), 4), round(max(v), 4)) for k, v in ts.items()}


def on_path(smfmac, fn):
    def run():
        semi.USE_SMFMAC = smfmac
        return fn()
    return run


def layer_lines(out_f, in_f, tokens, loops, reps):
    dev = torch.device("cuda:0")
    W = torch.randn(out_f, in_f, device=dev).bfloat16()
    A = sparse_semi_structured_prune(W)
    Wd = A.to_dense()
    X = torch.randn(tokens, in_f, device=dev).bfloat16()
    G = torch.randn(tokens, out_f, device=dev).bfloat16()
    base = {"out": out_f, "in": in_f, "tokens": tokens, "dtype": "bfloat16", "device": torch.cuda.get_device_name(0)}
    ops = 2.0 * tokens * out_f * in_f
    rate = lambda ms: round(ops / (ms * 1e-3) / 1e12, 1)      # noqa: E731
    lines = []
    with torch.no_grad():
        ours = lambda: sparse_semi_structured_linear(X, A)    # noqa: E731
        t = blocks({"dense": lambda: torch.nn.functional.linear(X, Wd), "expand": on_path(False, ours), "smfmac": on_path(True, ours)}, loops, reps)
        diff = float((on_path(True, ours)().float() - on_path(False, ours)().float()).abs().max())
    lines.append({"case": "forward", **base, "dense_linear_ms": t["dense"], "expand_ms": t["expand"], "smfmac_ms": t["smfmac"],
                  "smfmac_over_expand": round(t["smfmac"][0] / t["expand"][0], 4), "smfmac_over_dense": round(t["smfmac"][0] / t["dense"][0], 4),
                  "expand_over_dense": round(t["expand"][0] / t["dense"][0], 4),
                  "dense_equivalent_TFLOPs": {k: rate(v[0]) for k, v in t.items()}, "max_abs_difference_between_paths": diff})
    Wg, Xg = Wd.clone().requires_grad_(True), X.clone().requires_grad_(True)
    vg = A.values.clone().requires_grad_(True)

    def dense_fb():
        return torch.autograd.grad(torch.nn.functional.linear(Xg, Wg), (Wg, Xg), G)

    def ours_fb():
        return torch.autograd.grad(sparse_semi_structured_linear(Xg, A.with_values(vg)), (vg, Xg), G)

    t = blocks({"dense": dense_fb, "expand": on_path(False, ours_fb), "smfmac": on_path(True, ours_fb)}, loops, reps)
    lines.append({"case": "forward_backward", **base, "dense_linear_ms": t["dense"], "expand_ms": t["expand"], "smfmac_ms": t["smfmac"],
                  "smfmac_over_expand": round(t["smfmac"][0] / t["expand"][0], 4), "smfmac_over_dense": round(t["smfmac"][0] / t["dense"][0], 4),
                  "note": "the two gradient kernels are the same on both paths (dense MFMA); the weight gradient is (out, in / 2)"})
    return lines


def prune_line(out_f, in_f, loops, reps):
    W = torch.randn(out_f, in_f, device="cuda:0").bfloat16()
    with torch.no_grad():
        t = blocks({"prune": lambda: sparse_semi_structured_prune(W)}, loops, reps)["prune"]
    moved = out_f * in_f * 2 * 1.5 + out_f * in_f / 8
    return {"case": "prune", "out": out_f, "in": in_f, "dtype": "bfloat16", "prune_ms": t, "GB_per_s": round(moved / (t[0] * 1e-3) / 1e9, 1),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="256 x 512 layers: a check of the tool, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "semi", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "semibench needs an MI355X"
    torch.manual_seed(0)
    layers = ((256, 512),) if args.small else ((4096, 4096), (8192, 28672))
    token_counts = (64, 512) if args.small else (512, 2048, 8192)
    lines = []
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)
        with open(args.out, "w") as f:          # rewritten after every case: a run that is cut short leaves what it measured
            for ln in lines:
                f.write(json.dumps(ln) + "\n")

    t0 = time.perf_counter()
    for out_f, in_f in layers:
        emit(prune_line(out_f, in_f, args.loops, args.reps))
        for tokens in token_counts:
            for line in layer_lines(out_f, in_f, tokens, args.loops, args.reps):
                emit(line)
    print(f"# {time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
