#!/usr/bin/env python3
"""neighbor_mm timings on one GPU beside the two compositions it replaces: one JSON line per case.

    python tools/convbench.py [--loops 10] [--reps 5] [--sets dense64,shell256] [--out profiles/conv/tool_lines.jsonl]

Voxel sets, built here: "dense64", a full 64^3 block (every voxel has all 27 neighbours but at the faces), and "shell256", the
voxels of a 256^3 grid within half a voxel of a sphere of radius 100 (surface-like occupancy), both in raster order.  K = 27 (a 3^3
submanifold convolution), (D1, D2) = (16, 16), (32, 32), (64, 64), (128, 128), float32 and bfloat16, int32 tables; forward (no graph)
and forward + backward with x, w and bias requiring a gradient.

Beside the fused op, in the same run and taking turns block by block, with torch autograd through them:
  * "offsets": per offset `index_select -> mm -> index_add_` over that offset's present pairs (the pair lists are built once);
  * "gather_mm": the package's `gather_mm` over all present pairs at once (x gathered to (pairs, D1), the relation index the
    offset), then one `index_add_`.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up (the compositions: a fifth of the loops) with
the least and the greatest block beside them; the peak memory of forward + backward; and the fraction of the forward's LDS stages
the occupancy skip drops, computed from the table (128-row tiles, whole offsets per stage as csrc/conv_impl.h packs them).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torchsparsegradutils_amd import gather_mm, kernel_offsets, neighbor_mm, voxel_neighbors  # noqa: E402

KC = {torch.float32: 64, torch.bfloat16: 128}


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def voxels(name, dev):
    if name == "dense64":
        ax = torch.arange(64, device=dev)
        return torch.cartesian_prod(ax[:1], ax, ax, ax).int()
    ax = torch.arange(256, device=dev, dtype=torch.float32) - 127.5
    r = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt()
    xyz = ((r - 100).abs() < 0.5).nonzero()
    return torch.cat([torch.zeros_like(xyz[:, :1]), xyz], 1).int()


def skipped(nbr, d1, dtype):
    """Fraction of the forward's (tile, stage) pairs without a present neighbour."""
    n, K = nbr.shape
    S = 1 if d1 > KC[dtype] else min(8, KC[dtype] // d1)
    pad_n, pad_k = -n % 128, -K % S
    has = torch.nn.functional.pad((nbr >= 0).to(torch.uint8), (0, pad_k, 0, pad_n)).view(-1, 128, (K + pad_k) // S, S)
    return round(1.0 - float(has.amax((1, 3)).float().mean()), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sets", default="dense64,shell256")
    ap.add_argument("--out", default=os.path.join("profiles", "conv", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "convbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.sets.split(","):
            coords = voxels(name, dev)
            n = coords.size(0)
            nbr = voxel_neighbors(coords, kernel_offsets(3))
            K = nbr.size(1)
            dst, rel = (nbr >= 0).nonzero(as_tuple=True)
            src = nbr[dst, rel].long()
            order = torch.argsort(rel, stable=True)
            cuts = torch.searchsorted(rel[order].contiguous(), torch.arange(K + 1, device=dev)).tolist()
            per_k = [(dst[order[a:b]], src[order[a:b]]) for a, b in zip(cuts[:-1], cuts[1:])]
            rel32 = rel.int()

            def by_offsets(x, w, b):
                res = b.expand(n, -1).clone()
                for k, (d, s) in enumerate(per_k):
                    res = res.index_add(0, d, x.index_select(0, s) @ w[k])
                return res

            def by_gather_mm(x, w, b):
                return b.expand(n, -1).clone().index_add(0, dst, gather_mm(x.index_select(0, src), w, rel32))

            for dtype in (torch.float32, torch.bfloat16):
                for d1, d2 in ((16, 16), (32, 32), (64, 64), (128, 128)):
                    ops = tuple(t.to(dtype) for t in (torch.randn(n, d1, device=dev), torch.randn(K, d1, d2, device=dev) / (K * d1) ** 0.5,
                                                      torch.randn(d2, device=dev)))
                    G = torch.randn(n, d2, device=dev).to(dtype)
                    gops = tuple(t.clone().requires_grad_(True) for t in ops)
                    fused = lambda x, w, b: neighbor_mm(x, w, nbr, b)   # noqa: E731

                    def fwd(f):
                        with torch.no_grad():
                            return f(*ops)

                    def fwdbwd(f):
                        for t in gops:
                            t.grad = None
                        f(*gops).backward(G)

                    fns = {}
                    for tag, f, div in (("fused", fused, 1), ("offsets", by_offsets, 5), ("gather_mm", by_gather_mm, 5)):
                        fns[tag + "_fwd"] = (lambda f=f: fwd(f), div)
                        fns[tag + "_fwdbwd"] = (lambda f=f: fwdbwd(f), div)
                    err = {tag: float((fwd(fused).float() - fwd(f).float()).abs().max()) for tag, f in (("offsets", by_offsets), ("gather_mm", by_gather_mm))}
                    t = blocks(fns, args.loops, args.reps)
                    mem = {tag: peak(lambda f=f: fwdbwd(f)) for tag, f in (("fused", fused), ("offsets", by_offsets), ("gather_mm", by_gather_mm))}
                    ratio = (lambda x, y: round(t[x][0] / t[y][0], 3))
                    line = {"set": name, "n": n, "K": K, "pairs": int(dst.numel()), "d1": d1, "d2": d2, "dtype": str(dtype).replace("torch.", ""),
                            "index": "int32", "us_median_min_max": {k: list(v) for k, v in t.items()},
                            "fwd_offsets_over_fused": ratio("offsets_fwd", "fused_fwd"),
                            "fwd_gather_mm_over_fused": ratio("gather_mm_fwd", "fused_fwd"),
                            "fwdbwd_offsets_over_fused": ratio("offsets_fwdbwd", "fused_fwdbwd"),
                            "fwdbwd_gather_mm_over_fused": ratio("gather_mm_fwdbwd", "fused_fwdbwd"),
                            "peak_bytes_fwdbwd": mem, "stages_skipped": skipped(nbr, d1, dtype), "max_abs_diff_from_fused": err,
                            "device": torch.cuda.get_device_name(0)}
                    print(json.dumps(line), flush=True)
                    out.write(json.dumps(line) + "\n")
                    out.flush()
                    del gops, ops, G
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
