#!/usr/bin/env python3
"""sparse_bsr_mm timings on one GPU beside sparse_mm on the CSR expansion and torch.mm on the densified operand: one JSON line per case.

    python tools/bsrbench.py [--loops 10] [--reps 5] [--out profiles/bsr_mm/tool_lines.jsonl]

Cases: ONE 16384 x 16384 operand whose 128 x 128 blocks are stored with probability 0.1, expressed as BSR with block sizes 8, 16,
32, 64 and 128 (the same stored elements every time), int32 indices; fp32 and bf16 with p = 64 and 256 columns; forward (no
graph), and forward + backward with both operands requiring a gradient (torch.autograd.grad), through the public functions.

Yardsticks, measured in the same run on the same matrix: `sparse_mm` on its CSR form (every stored element an entry) and
`torch.mm` on its dense form.

Per case: the time, the compulsory bytes over the time, the FLOP/s of the stored elements (2·nnz·p forward, three times that with
the backward; the dense product: 2·n·m·p), and the roofline bound max(bytes / 8 TB/s, flops / matrix peak of the dtype) with the
fraction of it the time reaches.  Compulsory bytes: every operand and result once — forward: values + indices + B + C; the
backward adds G + B + indices + the values' gradient (SDDMM) and values + indices + G + dB (transposed product).  Peaks (spec):
fp32 matrix 157.3 TFLOP/s, bf16 2.5 PFLOP/s, HBM 8 TB/s.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up, the functions taking turns block by
block, with the least and the greatest block beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd import sparse_bsr_mm, sparse_mm  # noqa: E402

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

N, COARSE, DENSITY = 16384, 128, 0.1
BLOCKS = (8, 16, 32, 64, 128)
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2.5e15}
HBM = 8e12


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


def expand(ptr, idx, coarse_vals, bs):
    """(crow, col, values [nnzb, bs, bs]) of the matrix whose stored 128 x 128 blocks are `coarse_vals` (CSR order of the coarse
    pattern ptr / idx), as blocks of bs x bs in sorted (block row, block column) order."""
    r = COARSE // bs
    dev = coarse_vals.device
    sub = torch.arange(r, device=dev, dtype=torch.int32)
    crow, col, val = [torch.zeros(1, dtype=torch.int64, device=dev)], [], []
    for i in range(ptr.numel() - 1):
        lo, hi = int(ptr[i]), int(ptr[i + 1])
        k = hi - lo
        v = coarse_vals[lo:hi].view(k, r, bs, r, bs).permute(1, 0, 3, 2, 4).reshape(-1, bs, bs)
        c = (idx[lo:hi, None] * r + sub[None, :]).reshape(-1)
        val.append(v)
        col.append(c.repeat(r))
        crow.append(torch.full((r,), k * r, dtype=torch.int64, device=dev))
    crow = torch.cumsum(torch.cat(crow), 0).to(torch.int32)
    return crow, torch.cat(col).to(torch.int32), torch.cat(val).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bsr_mm", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bsrbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    nb = N // COARSE
    mask = torch.rand(nb, nb) < DENSITY
    ptr = torch.zeros(nb + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(mask.sum(1), 0)
    idx = torch.nonzero(mask)[:, 1].to(torch.int32).to(dev)
    nnz = int(ptr[-1]) * COARSE * COARSE
    coarse32 = torch.randn(int(ptr[-1]), COARSE, COARSE, device=dev)

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    for dtype in (torch.float32, torch.bfloat16):
        eb = torch.empty(0, dtype=dtype).element_size()
        coarse = coarse32.to(dtype)
        operands = {}
        for bs in BLOCKS:
            crow, col, val = expand(ptr, idx, coarse, bs)
            operands[f"bsr{bs}"] = (torch.sparse_bsr_tensor(crow, col, val, (N, N)), sparse_bsr_mm, col.numel())
        crow, col, val = expand(ptr, idx, coarse, 1)
        operands["csr"] = (torch.sparse_csr_tensor(crow, col, val.reshape(-1), (N, N)), sparse_mm, nnz)
        dense = torch.zeros(N, N, dtype=dtype, device=dev)
        for i in range(nb):
            lo, hi = int(ptr[i]), int(ptr[i + 1])
            dense[i * COARSE:(i + 1) * COARSE].view(COARSE, nb, COARSE)[:, idx[lo:hi].long()] = coarse[lo:hi].permute(1, 0, 2)
        operands["dense"] = (dense, torch.mm, 0)
        del crow, col, val

        for p in (64, 256):
            B = torch.randn(N, p, device=dev).to(dtype)
            G = torch.randn(N, p, device=dev).to(dtype)
            Bg = B.clone().requires_grad_(True)
            with torch.no_grad():
                want = torch.mm(dense, B).float()
            fns, info = {}, {}
            for name, (A, f, stored) in operands.items():
                Ag = A.detach().requires_grad_(True)

                def fwd(A=A, f=f):
                    with torch.no_grad():
                        return f(A, B)

                def fwdbwd(Ag=Ag, f=f):
                    return torch.autograd.grad(f(Ag, Bg), (Ag, Bg), G)

                first, again = fwd(), fwd()
                assert torch.equal(first, again), f"{name}: two runs of the forward differ"
                err = float((first.float() - want).abs().max() / want.abs().max())
                assert err < (2e-2 if dtype == torch.bfloat16 else 1e-4), (name, err)
                fns[name + "_fwd"], fns[name + "_fwdbwd"] = fwd, fwdbwd
                bs = int(name[3:]) if name.startswith("bsr") else 1
                if name == "dense":
                    by_f, fl_f = N * N * eb + 2 * N * p * eb, 2.0 * N * N * p
                    by_b = 2 * (N * N * eb + 2 * N * p * eb)
                else:
                    index = stored * 4 + (N // bs + 1) * 4
                    by_f, fl_f = nnz * eb + index + 2 * N * p * eb, 2.0 * nnz * p
                    by_b = (2 * N * p * eb + index + nnz * eb) + (nnz * eb + index + stored * 8 + 2 * N * p * eb)
                info[name] = (bs, stored, err, {"fwd": (by_f, fl_f), "fwdbwd": (by_f + by_b, 3 * fl_f)})
            t = blocks(fns, args.loops, args.reps)
            with open(args.out, "a") as out:
                for name, (bs, stored, err, work) in info.items():
                    for mode, (nbytes, flops) in work.items():
                        med, lo, hi = t[f"{name}_{mode}"]
                        bound_us = max(nbytes / HBM, flops / PEAK[dtype]) * 1e6
                        line = {"n": N, "density": DENSITY, "nnz": nnz, "operand": name, "block": bs if name.startswith("bsr") else None,
                                "stored_blocks": stored, "mode": mode, "p": p, "dtype": str(dtype).replace("torch.", ""), "index": "int32",
                                "us_median_min_max": [med, lo, hi], "compulsory_bytes": nbytes, "TBps_compulsory": round(nbytes / med / 1e6, 3),
                                "TFLOPs": round(flops / med / 1e6, 2), "roofline_bound_us": round(bound_us, 2),
                                "fraction_of_bound": round(bound_us / med, 4), "over_csr": round(med / t[f"csr_{mode}"][0], 3),
                                "over_dense": round(med / t[f"dense_{mode}"][0], 3), "fwd_rel_err_vs_dense": round(err, 7),
                                "device": torch.cuda.get_device_name(0)}
                        print(json.dumps(line), flush=True)
                        out.write(json.dumps(line) + "\n")
        del operands, dense, coarse


if __name__ == "__main__":
    main()
