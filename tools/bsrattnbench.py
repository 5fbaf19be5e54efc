#!/usr/bin/env python3
"""sparse_bsr_attention timings on one GPU beside sparse_attention on the CSR expansion and torch's scaled_dot_product_attention
with the dense boolean mask: one JSON line per case.

    python tools/bsrattnbench.py [--loops 5] [--reps 5] [--out profiles/bsr_attention/tool_lines.jsonl]

Pattern: ONE sequence of 16384 tokens under a block-banded + global-blocks mask (every block row attends to its neighbours within
BAND blocks and to the first GLOBAL blocks, which also attend to everything), defined on 128 x 128 blocks so that it is exactly a
64 x 64 block mask and re-expressed with blocks of 16, 32, 64 and 128 (the same stored elements every time), int32 indices, no bias
(`values_as_bias=False`, as the boolean mask of the yardsticks).  Cases: fp32 and bf16, (H, d) = (4, 64) and (8, 128), forward (no
graph) and forward + backward of Q, K and V (torch.autograd.grad), through the public functions.

Yardsticks, measured in the same run on the same mask: `sparse_attention` on its CSR form (every stored element an entry) and
`torch.nn.functional.scaled_dot_product_attention` with the dense boolean mask ([1, H, n, d] operands prepared outside the timing).

Per case: the time, the compulsory bytes over the time and the FLOP/s of the stored logits against the matrix peak of the dtype.
Compulsory bytes: Q, K, V and O once (forward) plus dO, O, Q, K, V, dQ, dK, dV (backward) and the index arrays.  FLOPs: 4·nnz·H·d
forward (Q·Kᵀ and P·V), 10·nnz·H·d more with the backward (dO·Vᵀ, the recomputed Q·Kᵀ, dS·K, dSᵀ·Q, Pᵀ·dO).  Peaks (spec): fp32 matrix
157.3 TFLOP/s, bf16 2.5 PFLOP/s, HBM 8 TB/s.

Times are device-event medians (us) over `reps` blocks of `loops` calls after warm-up, the functions taking turns block by block,
with the least and the greatest block beside them: differences inside that spread are noise.
"""
import argparse
import json
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torchsparsegradutils_amd as tsgu  # noqa: E402
from torchsparsegradutils_amd import sparse_attention, sparse_bsr_attention  # noqa: E402

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

N, COARSE, BAND, GLOBAL = 16384, 128, 1, 1
BLOCKS = (16, 32, 64, 128)
PEAK = {torch.float32: 157.3e12, torch.bfloat16: 2.5e15}
HBM = 8e12


def blocks(fns, loops, reps):
    """{name: (median, min, max)} in us per call; the functions take turns block by block."""
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
            ts[k].append(a.elapsed_time(b) * 1e3 / loops)
    return {k: (round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)) for k, v in ts.items()}


def block_mask(bs):
    """The mask as a boolean (N / bs) x (N / bs) block matrix."""
    nb = N // COARSE
    i = torch.arange(nb)
    coarse = ((i[:, None] - i[None, :]).abs() <= BAND) | (i[None, :] < GLOBAL) | (i[:, None] < GLOBAL)
    return coarse.repeat_interleave(COARSE // bs, 0).repeat_interleave(COARSE // bs, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "bsr_attention", "tool_lines.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bsrattnbench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    sdpa = torch.nn.functional.scaled_dot_product_attention

    dense_mask = block_mask(1).to(dev)
    nnz = int(dense_mask.sum())
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    for dtype in (torch.float32, torch.bfloat16):
        eb = torch.empty(0, dtype=dtype).element_size()
        operands = {}
        for bs in BLOCKS:
            m = block_mask(bs)
            crow = torch.zeros(m.size(0) + 1, dtype=torch.int32)
            crow[1:] = m.sum(1).cumsum(0)
            col = m.nonzero()[:, 1].to(torch.int32)
            val = torch.zeros((col.numel(), bs, bs), dtype=dtype, device=dev)
            operands[f"bsr{bs}"] = (torch.sparse_bsr_tensor(crow.to(dev), col.to(dev), val, (N, N)), col.numel(), m.size(0))
        crow = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        crow[1:] = dense_mask.sum(1).cumsum(0)
        col = dense_mask.nonzero()[:, 1].to(torch.int32)
        operands["csr"] = (torch.sparse_csr_tensor(crow, col, torch.zeros(nnz, dtype=dtype, device=dev), (N, N)), nnz, N)
        operands["sdpa"] = (None, 0, 0)

        for heads, d in ((4, 64), (8, 128)):
            Q, K, V, dO = (torch.randn(N, heads, d, device=dev).to(dtype) for _ in range(4))
            Qg, Kg, Vg = (x.clone().requires_grad_(True) for x in (Q, K, V))
            Qs, Ks, Vs, dOs = (x.permute(1, 0, 2).unsqueeze(0).contiguous() for x in (Q, K, V, dO))
            Qsg, Ksg, Vsg = (x.clone().requires_grad_(True) for x in (Qs, Ks, Vs))
            with torch.no_grad():
                want = sdpa(Qs, Ks, Vs, attn_mask=dense_mask)[0].permute(1, 0, 2).float()
            fns, info = {}, {}
            for name, (A, stored, groups) in operands.items():
                if name == "sdpa":
                    def fwd():
                        with torch.no_grad():
                            return sdpa(Qs, Ks, Vs, attn_mask=dense_mask)

                    def fwdbwd():
                        return torch.autograd.grad(sdpa(Qsg, Ksg, Vsg, attn_mask=dense_mask), (Qsg, Ksg, Vsg), dOs)

                    err = 0.0
                else:
                    f = sparse_attention if name == "csr" else sparse_bsr_attention

                    def fwd(A=A, f=f):
                        with torch.no_grad():
                            return f(A, Q, K, V, values_as_bias=False)

                    def fwdbwd(A=A, f=f):
                        return torch.autograd.grad(f(A, Qg, Kg, Vg, values_as_bias=False), (Qg, Kg, Vg), dO)

                    first, again = fwd(), fwd()
                    assert torch.equal(first, again), f"{name}: two runs of the forward differ"
                    err = float((first.float() - want).abs().max() / want.abs().max())
                    assert err < (2e-2 if dtype == torch.bfloat16 else 1e-4), (name, err)
                fns[name + "_fwd"], fns[name + "_fwdbwd"] = fwd, fwdbwd
                dense_bytes = N * heads * d * eb
                index = 0 if name == "sdpa" else (stored + groups + 1) * 4
                extra = N * N if name == "sdpa" else 0                     # the boolean mask
                work = {"fwd": (4 * dense_bytes + index + extra, 4.0 * nnz * heads * d),
                        "fwdbwd": (12 * dense_bytes + 3 * index + 2 * extra, 14.0 * nnz * heads * d)}
                info[name] = (stored, err, work)
            t = blocks(fns, args.loops, args.reps)
            with open(args.out, "a") as out:
                for name, (stored, err, work) in info.items():
                    for mode, (nbytes, flops) in work.items():
                        med, lo, hi = t[f"{name}_{mode}"]
                        line = {"n": N, "nnz": nnz, "operand": name, "block": int(name[3:]) if name.startswith("bsr") else None,
                                "stored": stored, "mode": mode, "heads": heads, "d": d, "dtype": str(dtype).replace("torch.", ""),
                                "index": "int32", "us_median_min_max": [med, lo, hi], "compulsory_bytes": nbytes,
                                "TBps_compulsory": round(nbytes / med / 1e6, 3), "TFLOPs": round(flops / med / 1e6, 2),
                                "fraction_of_matrix_peak": round(flops / med / 1e-6 / PEAK[dtype], 5),
                                "over_csr": round(med / t[f"csr_{mode}"][0], 3), "over_sdpa": round(med / t[f"sdpa_{mode}"][0], 3),
                                "fwd_rel_err_vs_sdpa": round(err, 7), "device": torch.cuda.get_device_name(0)}
                        print(json.dumps(line), flush=True)
                        out.write(json.dumps(line) + "\n")
        del operands


if __name__ == "__main__":
    main()
