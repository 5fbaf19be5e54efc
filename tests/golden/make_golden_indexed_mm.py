#!/usr/bin/env python3
"""Golden vectors of segment_mm / gather_mm, produced by importing the REAL reference in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_indexed_mm.py

* indexed_mm.npz — one entry per case: ``<case>.meta`` (JSON: function, shapes, index dtype), the inputs (``.a``, ``.b``,
  ``.idx`` = seglen_a or idx_b), the reference's fp32 output (``.out``) and its autograd gradients of ``Σ out · w``
  (``.w``, ``.ga``, ``.gb``).  Covers the reference test's "small" shape (100, 32, 7, 10) with both index dtypes, zero-length
  segments (the first and the last among them), a last length below and above what N leaves, a prefix sum that overshoots N,
  and relations that no row uses.
* indexed_mm_errors.json — exception type and message of every validation error of the two functions.
"""
import json
import os
import sys
import warnings
from unittest.mock import patch

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from torchsparsegradutils import indexed_matmul  # noqa: E402  (the reference)
from torchsparsegradutils.indexed_matmul import gather_mm, segment_mm  # noqa: E402

warnings.filterwarnings("ignore")
OUT = {}


def case(name, fn, a, b, idx):
    a = a.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True)
    out = (segment_mm if fn == "segment" else gather_mm)(a, b, idx)
    w = torch.randn(out.shape, generator=GEN)
    ga, gb = torch.autograd.grad((out * w).sum(), (a, b))
    meta = {"fn": fn, "N": a.shape[0], "R": b.shape[0], "D1": b.shape[1], "D2": b.shape[2], "itype": str(idx.dtype)}
    OUT[f"{name}.meta"] = np.array(json.dumps(meta))
    OUT[f"{name}.a"] = a.detach().numpy()
    OUT[f"{name}.b"] = b.detach().numpy()
    OUT[f"{name}.idx"] = idx.numpy()
    OUT[f"{name}.out"] = out.detach().numpy()
    OUT[f"{name}.w"] = w.numpy()
    OUT[f"{name}.ga"] = ga.numpy()
    OUT[f"{name}.gb"] = gb.numpy()


def operands(n, r, d1, d2):
    return torch.randn(n, d1, generator=GEN), torch.randn(r, d1, d2, generator=GEN)


def main():
    global GEN
    GEN = torch.Generator().manual_seed(20)
    # the reference test's "small" shape and its way of drawing lengths / indices
    for itype in (torch.int32, torch.int64):
        tag = str(itype).split(".")[-1]
        n, r, d1, d2 = 100, 32, 7, 10
        a, b = operands(n, r, d1, d2)
        seglen = torch.randint(1, n // r, (r,), generator=GEN).to(itype)
        seglen[-1] = n - seglen[:-1].sum()
        case(f"small_segment_{tag}", "segment", a, b, seglen)
        a, b = operands(n, r, d1, d2)
        case(f"small_gather_{tag}", "gather", a, b, torch.randint(0, r, (n,), generator=GEN).to(itype))

    def seg(name, n, lens, d1=5, d2=6, itype=torch.int64):
        a, b = operands(n, len(lens), d1, d2)
        case(name, "segment", a, b, torch.tensor(lens, dtype=itype))

    seg("seg_zero_first", 12, [0, 5, 7])
    seg("seg_zero_middle", 12, [4, 0, 0, 8], itype=torch.int32)
    seg("seg_zero_last", 12, [0, 4, 0, 8, 0])           # boundaries 0, 0, 4, 4, 12, 12: the last segment is empty
    seg("seg_last_short", 12, [3, 4, 1])                # the last length is never read: rows 7 .. 12 go to b[2]
    seg("seg_last_long", 12, [3, 4, 20])
    seg("seg_overshoot", 12, [5, 9, 4])                 # 0, 5, 14 -> 12: the last segment is empty, the middle one clamped
    seg("seg_overshoot_early", 12, [15, 2, 3, 1], itype=torch.int32)
    seg("seg_single", 9, [9])
    seg("seg_wide", 40, [10, 0, 17, 13], d1=33, d2=18)

    def gat(name, n, r, idx, d1=5, d2=6, itype=torch.int64):
        a, b = operands(n, r, d1, d2)
        case(name, "gather", a, b, torch.tensor(idx, dtype=itype))

    gat("gather_unused", 10, 6, [4, 1, 4, 4, 1, 1, 4, 1, 4, 4])
    gat("gather_unused_ends", 9, 5, [2, 2, 1, 3, 1, 2, 3, 3, 1], itype=torch.int32)
    gat("gather_one_rel", 7, 3, [1] * 7, d1=17, d2=3)
    gat("gather_sorted", 8, 4, [0, 0, 1, 1, 2, 2, 3, 3])

    np.savez_compressed(os.path.join(HERE, "indexed_mm.npz"), **OUT)
    print(f"indexed_mm.npz: {len(OUT) // 8} cases")

    errs = {}

    def err(name, fn, *args, version=None):
        try:
            if version is not None:
                with patch.object(torch, "__version__", version):
                    getattr(indexed_matmul, fn)(*args)
            else:
                getattr(indexed_matmul, fn)(*args)
        except Exception as exc:  # noqa: BLE001
            errs[name] = {"fn": fn, "type": type(exc).__name__, "msg": str(exc)}
        else:
            raise AssertionError(f"{name}: the reference did not raise")

    a, b = torch.randn(10, 4), torch.randn(2, 4, 3)
    err("segment_old_torch", "segment_mm", a, b, torch.tensor([5, 5]), version="2.3.0")
    err("segment_a_1d", "segment_mm", a[0], b, torch.tensor([5, 5]))
    err("segment_b_2d", "segment_mm", a, b[0], torch.tensor([5, 5]))
    err("segment_seglen_2d", "segment_mm", a, b, torch.tensor([[5, 5]]))
    err("segment_d1_mismatch", "segment_mm", torch.randn(10, 5), b, torch.tensor([5, 5]))
    err("segment_r_mismatch", "segment_mm", a, b, torch.tensor([5, 3, 2]))
    a, b = torch.randn(3, 4), torch.randn(2, 4, 5)
    err("gather_old_torch", "gather_mm", a, b, torch.tensor([0, 1, 0]), version="2.3.0")
    err("gather_not_tensor_a", "gather_mm", a.tolist(), b, torch.tensor([0, 1, 0]))
    err("gather_not_tensor_idx", "gather_mm", a, b, [0, 1, 0])
    err("gather_a_1d", "gather_mm", a[0], b, torch.tensor([0, 1, 0]))
    err("gather_b_2d", "gather_mm", a, b[0], torch.tensor([0, 1, 0]))
    err("gather_idx_2d", "gather_mm", a, b, torch.tensor([[0, 1, 0]]))
    err("gather_n_mismatch", "gather_mm", a, b, torch.tensor([0, 1]))
    err("gather_d1_mismatch", "gather_mm", torch.randn(3, 5), b, torch.tensor([0, 1, 0]))
    with open(os.path.join(HERE, "indexed_mm_errors.json"), "w") as f:
        json.dump(errs, f, indent=1, sort_keys=True)
    print(f"indexed_mm_errors.json: {len(errs)} cases")


if __name__ == "__main__":
    main()
