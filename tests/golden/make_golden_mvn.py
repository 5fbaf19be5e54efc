#!/usr/bin/env python3
"""Golden vectors of SparseMultivariateNormalNative, produced by importing the REAL reference in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mvn.py

* mvn_native.npz — for float32 and float64: a lower-triangular CSR factor with a stored positive diagonal at n = 96 (the reference's
  PairwiseEncoder, strictly lower, on a 2 x 4 x 3 x 4 volume plus a diagonal: the ``Lfull`` construction of make_golden_r2.py), ``loc``,
  7 values and 7 rows of fixed noise; the reference's ``log_prob`` (one value and the batch of 7), ``variance``,
  ``covariance_matrix`` and ``rsample((7,))`` under that noise.  The reference is run with int32 AND int64 index tensors; its
  results are the same bits for both (asserted here), so they are stored once per value type beside both index sets.
* mvn_native_errors.json — type and message of the five constructor errors.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
import torchsparsegradutils.distributions.sparse_multivariate_normal as smn  # noqa: E402  (the reference)
from torchsparsegradutils.distributions import SparseMultivariateNormalNative  # noqa: E402
from torchsparsegradutils.encoders.pairwise_encoder import PairwiseEncoder  # noqa: E402

warnings.filterwarnings("ignore")
SHAPE, RADIUS = (2, 4, 3, 4), 1.5
N = 2 * 4 * 3 * 4


def main():
    g = torch.Generator().manual_seed(20240607)
    d = {}
    enc = PairwiseEncoder(RADIUS, SHAPE, diag=False, upper=False, channel_voxel_relation="intra", layout=torch.sparse_csr)
    for vn, dt in (("f32", torch.float32), ("f64", torch.float64)):
        w = 0.05 * torch.randn((len(enc.offsets),) + SHAPE, generator=g, dtype=dt)
        Ls = enc(w)
        assert bool((Ls.to_dense().triu() == 0).all())
        eye = torch.sparse_coo_tensor(torch.arange(N).repeat(2, 1), 1.0 + torch.rand(N, generator=g, dtype=dt), (N, N))
        L = (Ls.to_sparse_coo() + eye).coalesce().to_sparse_csr()
        loc = torch.randn(N, generator=g, dtype=dt)
        eps = torch.randn(7, N, generator=g, dtype=dt)
        x = loc + 1.5 * torch.randn(7, N, generator=g, dtype=dt)
        got = {}
        for iname, idt in (("i32", torch.int32), ("i64", torch.int64)):
            Li = torch.sparse_csr_tensor(L.crow_indices().to(idt), L.col_indices().to(idt), L.values(), (N, N))
            dist = SparseMultivariateNormalNative(loc, Li)
            orig = smn._standard_normal
            smn._standard_normal = lambda shape, dtype, device: eps.reshape(shape)      # fixed noise
            try:
                sample = dist.rsample((7,))
            finally:
                smn._standard_normal = orig
            got[iname] = dict(lp1=dist.log_prob(x[0]), lp7=dist.log_prob(x), variance=dist.variance,
                              covariance=dist.covariance_matrix, sample=sample)
            d[f"{vn}_{iname}_crow"], d[f"{vn}_{iname}_col"] = Li.crow_indices().numpy(), Li.col_indices().numpy()
        for k, v in got["i64"].items():
            assert torch.equal(v, got["i32"][k]), (vn, k)
            d[f"{vn}_{k}"] = v.numpy()
        d[f"{vn}_val"], d[f"{vn}_loc"], d[f"{vn}_eps"], d[f"{vn}_x"] = L.values().numpy(), loc.numpy(), eps.numpy(), x.numpy()
    np.savez_compressed(os.path.join(HERE, "mvn_native.npz"), **d)

    # the five constructor errors
    loc = torch.zeros(4)
    L = torch.eye(4).to_sparse_csr()
    cases = {
        "loc_not_1d": lambda: SparseMultivariateNormalNative(torch.zeros(2, 4), L),
        "not_csr": lambda: SparseMultivariateNormalNative(loc, torch.eye(4).to_sparse_coo()),
        "batched": lambda: SparseMultivariateNormalNative(loc, torch.stack([torch.eye(4)] * 2).to_sparse_csr()),
        "not_square": lambda: SparseMultivariateNormalNative(loc, torch.ones(4, 5).to_sparse_csr()),
        "size_mismatch": lambda: SparseMultivariateNormalNative(torch.zeros(5), L),
    }
    errs = {}
    for name, fn in cases.items():
        try:
            fn()
        except Exception as exc:  # noqa: BLE001
            errs[name] = {"type": type(exc).__name__, "message": str(exc)}
        else:
            raise AssertionError(f"the reference accepted {name}")
    with open(os.path.join(HERE, "mvn_native_errors.json"), "w") as f:
        json.dump(errs, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
    print("wrote mvn_native.npz, mvn_native_errors.json")
