"""Float64 numpy log-sum-exp of segmented groups (pinned to tests/golden/logsumexp.npz by the CPU tests), and the loader of the
golden cases shared by the CPU and GPU tests."""

import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def group_lse(ptr, vals, axis_len=None):
    """log Σ exp over the segments [ptr[g], ptr[g+1]) of vals in float64, plus (axis_len − count) exp(0) terms when axis_len is
    given.  NaN → NaN, +inf → +inf, no terms → -inf.  Returns (lse, terms per group)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    v = np.asarray(vals, dtype=np.float64)
    n = ptr.size - 1
    counts = np.diff(ptr)
    grp = np.repeat(np.arange(n), counts)
    top = np.full(n, -np.inf)
    np.maximum.at(top, grp, v)
    nans = np.zeros(n)
    np.add.at(nans, grp, np.isnan(v))
    zeros = (axis_len - counts).astype(np.float64) if axis_len is not None else np.zeros(n)
    shift = np.where(zeros > 0, np.maximum(top, 0.0), top)
    shift = np.where(np.isfinite(shift), shift, 0.0)
    total = np.zeros(n)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(total, grp, np.exp(v - shift[grp]))
        total += np.where(zeros > 0, zeros * np.exp(-shift), 0.0)
        with np.errstate(divide="ignore"):
            out = np.where(total == 0, -np.inf, shift + np.log(total))
    out = np.where(nans > 0, np.nan, out)
    return out, counts + (zeros if axis_len is not None else 0)


def fwd_bound(lse_ref, k, n_pieces, eps, lane_max=48, wave=64):
    """Bound on |kernel result − float64 value| of one group's log-sum-exp, for a kernel accumulating with machine epsilon
    `eps`: the smaller of a term-count form and a reduction-depth form, both plus 4ε·|lse| for the shift and the final add.

    Term-count form, (2k + 8)·ε: k rounded exp terms summed after the shift by the group's maximum (the total is ≥ 1), each
    addition and each exp costing at most ε relative, and a few ε for the log and the absent-entry term.

    Depth form, (L + 6 + 3·(⌈P/64⌉ + 6) + 2 + ln(1 + k) + 8)·ε, with P the group's range pieces (`n_pieces`) and
    L = kLseLaneMax.  The sums are of positive terms, so the relative error of a total is bounded by the longest chain of
    roundings from a term to it, not by the number of terms:
      - a piece: one lane adds ≤ L terms in sequence (the lane path takes ≤ L entries, the wave path ≤ R/64 ≤ L per lane), then
        a 6-level butterfly: L + 6;
      - the merge: each lane combines ⌈P/64⌉ partials in sequence, then a 6-level butterfly; a combine rounds an exp, a product
        and a sum: 3·(⌈P/64⌉ + 6);
      - each exp term costs ≤ 2ε, and its argument v − m is rounded by ≤ ε/2·|v − m|: weighted by the terms, Σ pᵢ·|ln tᵢ| is an
        entropy ≤ ln k, so ≤ ln(1 + k)·ε over the shift and the rescaling of partials together;
      - the absent entries (one product and one exp), the log and its addition: 8.
    An error δ relative in the total is δ absolute in its log.  For the 2^20-entry row of 512 pieces this is ≈ 1.4e-5
    (+ 4ε·|lse|) in fp32, where the term-count form allows 0.25; short groups keep the term-count form."""
    lse_ref = np.asarray(lse_ref, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    p = np.asarray(n_pieces, dtype=np.float64)
    by_count = 2 * k + 8
    by_depth = lane_max + 6 + 3 * (np.ceil(p / wave) + 6) + 2 + np.log1p(k) + 8
    return np.minimum(by_count, by_depth) * eps + 4 * eps * np.abs(lse_ref)


def group_lse_grad(ptr, vals, g, lse):
    """g[grp(k)] · exp(v[k] − lse[grp(k)]) in float64."""
    ptr = np.asarray(ptr, dtype=np.int64)
    grp = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    v = np.asarray(vals, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(g, np.float64)[grp] * np.exp(v - np.asarray(lse, np.float64)[grp])


def cases():
    z = np.load(os.path.join(GOLDEN, "logsumexp.npz"), allow_pickle=False)
    names = sorted({k.rsplit(".", 1)[0] for k in z.files})
    return z, names


def errors():
    with open(os.path.join(GOLDEN, "logsumexp_errors.json")) as f:
        return json.load(f)


def build(z, name, device="cpu", requires_grad=False):
    """(meta, values leaf, sparse input) of a golden case on `device`."""
    meta = json.loads(str(z[name + ".meta"]))
    shape = tuple(meta["shape"])
    t = lambda k: torch.from_numpy(np.ascontiguousarray(z[f"{name}.{k}"])).to(device)  # noqa: E731
    v = t("val").clone().requires_grad_(requires_grad)
    if meta["layout_in"] == "coo":
        A = torch.sparse_coo_tensor(t("idx"), v, shape, is_coalesced=meta["coalesced"] or None)
    elif meta["layout_in"] == "csr":
        A = torch.sparse_csr_tensor(t("crow"), t("col"), v, shape)
    else:
        A = torch.sparse_csc_tensor(t("ccol"), t("row"), v, shape)
    return meta, v, A


def run(mod, A, meta):
    """The golden case's call with the package module `mod`: the list of outputs as the golden stores them."""
    if meta["fn"] == "lse":
        return [mod.sparse_logsumexp(A, meta["dim"], meta["keepdim"], meta["include_zeros"])]
    out = mod.sparse_bidir_logsumexp(A, keepdim=meta["keepdim"], include_zeros=meta["include_zeros"], output_layout=meta["layout"])
    if meta["layout"] == "padded":
        return [out]
    if meta["layout"] == "nested":
        return list(out.unbind())
    return list(out)


def tol(dtype):
    """The reference tests' tolerances: fp64 1e-6, fp32 1e-4 (absolute / relative)."""
    return (1e-6, 1e-6) if dtype == torch.float64 else (1e-4, 1e-4)


def check_case(mod, z, name, device="cpu"):
    meta, v, A = build(z, name, device, requires_grad=meta_grad(z, name))
    outs = run(mod, A, meta)
    atol, rtol = tol(v.dtype)
    for i, o in enumerate(outs):
        want = torch.from_numpy(z[f"{name}.out{i}"])
        got = o.detach().cpu()
        assert got.shape == want.shape and got.dtype == want.dtype, (name, i, got.shape, want.shape, got.dtype, want.dtype)
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, i, got, want)
        assert torch.equal(torch.isinf(got) & (got > 0), torch.isinf(want) & (want > 0)), (name, i, got, want)
        assert torch.equal(torch.isinf(got) & (got < 0), torch.isinf(want) & (want < 0)), (name, i, got, want)
        torch.testing.assert_close(got, want, atol=atol, rtol=rtol, equal_nan=True, msg=lambda m: f"{name} out{i}: {m}")
    if meta["grad"]:
        ws = [torch.from_numpy(z[f"{name}.w{i}"]).to(device) for i in range(len(outs))]
        gv, = torch.autograd.grad(outs, v, ws)
        want = torch.from_numpy(z[f"{name}.grad"])
        torch.testing.assert_close(gv.detach().cpu(), want, atol=atol, rtol=rtol, equal_nan=True,
                                   msg=lambda m: f"{name} grad: {m}")
    return meta


def meta_grad(z, name):
    return bool(json.loads(str(z[name + ".meta"]))["grad"])
