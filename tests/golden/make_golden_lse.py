#!/usr/bin/env python3
"""Golden vectors of sparse_logsumexp / sparse_bidir_logsumexp, produced by importing the REAL reference in the build container:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lse.py

* logsumexp.npz — one entry per case: ``<case>.meta`` (JSON: call and input description), the input's parts
  (``.idx`` / ``.crow`` / ``.col`` / ``.ccol`` / ``.row``, ``.val``), the outputs (``.out0`` [, ``.out1``]) and, where the
  reference can differentiate the input, the gradient of ``Σ out · w`` (``.w0`` [, ``.w1``], ``.grad``).
  Covers the reference tests' fixtures (5×4 with an empty row and column, the ragged (3, 5, 4) batch, an equal-nnz batch),
  every layout × index dtype × value dtype × dim × include_zeros × keepdim, the bidirectional call in its three layouts, and
  the edge cases (empty group, +inf, NaN, all-negative values, uncoalesced COO, duplicate CSR indices).
* logsumexp_errors.json — exception type and message of every validation error.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from torchsparsegradutils.sparse_logsumexp import sparse_bidir_logsumexp, sparse_logsumexp  # noqa: E402  (the reference)

warnings.filterwarnings("ignore")
OUT = {}
N_CASES = [0]


def fixture_5x4():
    g = torch.Generator().manual_seed(7)
    d = torch.randn(5, 4, generator=g, dtype=torch.float64)
    d[2] = 0        # an empty row
    d[:, 1] = 0     # an empty column
    d[0, 3] = 0
    d[4, 0] = 0
    return d


def fixture_batch_equal():
    g = torch.Generator().manual_seed(8)
    d = torch.randn(3, 5, 4, generator=g, dtype=torch.float64)
    d[:, torch.rand(5, 4, generator=g) < 0.45] = 0
    return d


def fixture_batch_ragged():
    g = torch.Generator().manual_seed(9)
    d = torch.randn(3, 5, 4, generator=g, dtype=torch.float64)
    d[0][torch.rand(5, 4, generator=g) < 0.3] = 0
    d[1][torch.rand(5, 4, generator=g) < 0.7] = 0
    d[2, 1] = 0
    return d


def to_layout(d, layout, itype, vtype):
    d = d.to(vtype)
    if layout == "coo":
        return d.to_sparse_coo()
    A = d.to_sparse_csr() if layout == "csr" else d.to_sparse_csc()
    if itype == torch.int32:
        if layout == "csr":
            A = torch.sparse_csr_tensor(A.crow_indices().int(), A.col_indices().int(), A.values(), A.shape)
        else:
            A = torch.sparse_csc_tensor(A.ccol_indices().int(), A.row_indices().int(), A.values(), A.shape)
    return A


def parts(A):
    if A.layout == torch.sparse_coo:
        return {"idx": A._indices().numpy(), "val": A._values().detach().numpy()}
    if A.layout == torch.sparse_csr:
        return {"crow": A.crow_indices().numpy(), "col": A.col_indices().numpy(), "val": A.values().detach().numpy()}
    return {"ccol": A.ccol_indices().numpy(), "row": A.row_indices().numpy(), "val": A.values().detach().numpy()}


def leaf_from(p, layout, shape, coalesced):
    v = torch.from_numpy(p["val"]).clone().requires_grad_(True)
    if layout == "coo":
        A = torch.sparse_coo_tensor(torch.from_numpy(p["idx"]), v, shape, is_coalesced=coalesced or None)
    elif layout == "csr":
        A = torch.sparse_csr_tensor(torch.from_numpy(p["crow"]), torch.from_numpy(p["col"]), v, shape)
    else:
        A = torch.sparse_csc_tensor(torch.from_numpy(p["ccol"]), torch.from_numpy(p["row"]), v, shape)
    return v, A


def run(A, call):
    if call["fn"] == "lse":
        return [sparse_logsumexp(A, call["dim"], call["keepdim"], call["include_zeros"])]
    out = sparse_bidir_logsumexp(A, keepdim=call["keepdim"], include_zeros=call["include_zeros"], output_layout=call["layout"])
    if call["layout"] == "padded":
        return [out]
    if call["layout"] == "nested":
        return list(out.unbind())
    return list(out)


def case(name, A, call, grad=False):
    layout = {torch.sparse_coo: "coo", torch.sparse_csr: "csr", torch.sparse_csc: "csc"}[A.layout]
    coalesced = A.is_coalesced() if layout == "coo" else True
    p = parts(A)
    meta = dict(call, layout_in=layout, shape=list(A.shape), coalesced=coalesced, grad=grad)
    outs = run(A, call)
    for i, o in enumerate(outs):
        OUT[f"{name}.out{i}"] = o.detach().numpy()
    if grad:
        v, L = leaf_from(p, layout, tuple(A.shape), coalesced)
        outs = run(L, call)
        g = torch.Generator().manual_seed(N_CASES[0])
        ws = [torch.rand(o.shape, generator=g, dtype=o.dtype) + 0.5 for o in outs]
        gv, = torch.autograd.grad(outs, v, ws)
        for i, w in enumerate(ws):
            OUT[f"{name}.w{i}"] = w.numpy()
        OUT[f"{name}.grad"] = gv.numpy()
    for k, a in p.items():
        OUT[f"{name}.{k}"] = a
    OUT[f"{name}.meta"] = np.array(json.dumps(meta))
    N_CASES[0] += 1


def main():
    d2 = fixture_5x4()
    for layout in ("coo", "csr", "csc"):
        for itype in ((torch.int64,) if layout == "coo" else (torch.int32, torch.int64)):
            for vtype in (torch.float32, torch.float64):
                A = to_layout(d2, layout, itype, vtype)
                tag = f"f5x4_{layout}_{str(itype)[-5:]}_{str(vtype)[-7:]}"
                for dim in (0, 1, [0, 1], -1):
                    for iz in (True, False):
                        for kd in (False, True):
                            grad = layout in ("coo", "csr") and vtype == torch.float64 and not kd
                            case(f"{tag}_d{dim}_z{int(iz)}_k{int(kd)}".replace(" ", ""),
                                 A, dict(fn="lse", dim=dim, keepdim=kd, include_zeros=iz), grad=grad)
                for ol in ("tuple", "padded", "nested"):
                    for iz in (True, False):
                        grad = ol == "tuple" and layout in ("coo", "csr") and vtype == torch.float64
                        case(f"{tag}_bidir_{ol}_z{int(iz)}", A, dict(fn="bidir", layout=ol, keepdim=False, include_zeros=iz),
                             grad=grad)
                case(f"{tag}_bidir_tuple_k1", A, dict(fn="bidir", layout="tuple", keepdim=True, include_zeros=True))
    for fname, dfix, layouts in (("beq", fixture_batch_equal(), ("coo", "csr", "csc")), ("brag", fixture_batch_ragged(), ("coo",))):
        for layout in layouts:
            for vtype in (torch.float32, torch.float64):
                A = to_layout(dfix, layout, torch.int64, vtype)
                tag = f"{fname}_{layout}_{str(vtype)[-7:]}"
                for dim in (1, 2, [1, 2], -1):
                    for iz in (True, False):
                        for kd in (False, True):
                            grad = layout == "coo" and vtype == torch.float64 and not kd
                            case(f"{tag}_d{dim}_z{int(iz)}_k{int(kd)}".replace(" ", ""),
                                 A, dict(fn="lse", dim=dim, keepdim=kd, include_zeros=iz), grad=grad)
                for ol in ("tuple", "padded", "nested"):
                    for iz in (True, False):
                        case(f"{tag}_bidir_{ol}_z{int(iz)}", A, dict(fn="bidir", layout=ol, keepdim=False, include_zeros=iz),
                             grad=ol == "tuple" and layout == "coo" and vtype == torch.float64)

    # edge cases
    inf, nan = float("inf"), float("nan")
    i2 = torch.tensor([[0, 0, 1, 1], [0, 1, 0, 2]])
    for name, vals in (("pinf", [inf, 1.0, 2.0, 3.0]), ("nan", [nan, 1.0, 2.0, 3.0]), ("neg", [-1000.0, -1000.0, -1000.0, -999.0]),
                       ("minf", [-inf, -inf, 1.0, 2.0])):
        A = torch.sparse_coo_tensor(i2, torch.tensor(vals, dtype=torch.float64), (3, 3)).coalesce()
        for dim in (0, 1, [0, 1]):
            for iz in (True, False):
                case(f"edge_{name}_coo_d{dim}_z{int(iz)}".replace(" ", ""), A,
                     dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz), grad=True)
                case(f"edge_{name}_csr_d{dim}_z{int(iz)}".replace(" ", ""), A.to_sparse_csr(),
                     dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz), grad=True)
        case(f"edge_{name}_bidir", A, dict(fn="bidir", layout="padded", keepdim=False, include_zeros=True))
    # the reference's own example of a +inf gradient: row [inf, 1] of width 3
    A = torch.sparse_coo_tensor(torch.tensor([[0, 0], [0, 1]]), torch.tensor([inf, 1.0], dtype=torch.float64), (1, 3)).coalesce()
    case("edge_pinf_row", A, dict(fn="lse", dim=1, keepdim=False, include_zeros=True), grad=True)
    # uncoalesced COO: duplicates summed before exp
    iu = torch.tensor([[0, 2, 0, 1, 2], [1, 0, 1, 2, 0]])
    vu = torch.tensor([0.5, 1.5, -2.0, 3.0, 0.25], dtype=torch.float64)
    for vtype in (torch.float32, torch.float64):
        A = torch.sparse_coo_tensor(iu, vu.to(vtype), (3, 4))
        for dim in (0, 1, [0, 1]):
            for iz in (True, False):
                case(f"edge_uncoalesced_{str(vtype)[-7:]}_d{dim}_z{int(iz)}".replace(" ", ""), A,
                     dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz), grad=vtype == torch.float64)
        case(f"edge_uncoalesced_{str(vtype)[-7:]}_bidir", A, dict(fn="bidir", layout="padded", keepdim=False, include_zeros=True))
    # duplicate CSR / CSC indices: every stored entry is its own term (row 0 = cols [1, 1], vals [1, 2], width 3); the reference
    # cannot differentiate these (torch's compressed-tensor backward coalesces them)
    for itype in (torch.int32, torch.int64):
        crow = torch.tensor([0, 2, 3, 3], dtype=itype)
        col = torch.tensor([1, 1, 0], dtype=itype)
        vd = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)
        A = torch.sparse_csr_tensor(crow, col, vd, (3, 3))
        B = torch.sparse_csc_tensor(crow, col, vd, (3, 3))
        for dim in (0, 1, [0, 1]):
            for iz in (True, False):
                case(f"edge_dupcsr_{str(itype)[-5:]}_d{dim}_z{int(iz)}".replace(" ", ""), A,
                     dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz))
                case(f"edge_dupcsc_{str(itype)[-5:]}_d{dim}_z{int(iz)}".replace(" ", ""), B,
                     dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz))
        case(f"edge_dupcsr_{str(itype)[-5:]}_bidir", A, dict(fn="bidir", layout="padded", keepdim=False, include_zeros=True))
    # a matrix with no stored entries at all
    A = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64), (2, 3)).coalesce()
    for dim in (0, 1, [0, 1]):
        for iz in (True, False):
            case(f"edge_empty_d{dim}_z{int(iz)}".replace(" ", ""), A, dict(fn="lse", dim=dim, keepdim=False, include_zeros=iz))

    np.savez_compressed(os.path.join(HERE, "logsumexp.npz"), **OUT)
    print(f"logsumexp.npz: {N_CASES[0]} cases")

    errs = {}
    for name, fn in error_cases().items():
        try:
            fn()
        except Exception as exc:  # noqa: BLE001
            errs[name] = {"type": type(exc).__name__, "msg": str(exc)}
        else:
            raise AssertionError(f"{name} did not raise")
    with open(os.path.join(HERE, "logsumexp_errors.json"), "w") as f:
        json.dump(errs, f, indent=1, sort_keys=True)
    print(f"logsumexp_errors.json: {len(errs)} cases")


def error_cases(lse=None, bidir=None):
    """name -> call raising the reference's validation error (the tests call the same builders with the package's functions)."""
    lse = lse or sparse_logsumexp
    bidir = bidir or sparse_bidir_logsumexp
    A2 = torch.eye(3).to_sparse_coo()
    A3 = torch.ones(2, 3, 3).to_sparse_coo()
    A1 = torch.ones(3).to_sparse_coo()
    A4 = torch.ones(2, 2, 2, 2).to_sparse_coo()
    hybrid = torch.ones(3, 3, 2).to_sparse(2)
    dense = torch.ones(3, 3)
    return {
        "lse_ndim1": lambda: lse(A1, 0),
        "lse_ndim4": lambda: lse(A4, 1),
        "lse_layout": lambda: lse(dense, 0),
        "lse_hybrid": lambda: lse(hybrid, 0),
        "lse_dim_empty": lambda: lse(A2, []),
        "lse_dim_high": lambda: lse(A2, 2),
        "lse_dim_low": lambda: lse(A2, -3),
        "lse_dim_high_3d": lambda: lse(A3, 3),
        "lse_dim_repeat": lambda: lse(A2, [1, -1]),
        "lse_batch_dim": lambda: lse(A3, 0),
        "lse_batch_dim_seq": lambda: lse(A3, [0, 2]),
        "lse_batch_dim_neg": lambda: lse(A3, -3),
        "bidir_ndim1": lambda: bidir(A1),
        "bidir_layout": lambda: bidir(dense),
        "bidir_hybrid": lambda: bidir(hybrid),
        "bidir_output_layout": lambda: bidir(A2, output_layout="flat"),
        "bidir_keepdim_padded": lambda: bidir(A2, keepdim=True, output_layout="padded"),
        "bidir_keepdim_nested": lambda: bidir(A2, keepdim=True, output_layout="nested"),
    }


if __name__ == "__main__":
    main()
