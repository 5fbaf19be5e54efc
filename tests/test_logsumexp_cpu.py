"""sparse_logsumexp / sparse_bidir_logsumexp without a GPU: exports, validation errors, CPU operands against the reference's golden
outputs and torch.logsumexp, the ABI symbols, and the float64 helper the large GPU tests use."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _lse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z, NAMES = _lse_ref.cases()


def test_exports():
    import torchsparsegradutils_amd as tsgu
    from torchsparsegradutils_amd import sparse_bidir_logsumexp, sparse_logsumexp  # noqa: F401

    assert "sparse_logsumexp" in tsgu.__all__ and "sparse_bidir_logsumexp" in tsgu.__all__
    from torchsparsegradutils_amd.sparse_logsumexp import __all__ as mod_all

    assert set(mod_all) == {"sparse_logsumexp", "sparse_bidir_logsumexp"}


@pytest.mark.parametrize("name", sorted(_lse_ref.errors()))
def test_validation_errors(name):
    import torchsparsegradutils_amd as tsgu

    want = _lse_ref.errors()[name]
    fn = _error_builders(tsgu)[name]
    with pytest.raises(Exception) as info:
        fn()
    assert type(info.value).__name__ == want["type"]
    got, exp = str(info.value), want["msg"]
    if "Supported: {" in exp:   # (a set of layouts: its order follows the layouts' hashes)
        got, exp = got.split("Supported:")[0], exp.split("Supported:")[0]
        assert str(info.value).count("torch.sparse_") == 3
    assert got == exp


def _error_builders(mod):
    lse, bidir = mod.sparse_logsumexp, mod.sparse_bidir_logsumexp
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


@pytest.mark.filterwarnings("ignore")
def test_golden_cases_on_cpu():
    import torchsparsegradutils_amd as tsgu

    assert len(NAMES) > 400
    for name in NAMES:
        _lse_ref.check_case(tsgu, Z, name, "cpu")


@pytest.mark.filterwarnings("ignore")
@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_matches_dense_logsumexp(layout, dtype):
    import torchsparsegradutils_amd as tsgu

    g = torch.Generator().manual_seed(3)
    d = torch.randn(9, 7, generator=g, dtype=dtype)
    d[torch.rand(9, 7, generator=g) < 0.6] = 0
    d[4] = 0
    A = {"coo": d.to_sparse_coo, "csr": d.to_sparse_csr, "csc": d.to_sparse_csc}[layout]()
    atol, rtol = _lse_ref.tol(dtype)
    for dim in (0, 1, [0, 1], -1, (1, 0)):
        for kd in (False, True):
            torch.testing.assert_close(tsgu.sparse_logsumexp(A, dim, kd), torch.logsumexp(d, dim, kd), atol=atol, rtol=rtol)
    c, r = tsgu.sparse_bidir_logsumexp(A)
    torch.testing.assert_close(c, torch.logsumexp(d, 0), atol=atol, rtol=rtol)
    torch.testing.assert_close(r, torch.logsumexp(d, 1), atol=atol, rtol=rtol)


@pytest.mark.filterwarnings("ignore")
def test_bidir_equals_two_calls_and_views_padded_on_cpu():
    import torchsparsegradutils_amd as tsgu

    for name in NAMES:
        meta, _, A = _lse_ref.build(Z, name)
        if meta["fn"] != "bidir" or meta["layout"] != "tuple" or meta["keepdim"]:
            continue
        iz = meta["include_zeros"]
        c, r = tsgu.sparse_bidir_logsumexp(A, include_zeros=iz)
        off = 1 if A.dim() == 3 else 0
        assert torch.equal(c, tsgu.sparse_logsumexp(A, off, include_zeros=iz)) or torch.allclose(
            c, tsgu.sparse_logsumexp(A, off, include_zeros=iz), equal_nan=True)
        assert torch.allclose(r, tsgu.sparse_logsumexp(A, off + 1, include_zeros=iz), equal_nan=True)
        assert c._base is not None and c._base is r._base


def test_group_lse_helper_is_pinned_to_the_goldens():
    """_lse_ref.group_lse on the 2-D COO / CSR goldens (row direction) and the duplicate-index / edge cases."""
    checked = 0
    for name in NAMES:
        meta, v, A = _lse_ref.build(Z, name)
        if meta["fn"] != "lse" or meta["dim"] not in (1, -1) or A.dim() != 2 or meta["keepdim"]:
            continue
        if meta["layout_in"] == "coo":
            if not meta["coalesced"]:
                continue
            rows = A._indices()[0].numpy()
            ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=A.size(0)))])
            vals = A._values().numpy()
        elif meta["layout_in"] == "csr":
            ptr, vals = A.crow_indices().numpy(), A.values().numpy()
        else:
            continue
        got, _ = _lse_ref.group_lse(ptr, vals, A.size(1) if meta["include_zeros"] else None)
        want = Z[name + ".out0"].astype(np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4, equal_nan=True, err_msg=name)
        checked += 1
    assert checked >= 40


def test_library_exports_the_new_symbols():
    from torchsparsegradutils_amd import _backend

    header = open(os.path.join(ROOT, "include", "tsgu_hip.h")).read()
    for sym in ("tsgu_segment_logsumexp", "tsgu_segment_logsumexp_backward", "tsgu_segment_logsumexp_workspace"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in _backend.SIGNATURES
    if not os.path.exists(_backend.LIB_PATH):
        pytest.fail("libtsgu_hip.so is not built")
    lib = ctypes.CDLL(_backend.LIB_PATH)
    for sym in ("tsgu_segment_logsumexp", "tsgu_segment_logsumexp_backward", "tsgu_segment_logsumexp_workspace"):
        assert hasattr(lib, sym), sym
    out = ctypes.c_int64(0)
    fn = lib.tsgu_segment_logsumexp_workspace
    fn.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    assert fn(0, 1 << 20, ctypes.byref(out)) == 0 and out.value > 0
