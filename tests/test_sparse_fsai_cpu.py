"""sparse_fsai without a GPU: the properties of the numpy oracle of the GPU tests, the public API on CPU operands against that
oracle, M(R), every refusal, and the C-ABI header of the build with its host-side refusals."""

import ctypes
import os

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK
import _fsai_ref as sr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_fsai

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(ptr, idx, val, dtype=torch.float64, itype=torch.int64):
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(np.asarray(ptr)).to(itype), torch.from_numpy(np.asarray(idx)).to(itype),
                                   torch.from_numpy(np.asarray(val)).to(dtype), (n, n))


def _spd(ptr, idx, seed):
    """(float64 values on the pattern, the CSR of tril(A))."""
    val = sr.dominant_values(ptr, idx, seed=seed, symmetric=True)
    lptr, lidx, lval, _ = sr.lower_csr(ptr, idx, val)
    return val, (lptr, lidx, lval)


def test_exports():
    assert {"sparse_fsai", "SparseFSAI"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_fsai import __all__ as mod_all

    assert mod_all == ["sparse_fsai", "SparseFSAI"]
    assert tsgu.sparse_fsai is sparse_fsai and isinstance(tsgu.SparseFSAI, type)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle


@pytest.mark.parametrize("power", [1, 2])
def test_the_oracle_has_a_unit_diagonal(power):
    ptr, idx = sr.stencil(4, 3, 3, 27)
    val, (lptr, lidx, lval) = _spd(ptr, idx, 3)
    sptr, sidx = sr.power_lower_pattern(ptr, idx, power)
    if power == 1:
        assert np.array_equal(sptr, lptr) and np.array_equal(sidx, lidx)
    else:
        assert len(sidx) > len(lidx)                 # S holds positions that A does not store
    g, info = sr.fsai(lptr, lidx, lval, sptr, sidx)
    G, A = sr.dense_lower(sptr, sidx, g), sr.dense(ptr, idx, val)
    assert info == 0 and float(np.abs(np.diag(G @ A @ G.T) - 1).max()) < 1e-13


def test_the_oracle_is_the_inverse_cholesky_factor_where_that_lies_inside_the_pattern():
    ptr, idx = sr.block_diagonal([4, 1, 9, 6])
    val, (lptr, lidx, lval) = _spd(ptr, idx, 4)
    g, info = sr.fsai(lptr, lidx, lval, lptr, lidx)
    G, A = sr.dense_lower(lptr, lidx, g), sr.dense(ptr, idx, val)
    assert info == 0 and float(np.abs(G @ A @ G.T - np.eye(20)).max()) < 1e-12
    assert np.allclose(G, np.linalg.inv(np.linalg.cholesky(A)), rtol=1e-12, atol=1e-14)
    dptr, didx = sr.band(9, 0)
    d = np.arange(1.0, 10.0)
    g, info = sr.fsai(dptr, didx, d, dptr, didx)
    assert info == 0 and float(np.abs(g * d * g - 1).max()) < 1e-12


def test_the_oracle_on_the_diagonal_pattern_is_jacobi_scaling():
    ptr, idx = sr.stencil(4, 3, 3, 27)
    val, (lptr, lidx, lval) = _spd(ptr, idx, 5)
    dptr, didx = sr.band(len(ptr) - 1, 0)
    g, info = sr.fsai(lptr, lidx, lval, dptr, didx)
    assert info == 0 and np.allclose(g, np.diag(sr.dense(ptr, idx, val)) ** -0.5, rtol=1e-15, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# the public API on CPU operands


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_operands_against_the_oracle(dtype, itype):
    npdt = np.float32 if dtype == torch.float32 else np.float64
    ptr, idx = sr.random_pattern(60, 8, seed=2)
    val, _ = _spd(ptr, idx, 6)
    val = val.astype(npdt)
    lptr, lidx, lval, _ = sr.lower_csr(ptr, idx, val)
    want, _ = sr.fsai(lptr, lidx, lval, lptr, lidx)                 # float64 from the rounded inputs
    M = sparse_fsai(_csr(ptr, idx, val, dtype, itype))
    assert isinstance(M, tsgu.SparseFSAI) and M.shape == (60, 60) and M.dtype == dtype and M.device.type == "cpu"
    assert M.values.dtype == dtype and int(M.info) == 0 and M.info.dtype == torch.int64
    assert M.crow_indices.dtype == itype and torch.equal(M.crow_indices, torch.from_numpy(lptr).to(itype))
    assert torch.equal(M.col_indices, torch.from_numpy(lidx).to(itype))
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert float(np.abs(M.values.double().numpy() - want).max()) < tol * float(np.abs(want).max())
    G = M.G
    assert G.layout == torch.sparse_csr and torch.equal(G.values(), M.values)
    assert torch.equal(M.GT.to_dense(), G.to_dense().T)


def test_coo_unsorted_columns_and_the_upper_triangle():
    ptr, idx = sr.stencil(4, 3, 3, 27)
    val, (lptr, lidx, lval) = _spd(ptr, idx, 7)
    n = len(ptr) - 1
    A = _csr(ptr, idx, val)
    want = sparse_fsai(A).values
    assert np.allclose(want.numpy(), sr.fsai(lptr, lidx, lval, lptr, lidx)[0], rtol=1e-12, atol=1e-14)
    assert torch.equal(sparse_fsai(A.to_sparse_coo()).values, want)
    rev = np.concatenate([np.arange(ptr[i], ptr[i + 1])[::-1] for i in range(n)])
    M = sparse_fsai(_csr(ptr, idx[rev], val[rev]))
    assert torch.equal(M.values, want) and torch.equal(M.col_indices, torch.from_numpy(lidx))
    # only tril(A) is read
    rows = np.repeat(np.arange(n), np.diff(ptr))
    junk = np.where(idx > rows, 99.0, val)
    assert torch.equal(sparse_fsai(_csr(ptr, idx, junk)).values, want)


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_a_pattern_given_as_a_tensor(layout):
    ptr, idx = sr.stencil(4, 3, 3, 27)
    val, (lptr, lidx, lval) = _spd(ptr, idx, 8)
    n = len(ptr) - 1
    sptr, sidx = sr.power_lower_pattern(ptr, idx, 2)
    want, _ = sr.fsai(lptr, lidx, lval, sptr, sidx)
    # the carrier: S itself plus junk in the upper triangle, with values that must not matter
    mask = sr.dense(sptr, sidx, np.ones(len(sidx))) != 0
    mask |= np.triu(np.random.default_rng(0).random((n, n)) < 0.2, 1)
    carrier = torch.from_numpy(np.where(mask, 7.5, 0.0))
    P = carrier.to_sparse_coo() if layout == "coo" else carrier.to_sparse_csr()
    A = _csr(ptr, idx, val)
    M = sparse_fsai(A, pattern=P)
    assert torch.equal(M.crow_indices, torch.from_numpy(sptr)) and torch.equal(M.col_indices, torch.from_numpy(sidx))
    assert np.allclose(M.values.numpy(), want, rtol=1e-11, atol=1e-14)
    # the recipe of the docstring gives the same S
    M2 = sparse_fsai(A, pattern=tsgu.sparse_spgemm(A, A))
    assert torch.equal(M2.col_indices, M.col_indices) and torch.equal(M2.values, M.values)
    assert "sparse_spgemm(A, A)" in sparse_fsai.__doc__
    # a 32-bit operand with a 64-bit carrier: G takes the index dtype of A
    M3 = sparse_fsai(_csr(ptr, idx, val, itype=torch.int32), pattern=P)
    assert M3.col_indices.dtype == torch.int32 and torch.equal(M3.values, M.values)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_application(dtype):
    ptr, idx = sr.stencil(4, 3, 3, 27)
    val, _ = _spd(ptr, idx, 9)
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype).requires_grad_(True)
    M = sparse_fsai(A)
    assert not M.values.requires_grad and M.T is M
    G = M.G.to_dense().double().numpy()
    R = torch.randn(n, 3, dtype=dtype, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    for got, r in ((M(R), R), (M.solve(R[:, 0]), R[:, 0]), (M.solve(R, transpose=True), R), (M.T(R), R), (M.matmul(R[:, 1]), R[:, 1])):
        want = G.T @ (G @ r.detach().double().numpy())
        assert got.shape == r.shape and got.dtype == dtype and not got.requires_grad
        assert float(np.linalg.norm(got.double().numpy() - want)) < tol * float(np.linalg.norm(want))


def test_preconditioned_cg_on_cpu_operands():
    """The table of the documents, float64, mean relative residual 1e-6: 56 plain, 29 with tril(A), 20 with tril(A²)."""
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    ptr, idx = sr.stencil(12, 12, 12, 7)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    d = np.abs(idx - rows)
    val = np.where(d == 0, 222.0, np.where(d == 1, -100.0, np.where(d == 12, -10.0, -1.0)))
    A = _csr(ptr, idx, val)
    b = torch.from_numpy(np.random.default_rng(0).standard_normal((len(ptr) - 1, 2)))
    its = []
    for pre in (None, sparse_fsai(A), sparse_fsai(A, pattern=tsgu.sparse_spgemm(A, A))):
        linear_cg(A, b, tolerance=1e-6, eps=1e-20, stop_updating_after=1e-20, max_iter=500, max_tridiag_iter=0, preconditioner=pre)
        info = last_solve_info("linear_cg")
        assert info["tolerance_reached"]
        its.append(info["iterations"])
    print("iterations plain / FSAI(A) / FSAI(A²):", its)
    assert its[2] < its[1] < its[0], its


# ---------------------------------------------------------------------------------------------------------------------------
# refusals


def test_refusals():
    ptr, idx = sr.band(12, 1)
    val, _ = _spd(ptr, idx, 1)
    A = _csr(ptr, idx, val)
    with pytest.raises(ValueError, match="sparse_fsai: A should be an instance of torch.Tensor"):
        sparse_fsai(np.eye(3))
    with pytest.raises(ValueError, match="sparse_fsai: A should be in either COO or CSR sparse format"):
        sparse_fsai(A.to_dense())
    with pytest.raises(ValueError, match="sparse_fsai: A should be in either COO or CSR sparse format"):
        sparse_fsai(A.to_sparse_csc())
    with pytest.raises(ValueError, match="sparse_fsai: A must be a 2-D sparse matrix"):
        sparse_fsai(torch.stack([A.to_dense()] * 2).to_sparse_coo())
    with pytest.raises(ValueError, match="sparse_fsai: A must be square"):
        sparse_fsai(torch.ones(3, 4, dtype=torch.float64).to_sparse_csr())
    for bad in (torch.bfloat16, torch.float16, torch.int64):
        with pytest.raises(TypeError, match="sparse_fsai: float32 and float64 operands only"):
            sparse_fsai(torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values().to(bad), A.shape))
    # the pattern
    with pytest.raises(ValueError, match="sparse_fsai: pattern should be a sparse tensor"):
        sparse_fsai(A, pattern=A.to_dense())
    with pytest.raises(ValueError, match=r"sparse_fsai: pattern must have the shape of A, got \(13, 13\) and \(12, 12\)"):
        sparse_fsai(A, pattern=_csr(*sr.band(13, 1), np.ones(37)))
    with pytest.raises(ValueError, match="sparse_fsai: pattern must be on the device of A"):
        sparse_fsai(A, pattern=A.to("meta"))
    hole = torch.ones(12, 12, dtype=torch.float64)
    hole[5, 5] = 0
    with pytest.raises(ValueError, match="row 5 does not store its diagonal"):
        sparse_fsai(A, pattern=hole.to_sparse_csr())
    with pytest.raises(ValueError, match="row 0 does not store its diagonal"):
        sparse_fsai(torch.tensor([[0.0, 1.0], [1.0, 2.0]], dtype=torch.float64).to_sparse_csr())


def test_a_row_longer_than_the_capacity_is_refused():
    cap, rows = _backend.fsai_geometry(torch.float64)
    assert cap >= 64 and rows >= 1 and _backend.fsai_geometry(torch.float32)[0] >= 64
    n = cap + 3
    ptr, idx = sr.band(n, 1)
    val, _ = _spd(ptr, idx, 2)
    A = _csr(ptr, idx, val)
    full = torch.ones(n, n, dtype=torch.float64).to_sparse_csr()
    # (the longest row is the one that is named)
    with pytest.raises(ValueError, match=rf"sparse_fsai: row {n - 1} of the pattern stores {n} lower-triangular entries, more than the {cap} "):
        sparse_fsai(A, pattern=full)
    with pytest.raises(ValueError, match=rf"row {n - 1} of the pattern"):        # (the cached plan refuses again)
        sparse_fsai(A, pattern=full)
    # exactly the capacity is accepted
    fits = torch.tril(torch.ones(n, n, dtype=torch.float64))
    fits[cap:, :] = torch.eye(n, dtype=torch.float64)[cap:, :]
    assert int(sparse_fsai(A, pattern=fits.to_sparse_csr()).info) == 0


def test_right_hand_side_refusals():
    ptr, idx = sr.band(12, 1)
    val, _ = _spd(ptr, idx, 1)
    M = sparse_fsai(_csr(ptr, idx, val))
    for bad in (torch.zeros(11, dtype=torch.float64), torch.zeros(12, 2, 2, dtype=torch.float64), torch.zeros((), dtype=torch.float64), None):
        with pytest.raises(ValueError, match=r"a right-hand side of shape \(12,\) or \(12, p\) is required"):
            M(bad)
    with pytest.raises(RuntimeError, match="expected the factor and R to have the same dtype, got torch.float64 and torch.float32"):
        M(torch.zeros(12, dtype=torch.float32))


def test_breakdown_is_reported_with_its_row():
    ptr, idx = sr.block_diagonal([5, 5, 5])
    val, _ = _spd(ptr, idx, 3)
    rows = np.repeat(np.arange(15), np.diff(ptr))
    clean = sparse_fsai(_csr(ptr, idx, val))
    bad = val.copy()
    bad[(rows == 6) & (idx == 6)] = -1.0
    with pytest.raises(RuntimeError, match="sparse_fsai: local matrix not positive definite in row 6"):
        sparse_fsai(_csr(ptr, idx, bad))
    M = sparse_fsai(_csr(ptr, idx, bad), check=False)
    assert int(M.info) == 7
    lrows = np.repeat(np.arange(15), np.diff(M.crow_indices.numpy()))
    untouched = (lrows < 6) | (lrows >= 10)                     # every row whose J does not contain 6
    assert torch.equal(M.values[untouched], clean.values[untouched])
    assert not torch.isfinite(M.values[lrows == 6]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the header

FAKE = 0x7F0000001000          # an address that is never dereferenced: every call below is refused on the host


def _call(lib, **kw):
    a = dict(vtype=0, itype=0, n=40, a_ptr=FAKE, a_idx=FAKE + 0x1000, a_val=FAKE + 0x2000, s_ptr=FAKE + 0x3000, s_idx=FAKE + 0x4000,
             s_nnz=500, order=None, out=FAKE + 0x5000, info=FAKE + 0x6000, workgroups_per_cu=1, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_csr_fsai(*a.values())


def test_launcher_refusals_on_the_host():
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert _call(lib) == BAD_ARG
    assert _call(lib, vtype=1, itype=1, order=FAKE + 0x7000) == BAD_ARG
    for vt in (2, 3, -1):                                                         # bf16 included
        assert _call(lib, vtype=vt) == BAD_DTYPE
    for it in (2, -1):
        assert _call(lib, itype=it) == BAD_DTYPE
    for size in ("n", "s_nnz"):
        assert _call(lib, **{size: -1}) == BAD_ARG
    for operand in ("a_ptr", "a_idx", "a_val", "s_ptr", "s_idx", "out", "info"):
        assert _call(lib, **{operand: None}) == BAD_ARG, operand
    assert _call(lib, device=0, vtype=2) == BAD_DTYPE and _call(lib, device=0, out=None) == BAD_ARG
    assert _call(lib, n=0) == OK and _call(lib, n=0, s_nnz=0, a_idx=None, a_val=None, s_idx=None, out=None) == OK


def test_the_geometry_query_and_the_backend_checks():
    lib = _backend.load_library()
    cap, rows = ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_csr_fsai_geometry(2, ref(cap), ref(rows)) == BAD_DTYPE and lib.tsgu_csr_fsai_geometry(5, ref(cap), ref(rows)) == BAD_DTYPE
    assert lib.tsgu_csr_fsai_geometry(0, None, ref(rows)) == BAD_ARG and lib.tsgu_csr_fsai_geometry(0, ref(cap), None) == BAD_ARG
    assert lib.tsgu_csr_fsai_geometry(1, ref(cap), ref(rows)) == OK and cap.value >= 64
    # the packed lower triangles of a wave's rows, 32·(capacity + 1) values, eight workgroups of one wave per CU in 160 KiB
    assert 8 * (32 * (cap.value + 1) * 8 + 64 * 8) <= 160 * 1024
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError, match="float32 and float64 values only"):
        _backend.csr_fsai(z, z, torch.zeros(2, dtype=torch.bfloat16), z, z, 1)
    with pytest.raises(RuntimeError, match="CPU operands are served by"):
        _backend.csr_fsai(z, z, torch.zeros(2), z, z, 1)
