"""sparse_ilu0 / sparse_ic0 without a GPU: the numpy oracle of the GPU tests against dense factorisations where the incomplete factor
is the exact one, the public API on CPU operands against the oracle, every refusal, and the C-ABI header of the factorisations
with its host-side refusals."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK
import _factor_ref as fr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern, sparse_ic0, sparse_ilu0

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_FILL = {"tridiagonal": lambda: fr.band(40, 1), "blocks": lambda: fr.block_diagonal([4, 1, 9, 6]), "downward_arrow": lambda: fr.downward_arrow(25)}


def _csr(ptr, idx, val, dtype=torch.float64, itype=torch.int64):
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(ptr).to(itype), torch.from_numpy(idx).to(itype), torch.from_numpy(np.asarray(val)).to(dtype),
                                   (n, n))


def test_exports():
    assert {"sparse_ilu0", "sparse_ic0", "SparseILU0", "SparseIC0"} <= set(tsgu.__all__)
    from torchsparsegradutils_amd.sparse_factor import __all__ as mod_all

    assert mod_all == ["sparse_ilu0", "sparse_ic0", "SparseILU0", "SparseIC0"]


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle, where the incomplete factor is the exact one


@pytest.mark.parametrize("pattern", NO_FILL)
def test_the_oracle_is_the_dense_factorisation_without_fill(pattern):
    ptr, idx = NO_FILL[pattern]()
    val = fr.dominant_values(ptr, idx, seed=1)
    D = fr.dense(ptr, idx, val)
    out, info = fr.ilu0(ptr, idx, val)
    L, U = fr.split_lu(ptr, idx, out)
    Ld, Ud = fr.lu_nopivot(D)
    assert info == 0 and np.allclose(L, Ld, rtol=1e-12, atol=1e-14) and np.allclose(U, Ud, rtol=1e-12, atol=1e-14)
    assert np.allclose(L @ U, D, rtol=1e-13, atol=1e-13)
    sym = fr.dominant_values(ptr, idx, seed=2, symmetric=True)
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, sym)
    out, info = fr.ic0(lptr, lidx, lval)
    assert info == 0 and np.allclose(fr.dense(lptr, lidx, out), np.linalg.cholesky(fr.dense(ptr, idx, sym)), rtol=1e-12, atol=1e-14)


def test_the_oracle_drops_fill_and_keeps_the_pattern_exact():
    ptr, idx = fr.stencil(4, 3, 3, 27)
    val = fr.dominant_values(ptr, idx, seed=3, symmetric=True)
    out, _ = fr.ilu0(ptr, idx, val)
    L, U = fr.split_lu(ptr, idx, out)
    D = fr.dense(ptr, idx, val)
    err, bound = fr.pattern_residual_bound(ptr, idx, L, U, D, 2.0 ** -53)
    assert (err <= bound).all() and float(np.abs(L @ U - D).max()) > 1e-3            # exact on the pattern, not off it
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, val)
    lo, _ = fr.ic0(lptr, lidx, lval)
    Lc = fr.dense(lptr, lidx, lo)
    err, bound = fr.pattern_residual_bound(lptr, lidx, Lc, Lc.T, D, 2.0 ** -53)
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------------------------
# public API on CPU operands


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_operands_against_the_oracle(dtype, itype):
    npdt = np.float32 if dtype == torch.float32 else np.float64
    ptr, idx = fr.stencil(4, 3, 5, 27)
    val = fr.dominant_values(ptr, idx, seed=4).astype(npdt)
    M = sparse_ilu0(_csr(ptr, idx, val, dtype, itype))
    want, _ = fr.ilu0(ptr, idx, val, dtype=npdt)
    assert M.values.dtype == dtype and np.array_equal(M.values.numpy().view(np.uint8), want.view(np.uint8))      # the ILU(0) bits
    assert M.col_indices.dtype == itype and int(M.info) == 0
    sym = fr.dominant_values(ptr, idx, seed=5, symmetric=True).astype(npdt)
    lptr, lidx, lval, _ = fr.lower_csr(ptr, idx, sym)
    C = sparse_ic0(_csr(ptr, idx, sym, dtype, itype))
    want, _ = fr.ic0(lptr, lidx, lval.astype(np.float64))
    assert C.values.dtype == dtype and np.allclose(C.values.double().numpy(), want, rtol=1e-5 if npdt == np.float32 else 1e-13)
    assert torch.equal(C.crow_indices, torch.from_numpy(lptr).to(itype)) and torch.equal(C.col_indices, torch.from_numpy(lidx).to(itype))


def test_only_the_lower_triangle_is_read_by_ic0():
    ptr, idx = fr.stencil(3, 3, 3, 7)
    val = fr.dominant_values(ptr, idx, seed=6, symmetric=True)
    rows = np.repeat(np.arange(27), np.diff(ptr))
    other = np.where(idx > rows, 77.0, val)
    assert torch.equal(sparse_ic0(_csr(ptr, idx, val)).values, sparse_ic0(_csr(ptr, idx, other)).values)


def test_coo_and_unsorted_columns():
    ptr, idx = fr.random_pattern(60, 6, seed=2)
    val = fr.dominant_values(ptr, idx, seed=7)
    A = _csr(ptr, idx, val)
    want = sparse_ilu0(A)
    assert want._plan.gather.col.data_ptr() == A.col_indices().data_ptr()            # canonical already: A's own index tensors
    assert torch.equal(sparse_ilu0(A.to_sparse_coo()).values, want.values)
    rev = np.concatenate([np.arange(ptr[i], ptr[i + 1])[::-1] for i in range(60)])
    unsorted = _csr(ptr, idx[rev], val[rev])
    for _ in range(2):                                                               # (the second call finds the cached permutation)
        M = sparse_ilu0(unsorted)
        assert torch.equal(M.values, want.values) and torch.equal(M.col_indices, torch.from_numpy(idx))
    assert isinstance(_pattern.from_csr(unsorted).core.own["factor"], _pattern.FactorPlan)
    assert torch.equal(sparse_ic0(unsorted).values, sparse_ic0(A).values)


def test_shift():
    ptr, idx = fr.band(12, 2)
    val = fr.dominant_values(ptr, idx, seed=8, symmetric=True)
    rows = np.repeat(np.arange(12), np.diff(ptr))
    scaled = np.where(idx == rows, val * 1.5, val)
    assert torch.equal(sparse_ilu0(_csr(ptr, idx, val), shift=0.5).values, sparse_ilu0(_csr(ptr, idx, scaled)).values)
    assert torch.equal(sparse_ic0(_csr(ptr, idx, val), shift=0.5).values, sparse_ic0(_csr(ptr, idx, scaled)).values)
    want, _ = fr.ilu0(ptr, idx, val, shift=0.5)
    assert np.array_equal(sparse_ilu0(_csr(ptr, idx, val), shift=0.5).values.numpy(), want)
    # the usual remedy: an indefinite matrix on which IC(0) breaks down goes through with a shift
    weak = np.where(idx == rows, 1.0, 0.6)
    with pytest.raises(RuntimeError, match="non-positive pivot in row"):
        sparse_ic0(_csr(ptr, idx, weak))
    assert int(sparse_ic0(_csr(ptr, idx, weak), shift=2.0).info) == 0


def test_breakdown_is_reported_with_its_row():
    ptr, idx = fr.band(20, 1)
    val = fr.dominant_values(ptr, idx, seed=9)
    rows = np.repeat(np.arange(20), np.diff(ptr))
    at = lambda i, j: int(ptr[i] + np.nonzero(idx[ptr[i]:ptr[i + 1]] == j)[0][0])  # noqa: E731
    val[at(9, 9)] = (val[at(9, 8)] / fr.ilu0(ptr, idx, val)[0][at(8, 8)]) * fr.ilu0(ptr, idx, val)[0][at(8, 9)]      # the pivot of row 9 cancels
    with pytest.raises(RuntimeError, match="zero pivot in row 9"):
        sparse_ilu0(_csr(ptr, idx, val))
    M = sparse_ilu0(_csr(ptr, idx, val), check=False)
    want, info = fr.ilu0(ptr, idx, val)
    assert int(M.info) == 10 == info
    assert np.array_equal(M.values.numpy()[rows <= 9], want[rows <= 9]) and not np.isfinite(M.values.numpy()[rows == 10]).all()
    sym = fr.dominant_values(ptr, idx, seed=10, symmetric=True)
    sym[at(12, 12)] = -3.0
    with pytest.raises(RuntimeError, match="non-positive pivot in row 12"):
        sparse_ic0(_csr(ptr, idx, sym))
    C = sparse_ic0(_csr(ptr, idx, sym), check=False)
    assert int(C.info) == 13 and C.info.dtype == torch.int64


def test_refusals():
    ptr, idx = fr.band(6, 1)
    val = fr.dominant_values(ptr, idx, seed=1)
    A = _csr(ptr, idx, val)
    for f in (sparse_ilu0, sparse_ic0):
        name = f.__name__
        with pytest.raises(ValueError, match=f"{name}: A must be square, got \\(6, 7\\)"):
            f(torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values(), (6, 7)))
        with pytest.raises(ValueError, match=f"{name}: A must be a 2-D sparse matrix \\(batched operands are not supported\\), got 3 dimensions"):
            f(torch.stack([A.to_dense(), A.to_dense()]).to_sparse_csr())
        with pytest.raises(ValueError, match=f"{name}: A must be a 2-D sparse matrix"):
            f(torch.stack([A.to_dense(), A.to_dense()]).to_sparse_coo())
        with pytest.raises(TypeError, match=f"{name}: float32 and float64 operands only, got torch.bfloat16"):
            f(_csr(ptr, idx, val, torch.bfloat16))
        with pytest.raises(ValueError, match=f"{name}: A should be in either COO or CSR sparse format"):
            f(A.to_dense())
        with pytest.raises(ValueError, match=f"{name}: A should be an instance of torch.Tensor"):
            f(None)
        # row 3 does not store its diagonal
        keep = np.ones(idx.size, dtype=bool)
        keep[fr.diag_positions(ptr, idx)[3]] = False
        p2 = ptr.copy()
        p2[4:] -= 1
        with pytest.raises(ValueError, match="row 3 does not store its diagonal"):
            f(_csr(p2, idx[keep], val[keep]))
        # row 2 stores column 1 twice: adjacent, and separated by another column (found after sorting)
        for cols in ([1, 1, 2, 3], [1, 2, 1, 3]):
            p3 = np.array([0, 2, 5, 9, 12, 15, 17])
            i3 = np.array([0, 1, 0, 1, 2] + cols + [2, 3, 4, 3, 4, 5, 4, 5])
            with pytest.raises(ValueError, match="row 2 stores a column more than once"):
                f(torch.sparse_csr_tensor(torch.from_numpy(p3), torch.from_numpy(i3), torch.ones(17, dtype=torch.float64), (6, 6)))
    M = sparse_ilu0(A)
    with pytest.raises(ValueError, match="a right-hand side of shape \\(6,\\) or \\(6, p\\) is required"):
        M(torch.zeros(5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="the same dtype"):
        M(torch.zeros(6))


# ---------------------------------------------------------------------------------------------------------------------------
# the application objects


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_application_objects_on_cpu_operands(dtype):
    tol = 1e-4 if dtype == torch.float32 else 1e-12
    ptr, idx = fr.stencil(3, 4, 3, 27)
    val = fr.dominant_values(ptr, idx, seed=11)
    n = len(ptr) - 1
    A = _csr(ptr, idx, val, dtype, torch.int32).requires_grad_(True)
    M = sparse_ilu0(A)
    assert not M.values.requires_grad and M.dtype == dtype and M.device.type == "cpu" and M.shape == (n, n)
    L, U = M.L, M.U
    assert L.layout == torch.sparse_csr and U.layout == torch.sparse_csr
    Ld, Ud = L.to_dense(), U.to_dense()
    assert torch.equal(torch.diagonal(Ld), torch.ones(n, dtype=dtype)) and torch.equal(torch.triu(Ld, 1), torch.zeros_like(Ld))
    assert torch.equal(torch.tril(Ud, -1), torch.zeros_like(Ud))
    combined = torch.sparse_csr_tensor(M.crow_indices, M.col_indices, M.values, (n, n)).to_dense()
    assert torch.equal(torch.tril(Ld, -1) + Ud, combined)                       # L and U reconstruct `values`
    LU = (Ld.double() @ Ud.double())
    R = torch.from_numpy(np.random.default_rng(0).standard_normal((n, 3))).to(dtype)

    def rel(a, b):
        return float(torch.linalg.norm(a.double() - b) / torch.linalg.norm(b))

    assert rel(M(R), torch.linalg.solve(LU, R.double())) < tol
    assert M(R[:, 0]).shape == (n,) and rel(M(R[:, 0]), torch.linalg.solve(LU, R[:, 0].double())) < tol
    assert rel(M.solve(R, transpose=True), torch.linalg.solve(LU.T, R.double())) < tol
    assert rel(M.T(R), torch.linalg.solve(LU.T, R.double())) < tol and rel(M.T.T(R), torch.linalg.solve(LU, R.double())) < tol
    assert not M(R.clone().requires_grad_(True)).requires_grad

    sym = fr.dominant_values(ptr, idx, seed=12, symmetric=True)
    C = sparse_ic0(_csr(ptr, idx, sym, dtype, torch.int32))
    Lc = C.L.to_dense().double()
    assert C.T is C and torch.equal(torch.triu(Lc, 1), torch.zeros_like(Lc))
    assert rel(C(R), torch.linalg.solve(Lc @ Lc.T, R.double())) < tol and rel(C.solve(R[:, 1], transpose=True), torch.linalg.solve(Lc @ Lc.T, R[:, 1].double())) < tol


def test_ic0_factor_as_precision_tril_on_cpu():
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormal

    ptr, idx = fr.band(9, 1)
    val = fr.dominant_values(ptr, idx, seed=5, symmetric=True)
    loc = torch.zeros(9, dtype=torch.float64)
    xs = torch.from_numpy(np.random.default_rng(7).standard_normal((4, 9)))
    got = SparseMultivariateNormal(loc, precision_tril=sparse_ic0(_csr(ptr, idx, val)).L).log_prob(xs)
    want = torch.distributions.MultivariateNormal(loc, precision_matrix=torch.from_numpy(fr.dense(ptr, idx, val))).log_prob(xs)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: the header of the factorisations

HEADER = os.path.join(ROOT, "include", "tsgu_hip_factor.h")
FAKE = 0x7F0000001000          # an address that is never dereferenced: every call below is refused on the host


def _call(lib, name, **kw):
    a = dict(vtype=0, itype=0, n=40, nnz=500, ptr=FAKE, idx=FAKE + 0x1000, diag_pos=FAKE + 0x2000, val=FAKE + 0x3000, shift=0.0,
             out=FAKE + 0x4000, work=FAKE + 0x5000, info=FAKE + 0x6000, workgroups_per_cu=1, device=-1, stream=None)
    a.update(kw)
    return getattr(lib, name)(*a.values())


@pytest.mark.parametrize("name", ["tsgu_csr_ilu0", "tsgu_csr_ic0"])
def test_launcher_refusals_on_the_host(name):
    lib = _backend.load_library()
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert _call(lib, name) == BAD_ARG
    assert _call(lib, name, vtype=1, itype=1) == BAD_ARG
    assert _call(lib, name, vtype=2) == BAD_DTYPE                                 # bf16: a bf16 factor is of no use
    for vt in (3, -1):
        assert _call(lib, name, vtype=vt) == BAD_DTYPE
    for it in (2, -1):
        assert _call(lib, name, itype=it) == BAD_DTYPE
    for size in ("n", "nnz"):
        assert _call(lib, name, **{size: -1}) == BAD_ARG
    for operand in ("ptr", "idx", "diag_pos", "val", "out", "work", "info"):
        assert _call(lib, name, **{operand: None}) == BAD_ARG, operand
    assert _call(lib, name, device=0, vtype=2) == BAD_DTYPE and _call(lib, name, device=0, out=None) == BAD_ARG
    assert _call(lib, name, n=0) == OK and _call(lib, name, n=0, nnz=0, idx=None, val=None, out=None) == OK
    assert _call(lib, name, out=FAKE + 0x3000) == BAD_ARG                         # out == val passes the checks (in place is allowed)
    assert "out == val is allowed" in open(HEADER).read()


def test_the_geometry_and_work_queries():
    lib = _backend.load_library()
    cap, waves = ctypes.c_int(0), ctypes.c_int(0)
    ref = ctypes.byref
    assert lib.tsgu_csr_factor_geometry(2, ref(cap), ref(waves)) == BAD_DTYPE and lib.tsgu_csr_factor_geometry(5, ref(cap), ref(waves)) == BAD_DTYPE
    assert lib.tsgu_csr_factor_geometry(0, None, ref(waves)) == BAD_ARG and lib.tsgu_csr_factor_geometry(0, ref(cap), None) == BAD_ARG
    src = open(os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "ilu_impl.h")).read()
    caps = [int(c) for c in re.findall(r"kCap\s*=\s*(\d+);", src)]
    assert [_backend.factor_geometry(torch.float32), _backend.factor_geometry(torch.float64)] == [(caps[0], 4), (caps[1], 4)]
    # a workgroup's slices (32-bit columns + values, four waves) leave room for eight workgroups in a CU's 160 KiB of LDS
    assert 8 * 4 * caps[0] * (4 + 4) <= 160 * 1024 and 8 * 4 * caps[1] * (4 + 8) <= 160 * 1024
    sizes = [lib.tsgu_csr_factor_work_bytes(n) for n in (0, 1, 4, 5, 1000)]
    assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[4] - sizes[0] == 4000
    assert lib.tsgu_csr_factor_work_bytes(-1) == 0
    with pytest.raises(TypeError, match="float32 and float64 values only"):
        _backend.csr_factor("ilu0", *(torch.zeros(2, dtype=torch.int32),) * 3, torch.zeros(2, dtype=torch.bfloat16), 1)
