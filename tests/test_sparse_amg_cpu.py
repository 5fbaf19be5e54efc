"""sparse_amg without a GPU: the exports, every refusal, the staged C-ABI header against `_backend.SIGNATURES_AMG` and the library,
the host-side refusals of the three launchers and the geometry query, and the CPU path (the same Python code over the torch-op
primitives of `_cpu.py`) against the numpy oracle `_amg_ref.py`: aggregates exactly, prolongators, operators and the cycle within
1e-12, the retry rule, symmetry, `refresh`, a matrix that does not coarsen, and the iteration count of a preconditioned CG."""

import ctypes
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import _abi_cases as A
import _amg_ref as ar
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import SparseAMG, _backend, sparse_amg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED_HEADER = os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "tsgu_hip_amg.h")

# name -> (lattice, weights, theta, coarse_size)
CASES = {
    "lap_6x5x4": ((6, 5, 4), (1.0, 1.0, 1.0), 0.0, 16),
    "lap_12": ((12, 12, 12), (1.0, 1.0, 1.0), 0.0, 64),
    "aniso_8x8x16": ((8, 8, 16), (1.0, 1.0, 1000.0), 0.08, 64),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    dims, weights, theta, coarse = CASES[name]
    ptr, idx, val = ar.stencil(dims, weights)
    return ptr, idx, val, theta, coarse


@functools.lru_cache(maxsize=None)
def oracle(name, sweeps=1):
    ptr, idx, val, theta, coarse = problem(name)
    return ar.hierarchy(ptr, idx, val, theta, sweeps, coarse, 10, np.float64)


def tensor(ptr, idx, val, dtype=torch.float64, layout="csr", itype=torch.int64):
    n = len(ptr) - 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        csr = torch.sparse_csr_tensor(torch.from_numpy(ptr).to(itype), torch.from_numpy(idx).to(itype), torch.from_numpy(val).to(dtype), (n, n))
        return csr if layout == "csr" else csr.to_sparse_coo().coalesce()


@functools.lru_cache(maxsize=None)
def built(name, layout="csr", sweeps=1):
    ptr, idx, val, theta, coarse = problem(name)
    return sparse_amg(tensor(ptr, idx, val, layout=layout), theta=theta, coarse_size=coarse, sweeps=sweeps)


def relerr(x, ref):
    return float(np.linalg.norm(np.asarray(x, dtype=np.float64) - ref) / np.linalg.norm(ref))


# ---- the public interface ---------------------------------------------------------------------------------------------------------------

def test_exports():
    assert "sparse_amg" in tsgu.__all__ and "SparseAMG" in tsgu.__all__
    assert tsgu.sparse_amg is sparse_amg and tsgu.SparseAMG is SparseAMG
    assert issubclass(SparseAMG, tsgu.sparse_factor._Factor)


def test_refusals():
    ptr, idx, val, _, _ = problem("lap_6x5x4")
    Asp = tensor(ptr, idx, val)
    with pytest.raises(ValueError, match="sparse_amg: A should be an instance of torch.Tensor"):
        sparse_amg(np.eye(3))
    with pytest.raises(ValueError, match="sparse_amg: A should be in either COO or CSR sparse format"):
        sparse_amg(torch.eye(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="sparse_amg: A must be a 2-D sparse matrix"):
        sparse_amg(torch.stack([torch.eye(4, dtype=torch.float64)] * 2).to_sparse_coo())
    with pytest.raises(ValueError, match="sparse_amg: A must be square"):
        sparse_amg(torch.ones((3, 4), dtype=torch.float64).to_sparse_coo())
    with pytest.raises(TypeError, match="sparse_amg: float32 and float64 operands only"):
        sparse_amg(torch.eye(4, dtype=torch.bfloat16).to_sparse_coo())
    hollow = torch.tensor([[2.0, -1.0, 0.0], [-1.0, 0.0, -1.0], [0.0, -1.0, 2.0]], dtype=torch.float64).to_sparse_coo()
    with pytest.raises(ValueError, match="sparse_amg: row 1 does not store its diagonal"):
        sparse_amg(hollow)
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError, match=r"sparse_amg: theta must be in \[0, 1\)"):
            sparse_amg(Asp, theta=bad)
    for name in ("sweeps", "max_levels", "coarse_size"):
        with pytest.raises(ValueError, match=f"sparse_amg: {name} must be at least 1"):
            sparse_amg(Asp, **{name: 0})
    negative = torch.diag(torch.tensor([1.0, 2.0, -3.0, 4.0], dtype=torch.float64)).to_sparse_coo()
    with pytest.raises(RuntimeError, match="sparse_amg: non-positive diagonal in row 2 of level 0"):
        sparse_amg(negative)
    M = sparse_amg(negative, check=False)
    assert isinstance(M.info, torch.Tensor) and int(M.info) == 3


def test_refusals_of_the_application_and_of_refresh():
    ptr, idx, val, _, _ = problem("lap_6x5x4")
    M = built("lap_6x5x4")
    n = len(ptr) - 1
    with pytest.raises(ValueError, match=rf"a right-hand side of shape \({n},\) or \({n}, p\) is required, got \({n - 1},\)"):
        M(torch.zeros(n - 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="is required, got"):
        M(torch.zeros((n, 2, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="is required, got ndarray"):
        M(np.zeros(n))
    with pytest.raises(RuntimeError, match="expected the factor and R to have the same dtype, got torch.float64 and torch.float32"):
        M(torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="sparse_amg: refresh needs a matrix on the pattern of the hierarchy"):
        M.refresh(tensor(ptr, idx, val, layout="coo"))
    p2, i2, v2 = ar.stencil((6, 5, 5))
    with pytest.raises(ValueError, match="sparse_amg: refresh needs a matrix on the pattern of the hierarchy"):
        M.refresh(tensor(p2, i2, v2))
    with pytest.raises(ValueError, match="sparse_amg: refresh needs values of torch.float64"):
        M.refresh(tensor(ptr, idx, val, dtype=torch.float32))
    with pytest.raises(IndexError):
        M.P(len(M.levels) - 1)
    with pytest.raises(IndexError):
        M.aggregates(len(M.levels) - 1)


def test_object_protocol():
    M = built("lap_12")
    n = M.shape[0]
    assert M.T is M and M.dtype == torch.float64 and M.device.type == "cpu" and M.shape == (n, n)
    R = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 3))).requires_grad_()
    for r in (R, R[:, 0]):
        y = M(r)
        assert y.shape == r.shape and not y.requires_grad
        assert torch.equal(y, M.solve(r)) and torch.equal(y, M.solve(r, transpose=True)) and torch.equal(y, M.matmul(r))
    assert relerr(M(R[:, 1]).numpy(), M(R)[:, 1].numpy()) <= 1e-14      # (columns do not mix)
    assert [lv["n"] for lv in M.levels] == [1728, 180, 5]   # (the sizes of the prototype)
    assert M.levels[-1]["solver"] == "dense" and all("solver" not in lv for lv in M.levels[:-1])
    assert M.operator_complexity == sum(lv["nnz"] for lv in M.levels) / M.levels[0]["nnz"]
    assert M.grid_complexity == sum(lv["n"] for lv in M.levels) / n
    for l, lv in enumerate(M.levels[:-1]):
        assert M.A(l).layout == torch.sparse_csr and M.P(l).layout == torch.sparse_csr
        assert tuple(M.P(l).shape) == (lv["n"], M.levels[l + 1]["n"]) and lv["aggregates"] == M.levels[l + 1]["n"]
        agg = M.aggregates(l)
        assert agg.shape == (lv["n"],) and not agg.dtype.is_floating_point and int(agg.max()) == lv["aggregates"] - 1


# ---- the staged header ----------------------------------------------------------------------------------------------------------------

ENTRIES = ("tsgu_amg_geometry", "tsgu_csr_amg_hop", "tsgu_amg_mis2_update", "tsgu_csr_affine_spmm")


def test_the_staged_header_is_bound():
    assert _backend.STAGED_AMG == {"tsgu_hip_amg.h": _backend.SIGNATURES_AMG}
    assert not set(_backend.STAGED_AMG) & (set(_backend.ABI) | set(_backend.STAGED))
    names = set(_backend.SIGNATURES_AMG)
    assert not any(names & set(table) for table in (*_backend.ABI.values(), *_backend.STAGED.values()))
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_amg.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_AMG)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_AMG[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION


def test_geometry():
    widths, tile = _backend.amg_geometry()
    assert widths == (4, 8, 16, 32, 64) and tile == 8
    lib = _backend.load_library()
    outs = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int()]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tsgu_amg_geometry(*refs) == A.OK and [o.value for o in outs] == [4, 64, 8]
    for k in range(3):
        assert lib.tsgu_amg_geometry(*[None if j == k else r for j, r in enumerate(refs)]) == A.BAD_ARG


# ---- host refusals: fake pointers that are never dereferenced, device = -1 (refused by set_device behind every other check) ----------

def _hop(**ch):
    a = dict(itype=0, n=8, nnz=8, ptr=0x10000, idx=0x20000, keys=0x30000, out=0x40000, group=8)
    a.update(ch)
    return _backend.load_library().tsgu_csr_amg_hop(*a.values(), -1, None)


def _update(**ch):
    a = dict(mode=1, n=8, key=0x10000, t=0x20000, out=0x30000, undecided=0x40000)
    a.update(ch)
    return _backend.load_library().tsgu_amg_mis2_update(*a.values(), -1, None)


def _affine(**ch):
    a = dict(vtype=0, itype=0, n_rows=8, n_cols=8, nnz=8, p=4, ptr=0x10000, idx=0x20000, val=0x30000, x=0x40000, ldx=4, c=0x50000, ldc=4,
             b=0x60000, ldb=4, w=0x70000, alpha=1.0, out=0x80000, ldo=4)
    a.update(ch)
    return _backend.load_library().tsgu_csr_affine_spmm(*a.values(), -1, None)


def test_host_refusals_of_amg_hop():
    assert _hop() == A.BAD_ARG                                             # (the base call: refused by set_device only)
    assert _hop(n=0) == A.OK                                               # (nothing to do comes back before it)
    assert [_hop(itype=v) for v in (2, 7, -1)] == [A.BAD_DTYPE] * 3
    assert _hop(n=-1) == A.BAD_ARG and _hop(nnz=-1) == A.BAD_ARG and _hop(n=1 << 31) == A.TOO_LARGE
    assert [_hop(group=g) for g in (0, 1, 2, 3, 12, 128, -8)] == [A.BAD_ARG] * 7
    assert [_hop(**{p: None}) for p in ("ptr", "idx", "keys", "out")] == [A.BAD_ARG] * 4
    for p, v in (("ptr", 0x10000), ("idx", 0x20000)):
        assert _hop(**{p: v + 2}) == A.BAD_ARG and _hop(**{p: v + 4}, itype=1) == A.BAD_ARG
    for p, v in (("keys", 0x30000), ("out", 0x40000)):
        assert _hop(**{p: v + 4}) == A.BAD_ARG
    assert _hop(out=0x30000) == A.BAD_ARG and _hop(out=0x30000 + 8 * 7) == A.BAD_ARG and _hop(keys=0x40000 + 8 * 7) == A.BAD_ARG
    # the order of the checks: the index type before everything
    assert _hop(itype=7, n=-1, ptr=None) == A.BAD_DTYPE


def test_host_refusals_of_mis2_update():
    assert _update() == A.BAD_ARG and _update(n=0) == A.OK
    assert [_update(mode=m) for m in (-1, 3, 7)] == [A.BAD_ARG] * 3
    assert _update(n=-1) == A.BAD_ARG and _update(n=1 << 31) == A.TOO_LARGE
    assert [_update(**{p: None}) for p in ("key", "t", "out", "undecided")] == [A.BAD_ARG] * 4
    for p, v in (("key", 0x10000), ("t", 0x20000), ("out", 0x30000), ("undecided", 0x40000)):
        assert _update(**{p: v + 4}) == A.BAD_ARG
    assert _update(out=0x20000) == A.BAD_ARG and _update(out=0x10000 + 8) == A.BAD_ARG          # out on t, out inside key
    # the initial keys read neither key nor t; the root keys read no t
    assert _update(mode=0, key=None, t=None, undecided=None, n=0) == A.OK
    assert _update(mode=0, out=None, key=None, t=None, undecided=None) == A.BAD_ARG
    assert _update(mode=2, key=None, t=None, undecided=None) == A.BAD_ARG
    assert _update(mode=2, out=0x30004, t=None, undecided=None) == A.BAD_ARG


def test_host_refusals_of_affine_spmm():
    assert _affine() == A.BAD_ARG                                          # (the base call: refused by set_device only)
    assert _affine(n_rows=0) == A.OK and _affine(p=0) == A.OK
    assert [_affine(vtype=v) for v in (2, 7, -1)] == [A.BAD_DTYPE] * 3     # (bf16 included)
    assert [_affine(itype=v) for v in (2, -1)] == [A.BAD_DTYPE] * 2
    assert [_affine(**{k: -1}) for k in ("n_rows", "n_cols", "nnz", "p")] == [A.BAD_ARG] * 4
    assert [_affine(**{k: None}) for k in ("ptr", "idx", "val", "x", "out")] == [A.BAD_ARG] * 5
    for k, v in (("ptr", 0x10000), ("idx", 0x20000), ("val", 0x30000), ("x", 0x40000), ("c", 0x50000), ("b", 0x60000), ("w", 0x70000),
                 ("out", 0x80000)):
        assert _affine(**{k: v + 2}) == A.BAD_ARG, k
    for k, v in (("val", 0x30000), ("x", 0x40000), ("c", 0x50000), ("b", 0x60000), ("w", 0x70000), ("out", 0x80000)):
        assert _affine(**{k: v + 4}, vtype=1) == A.BAD_ARG, k
    assert [_affine(**{k: 3}) for k in ("ldx", "ldc", "ldb", "ldo")] == [A.BAD_ARG] * 4
    assert _affine(c=None, ldc=0, b=None, ldb=0, w=None) == A.BAD_ARG      # (optional operands: only set_device is left to refuse)
    assert _affine(c=None, ldc=0, b=None, ldb=0, w=None, n_rows=0) == A.OK
    # Out on X, inside X, X inside Out: by address ranges
    assert _affine(out=0x40000) == A.BAD_ARG and _affine(out=0x40000 + 4 * 31) == A.BAD_ARG and _affine(x=0x80000 + 4 * 31) == A.BAD_ARG
    assert _affine(out=0x40000 + 4 * 32) == A.BAD_ARG                      # (… and just past it only set_device refuses)
    # Out may be C or B itself, nothing else that meets them
    assert _affine(out=0x50000 + 4, ldo=4) == A.BAD_ARG and _affine(out=0x50000, ldo=8) == A.BAD_ARG
    assert _affine(out=0x60000 + 4) == A.BAD_ARG and _affine(out=0x70000) == A.BAD_ARG
    far = dict(x=1 << 40, c=2 << 40, b=3 << 40, w=4 << 40, out=5 << 40, ldx=1 << 20, ldc=1 << 20, ldb=1 << 20, ldo=1 << 20)
    assert _affine(p=8 * 65535 + 1, **far) == A.TOO_LARGE and _affine(p=8 * 65535, **far) == A.BAD_ARG
    assert _affine(vtype=2, n_rows=-1, ptr=None) == A.BAD_DTYPE


# ---- the CPU path against the oracle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("name", CASES)
def test_hierarchy_against_the_oracle(name, layout):
    ref, M = oracle(name), built(name, layout)
    assert [lv["n"] for lv in M.levels] == [lv["n"] for lv in ref] and [lv["nnz"] for lv in M.levels] == [lv["nnz"] for lv in ref]
    assert [lv["theta"] for lv in M.levels] == [lv["theta"] for lv in ref]
    assert M.levels[-1]["solver"] == ref[-1]["solver"] == "dense"
    for l, lv in enumerate(ref):
        err_a = relerr(M.A(l).to_dense().numpy(), lv["A"])
        assert np.array_equal((M.A(l).to_dense() != 0).numpy() | lv["mask"], lv["mask"])
        assert np.array_equal(M.A(l).crow_indices().numpy(), lv["ptr"]) and np.array_equal(M.A(l).col_indices().numpy(), lv["idx"])
        print(f"{name} {layout} level {l}: n {lv['n']}, |A - A_ref| / |A_ref| = {err_a:.2e}")
        assert err_a <= 1e-12
        if lv["agg"] is not None:
            assert np.array_equal(M.aggregates(l).numpy(), lv["agg"]) and M.levels[l]["aggregates"] == lv["n_c"]
            err_p = relerr(M.P(l).to_dense().numpy(), lv["P"])
            print(f"    |P - P_ref| / |P_ref| = {err_p:.2e}")
            assert err_p <= 1e-12
    assert len(ref) >= 2


@pytest.mark.parametrize("sweeps", [1, 2])
@pytest.mark.parametrize("name", CASES)
def test_cycle_against_the_oracle(name, sweeps):
    M = built(name, sweeps=sweeps)
    n = M.shape[0]
    b = np.random.default_rng(7).standard_normal((n, 5))
    want = ar.cycle(oracle(name, sweeps), b, np.float64)
    for cols in (slice(0, 5), slice(0, 1)):
        err = relerr(M(torch.from_numpy(b[:, cols].copy())).numpy(), want[:, cols])
        print(f"{name} sweeps {sweeps} p {want[:, cols].shape[1]}: cycle error {err:.2e}")
        assert err <= 1e-12
    assert relerr(M(torch.from_numpy(b[:, 2].copy())).numpy(), want[:, 2]) <= 1e-12


def test_the_retry_rule_fires_on_the_anisotropic_case():
    thetas = [lv["theta"] for lv in oracle("aniso_8x8x16")]
    assert thetas[0] == 0.08 and 0.0 in thetas[1:-1], thetas
    got = [lv["theta"] for lv in built("aniso_8x8x16").levels]
    assert got == thetas and got[-1] is None


@pytest.mark.parametrize("name", CASES)
def test_the_cycle_is_symmetric(name):
    M = built(name)
    rng = np.random.default_rng(11)
    u, v = (torch.from_numpy(rng.standard_normal(M.shape[0])) for _ in range(2))
    a, b = float(u @ M(v)), float(v @ M(u))
    print(f"{name}: <u, M v> = {a!r}, <v, M u> = {b!r}")
    assert abs(a - b) <= 1e-12 * abs(a)
    assert float(u @ M(u)) > 0 and float(v @ M(v)) > 0


@pytest.mark.parametrize("name", ["lap_12", "aniso_8x8x16"])
def test_refresh_equals_a_fresh_build(name):
    ptr, idx, val, theta, coarse = problem(name)
    M = sparse_amg(tensor(ptr, idx, val), theta=theta, coarse_size=coarse)
    held = [(lv.ptr.data_ptr(), lv.idx.data_ptr()) for lv in M._levels]
    held_p = [(M.P(l).crow_indices().data_ptr(), M.P(l).col_indices().data_ptr()) for l in range(len(M.levels) - 1)]
    aggs = [M.aggregates(l).clone() for l in range(len(M.levels) - 1)]
    scaled = tensor(ptr, idx, 2.5 * val)
    assert M.refresh(scaled) is M
    F = sparse_amg(tensor(ptr, idx, 2.5 * val), theta=theta, coarse_size=coarse)
    assert M.levels == F.levels
    assert held == [(lv.ptr.data_ptr(), lv.idx.data_ptr()) for lv in M._levels]
    assert held_p == [(M.P(l).crow_indices().data_ptr(), M.P(l).col_indices().data_ptr()) for l in range(len(M.levels) - 1)]
    for l in range(len(M.levels)):
        assert torch.equal(M.A(l).values(), F.A(l).values()) and torch.equal(M._levels[l].w, F._levels[l].w)
        if l < len(M.levels) - 1:
            assert torch.equal(M.P(l).values(), F.P(l).values()) and torch.equal(M.aggregates(l), aggs[l])
    assert torch.equal(M._levels[-1].inv, F._levels[-1].inv)
    R = torch.from_numpy(np.random.default_rng(5).standard_normal((M.shape[0], 2)))
    assert torch.equal(M(R), F(R))


def test_a_matrix_that_does_not_coarsen():
    n = 5000
    d = torch.from_numpy(np.random.default_rng(2).uniform(1.0, 3.0, n))
    ar_ = torch.arange(n + 1, dtype=torch.int64)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        D = torch.sparse_csr_tensor(ar_, ar_[:-1], d, (n, n))
        caught.clear()
        M = sparse_amg(D, coarse_size=64)
    ours = [w for w in caught if "sparse_amg" in str(w.message)]
    assert len(ours) == 1 and "does not coarsen" in str(ours[0].message)
    assert len(M.levels) == 1 and M.levels[0]["solver"] == "smoother" and M.levels[0]["n"] == n
    assert M.operator_complexity == 1.0 and M.grid_complexity == 1.0
    r = torch.from_numpy(np.random.default_rng(3).standard_normal(n))
    # 2·sweeps = 2 sweeps of damped Jacobi from a zero guess; ρ̂ = 1 on a diagonal matrix, so the weight is (4/3) / d
    w = 4.0 / 3.0
    x = w * r / d
    x = x + w * (r - d * x) / d
    assert relerr(M(r).numpy(), x.numpy()) <= 1e-14


def test_preconditioned_cg_halves_the_iterations():
    """linear_cg on the 12³ Laplacian, float64, 1e-8: the numpy prototype takes 14 iterations with the cycle against 49 without."""
    from torchsparsegradutils_amd.utils import last_solve_info, linear_cg

    ptr, idx, val, _, _ = problem("lap_12")
    Asp, M = tensor(ptr, idx, val), built("lap_12")
    n = len(ptr) - 1
    b = np.random.default_rng(0).standard_normal((n, 1))
    D = ar.to_dense(ptr, idx, val)[0]
    x64 = np.linalg.solve(D, b)
    its = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, pre in (("plain", None), ("amg", M)):
            x = linear_cg(Asp, torch.from_numpy(b), tolerance=1e-8, eps=1e-20, stop_updating_after=1e-20, max_iter=500, max_tridiag_iter=0,
                          preconditioner=pre)
            info = last_solve_info("linear_cg")
            its[name] = info["iterations"]
            err = relerr(x.numpy(), x64)
            print(f"{name}: {info['iterations']} iterations, relative error {err:.2e}")
            assert info["tolerance_reached"] and err < 200 * 1e-8, (name, info, err)
    ref_plain = ar.pcg(lambda v: D @ v, b[:, 0])[1]
    ref_amg = ar.pcg(lambda v: D @ v, b[:, 0], lambda r: ar.cycle(oracle("lap_12"), r[:, None], np.float64)[:, 0])[1]
    print(f"numpy PCG: plain {ref_plain}, amg {ref_amg}")
    assert 2 * its["amg"] <= its["plain"], its
