"""LSMR on the fused kernels (csrc/lsmr.hip): every step against float64 numpy (tests/_lsmr_cases.py), the public `lsmr`
against dense float64 least squares, column independence, and a long solve that replays a graph.

Step bounds are derived (u = 2^-24 or 2^-53 of the value type).  A vector output: one rounding per operation of the contract and
one per coefficient rounded to the value type (`ref_vector` carries the count); fp64 doubles it for the float64 reference's own
roundings.  A partial row is compared with the squares of the kernel's own output: m roundings for the m <= R rows of a workgroup,
gamma_m = m u / (1 - m u).  Scalar phases work in double on sums in the value type: with integer-valued partials the sums are exact
and what is left is a chain of fewer than 64 double operations on inputs of order one, 64 * 2^-53 < 2^-46 relative to max(1, |ref|)
(2^-44 is asserted); BETA is also run on random partials, where the norm carries gamma_rows of the value type."""

import sys

import numpy as np
import pytest
import torch

import _lsmr_cases as C
from torchsparsegradutils_amd import _backend
from torchsparsegradutils_amd.utils import _graph, last_solve_info, lsmr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
WIDTHS = [1, 3, 4, 5, 64, 65, 256]
TIGHT = dict(atol=1e-12, btol=1e-12, maxiter=400)
lsmr_mod = sys.modules[lsmr.__module__]
POSITIVE = [0, 1, 3, 4, 11, 14, 15, 16, 17, 18, 19, 20, 21, 27]           # norms, radii and sums of squares of the scalar block


def _u(td):
    return 2.0 ** -24 if td == torch.float32 else 2.0 ** -53


def _dev(a, td):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=td)


def _state(rng, p, stop=0):
    scal = rng.uniform(0.5, 1.5, (28, p)) * np.where(rng.random((28, p)) < 0.5, -1.0, 1.0)
    scal[POSITIVE] = np.abs(scal[POSITIVE])
    done = (np.arange(p) % 3 == 1).astype(np.int32)
    scal[25, done != 0] = 0.0                                             # a finished column: step 0
    flags = np.concatenate([[stop, 4], done, np.full(p, 2)]).astype(np.int32)
    return scal, flags


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("p", WIDTHS)
def test_vector_steps(td, p):
    lib, rng, u = _backend.load_library(), np.random.default_rng(p), _u(td) * (1 if td == torch.float32 else 2)
    vt, nd = _backend.vtype_of(torch.empty(0, dtype=td)), np.float32 if td == torch.float32 else np.float64
    wide = 16 // np.dtype(nd).itemsize
    R = (256 // -(-p // (wide if p % wide == 0 else 1))) * 4             # rows per workgroup (vec_geom, csrc/krylov_common.h)
    assert lib.tsgu_cg_num_blocks(vt, R, p) == 1 and lib.tsgu_cg_num_blocks(vt, R + 1, p) == 2
    for n in sorted({1, max(R - 1, 1), R, R + 1, 3 * R + 2}):
        nb = lib.tsgu_cg_num_blocks(vt, n, p)
        scal, flags = _state(rng, p)
        arrs = [rng.standard_normal((n, p)).astype(nd) for _ in range(4)]
        for which, names in ((0, ("y",)), (1, ("x", "h", "hbar"))):
            def run(stop=0):
                y, a1, h, hbar = (_dev(a, td) for a in arrs)
                part = torch.full((nb, p), -7.0, dtype=td, device=DEV)
                fl = _dev(flags, torch.int32)
                fl[0] = stop
                _backend.launch("tsgu_lsmr_vector", DEV, vt, which, n, p, y, a1, h if which else None, hbar if which else None,
                                _dev(scal, torch.float64), fl, part)
                assert np.array_equal(a1.cpu().numpy(), arrs[1])
                return [t.cpu().numpy() for t in ((y, h, hbar) if which else (y,))], part.cpu().numpy()
            got, part = run()
            ref, err = C.ref_vector(which, scal, *(a.astype(np.float64) for a in arrs))
            for name, g, r, e in zip(names, got, ref, err):
                assert np.all(np.abs(g - r) <= u * e), (name, which, n, p, float(np.max(np.abs(g - r) / np.maximum(u * e, 1e-300))))
            sq = got[0].astype(np.float64) ** 2
            sums = np.stack([sq[b * R:(b + 1) * R].sum(0) for b in range(nb)])
            m = min(R, n)
            assert np.all(np.abs(part - sums) <= m * u / (1 - m * u) * sums), ("partial", which, n, p)
            if which:
                assert np.array_equal(got[0][:, scal[25] == 0], arrs[0][:, scal[25] == 0])      # a finished column's x keeps its bits
            again, part2 = run()
            assert all(np.array_equal(a, b) for a, b in zip(got, again)) and np.array_equal(part, part2)
            idle, part0 = run(stop=1)
            assert all(np.array_equal(a, b) for a, b in zip(idle, (arrs[0], arrs[2], arrs[3]))) and np.all(part0 == -7.0)


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("phase", [0, 1, 2])
def test_scalar_phases(td, phase):
    lib, rng, u = _backend.load_library(), np.random.default_rng(10 + phase), _u(td)
    vt = _backend.vtype_of(torch.empty(0, dtype=td))
    args = (0.3, 0.1, 0.5, 1e-8, float(torch.finfo(td).eps))              # damp, atol, btol, ctol, eps: some columns stop, some go on
    for p in WIDTHS:
        for rows, exact in ((1, True), (5, True), (1030, True), (5, False), (1030, False)):     # 1030 > 4 * 256 rows: folded first
            if not exact and phase != 0:
                continue
            partial = rng.integers(0, 4, (rows, p)).astype(np.float64) if exact else rng.uniform(0.5, 1.5, (rows, p))
            partial = _dev(partial, td)
            scal, flags = _state(rng, p)

            def run(stop=0):
                sc, fl = _dev(scal, torch.float64), _dev(flags, torch.int32)
                fl[0] = stop
                fold = torch.empty((lib.tsgu_cg_fold_rows(), p), dtype=td, device=DEV)
                _backend.launch("tsgu_lsmr_scalar", DEV, vt, phase, partial, rows, fold, sc, fl, *args, p)
                return sc.cpu().numpy(), fl.cpu().numpy()
            got, gfl = run()
            ref, rfl = C.ref_scalar(phase, partial.double().cpu().numpy().sum(0), scal, flags, *args)
            assert np.array_equal(gfl, rfl), (phase, p, rows)
            rel = 2.0 ** -44 + (0.0 if exact else rows * u / (1 - rows * u))
            assert np.all(np.abs(got - ref) <= rel * np.maximum(1.0, np.abs(ref))), (phase, p, rows)
            again = run()
            assert np.array_equal(got, again[0]) and np.array_equal(gfl, again[1])
            idle, ifl = run(stop=1)
            assert np.array_equal(idle, scal) and np.array_equal(ifl[1:], flags[1:])


def _operand(A, td, layout):
    A = A.to(device=DEV, dtype=td)
    return {"coo": A.to_sparse_coo, "csr": A.to_sparse_csr, "dense": lambda: A}[layout]()


def _host_loop(*args, **kw):
    lsmr_mod.ENABLE_FUSED = False
    try:
        return lsmr(*args, **kw)
    finally:
        lsmr_mod.ENABLE_FUSED = True


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("layout", ["coo", "csr"])
@pytest.mark.parametrize("td", DTYPES)
def test_lsmr_against_dense_least_squares(td, layout, k):
    A = C.tall()                                                          # cond(A) = 9.3 (tests/test_lsmr_cpu.py holds it in (8, 12))
    B = C.rhs(A.shape[0], k)
    X = C.dense_lstsq(A, B)
    As, b = _operand(A, td, layout), B.to(device=DEV, dtype=td)
    b = b[:, 0] if k == 1 else b
    if td == torch.float64:
        x, its = lsmr(As, b, **TIGHT)
        assert x.shape == ((A.shape[1],) if k == 1 else (A.shape[1], k)) and last_solve_info("lsmr")["fused"]
        assert C.relerr(x, X) <= 1e-9, (C.relerr(x, X), its)             # cond² · atol = 1e-10, a decade of margin
    else:
        x, its = lsmr(As, b)
        xh, ith = _host_loop(As, b)
        print(f"fp32 {layout} k={k}: fused {C.relerr(x, X):.3e} in {its}, host loop {C.relerr(xh, X):.3e} in {ith}")
        assert C.relerr(x, X) <= 4 * C.relerr(xh, X) and abs(its - ith) <= 2


@pytest.mark.parametrize("variant", ["damp", "x0", "callables", "callables_1d", "dense"])
def test_lsmr_argument_forms(variant):
    A, td = C.tall(), torch.float64
    k = 1 if variant == "callables_1d" else 3
    B = C.rhs(A.shape[0], k)
    b = B.to(DEV)[:, 0] if k == 1 else B.to(DEV)
    damp = 0.3 if variant == "damp" else 0.0
    kw = dict(TIGHT, damp=damp)
    if variant == "x0":
        kw["x0"] = C.rhs(A.shape[1], k, seed=3).to(DEV)
    Ad = A.to(DEV)
    if variant.startswith("callables"):
        x, _ = lsmr(lambda v: Ad @ v, b, Armat=lambda w: Ad.t() @ w, n=A.shape[1], **kw)
    else:
        x, _ = lsmr(Ad if variant == "dense" else Ad.to_sparse_csr(), b, **kw)
    assert last_solve_info("lsmr")["fused"] and C.relerr(x, C.dense_lstsq(A, B, damp)) <= 1e-9


def test_columns_are_independent():
    n = 64
    H = torch.tensor([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=torch.float64) / 2
    A = torch.cat([torch.kron(torch.eye(n // 4, dtype=torch.float64), H), torch.zeros((2 * n, n), dtype=torch.float64)])
    assert torch.equal(A.t() @ A, torch.eye(n, dtype=torch.float64))      # orthonormal columns, exactly: beta = 0 after one step
    B = C.rhs(3 * n, 5)
    B[:, 1], B[:, 3] = 0.0, A[:, 7]
    As, b = A.to(DEV).to_sparse_csr(), B.to(DEV)
    x, its = lsmr(As, b, **TIGHT)
    info = last_solve_info("lsmr")
    singles = [lsmr(As, b[:, j], **TIGHT) for j in range(5)]
    xh, ith = _host_loop(As, b, **TIGHT)
    assert info["fused"] and info["iterations"] == its == max(s[1] for s in singles) == ith
    assert list(info["column_iterations"]) == [s[1] for s in singles] and info["column_iterations"][1] == 0
    assert not x[:, 1].any() and torch.allclose(x[:, 3], torch.eye(n, dtype=torch.float64, device=DEV)[7], rtol=0, atol=1e-14)
    for j in range(5):
        assert torch.allclose(x[:, j], singles[j][0], rtol=1e-9, atol=1e-12) and torch.allclose(x[:, j], xh[:, j], rtol=1e-9, atol=1e-12)


def test_a_long_solve_replays_a_graph():
    A = C.tall(dmin=C.DMIN_LONG)                                          # the host-driven loop needs more than 100 iterations
    B = C.rhs(A.shape[0], 2)                                              # (tests/test_lsmr_cpu.py checks that on the CPU)
    As, b = A.to(DEV).to_sparse_csr(), B.to(DEV)
    before = dict(_graph.STATS)
    x, its = lsmr(As, b, **TIGHT)
    assert its > 100 and _graph.STATS["captures"] == before["captures"] + 1 and _graph.STATS["replays"] > before["replays"]
    saved, _graph.MIN_ITERS = _graph.MIN_ITERS, 0
    try:
        xe, ite = lsmr(As, b, **TIGHT)
    finally:
        _graph.MIN_ITERS = saved
    assert ite == its and C.relerr(x, xe.double().cpu()) <= 1e-9 and C.relerr(x, C.dense_lstsq(A, B)) <= 1e-9
