"""The geometry of the sync-free triangular solve (csrc/sptrsm.hip), walked on the GPU: every column-lane width CL = 1 … 64 and the
multi-tile path against a float64 substitution and its componentwise bound (tests/_trsm_ref.py), row counts on both sides of the
class rule, the bit identities that follow from "each row sums its own entries in an order fixed by CL alone", every accepted stride
of B and X, the limits of the tile rule, non-finite values, and the width tuner of sparse_solve.py.

Inputs are generated on the CPU, rounded to the value type under test, and the reference is computed on the rounded inputs, once per
(dtype, mode) at the widest p: columns of a solve are independent, narrower solves are held against prefixes.
tests/test_trsm_ref_cpu.py shows, without a GPU, that an emulated kernel of each precision meets the same bound on the same inputs."""

import functools
import sys

import numpy as np
import pytest
import torch

import _trsm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}
TAG = {"f32": 0x7FC5A5A5, "bf16": 0x7FC5}          # the kernel's "not ready" pattern (Sentinel<V>::kTag, csrc/sptrsm_common.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def be():
    from torchsparsegradutils_amd import _backend

    return _backend


@functools.lru_cache(maxsize=None)
def case(kind, n, dtype, mode, p):
    return R.Case(kind, n, dtype, mode, p)


def dense(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(TORCH[dtype]).to(DEV)          # (exact: rounded already)


def arrays(csr, dtype, itype=torch.int32):
    ptr, idx, val = csr
    return torch.from_numpy(ptr).to(itype).to(DEV), torch.from_numpy(idx).to(itype).to(DEV), dense(val, dtype)


def sparse_csr(csr, dtype, itype=torch.int32):
    ptr, idx, val = arrays(csr, dtype, itype)
    n = ptr.numel() - 1
    return torch.sparse_csr_tensor(ptr, idx, val, (n, n))


def host(x):
    return x.detach().cpu().to(torch.float64).numpy()


def bits(x):
    return x.contiguous().view(BITS[x.dtype])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sweep(csr_dev, B, lower, unit=False, wg_per_cu=1):
    ptr, idx, val = csr_dev
    return be().csr_sptrsm(ptr, idx, val, B, ptr.numel() - 1, lower=lower, unit=unit, wg_per_cu=wg_per_cu)


def held(x, x64, bnd, dtype, what):
    """Every element within the bound, and the project's normwise bar; returns the worst ratio."""
    r = R.ratio(host(x), x64, bnd)
    assert r <= 1.0, (what, r)
    if dtype in R.NORMWISE:
        assert R.rel_err(host(x), x64) < R.NORMWISE[dtype], what
    return r


# ---- a. every width --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_width_within_the_componentwise_bound(dtype, mode):
    # sptrsm.hip `cl = p >= 64 ? 64 : next_pow2(p)`, `dispatch_pow2<1, 64>`, `entry_sum<A, EP>`: CL 1 … 64, EP 64 … 1, 1 … 4 tiles
    from torchsparsegradutils_amd import sparse_triangular_solve

    c = case("pattern", R.N_WIDTHS, dtype, mode, max(R.WIDTHS))
    A = sparse_csr(c.api, dtype)
    B, G = dense(c.B, dtype), dense(c.G, dtype)
    x64, bnd = c.forward()
    kw = dict(upper=c.upper, unitriangular=c.unit, transpose=c.transpose)
    worst = 0.0
    for p in R.WIDTHS:
        X = sparse_triangular_solve(A, B[:, :p].contiguous(), **kw)
        assert X.shape == (c.n, p) and X.dtype == TORCH[dtype]
        worst = max(worst, held(X, x64[:, :p], bnd[:, :p], dtype, ("forward", p)))
    print(f"sptrsm geometry {dtype} {mode}: forward worst {worst:.3f} of the bound")
    if dtype == "f32" or mode == "lower_T":
        # the backward solve is the sweep with the other transpose flag (sparse_solve.py SparseTriangularSolve.backward)
        g64, gbnd = c.backward()
        worst = 0.0
        for p in R.BACKWARD_WIDTHS:
            Bp = B[:, :p].clone().requires_grad_(True)
            X = sparse_triangular_solve(A, Bp, **kw)
            (gB,) = torch.autograd.grad(X, Bp, G[:, :p].contiguous())
            worst = max(worst, held(gB, g64[:, :p], gbnd[:, :p], dtype, ("backward", p)))
        print(f"sptrsm geometry {dtype} {mode}: backward worst {worst:.3f} of the bound")


# ---- b. row counts around the class rule -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.ROW_COUNTS)
def test_row_counts_around_the_class_rule(n):
    # sptrsm.hip `Q.wgc = min(blocks, 64)`, `cls = wg * kTrsmWaves + slot`; sptrsm_common.h `persistent_blocks`: fewer rows than
    # waves (n < 4), one workgroup, wgc below / at / above 64 (n = 255, 256, 257)
    for kind in R.PATTERNS:
        if kind == "arrow" and n not in R.ARROW_ROWS:
            continue
        for mode in ("lower", "upper"):
            c = case(kind, n, "f32", mode, max(R.ROW_WIDTHS))
            csr = arrays(c.api, "f32")
            B = dense(c.B, "f32")
            x64, bnd = c.forward()
            for p in R.ROW_WIDTHS:
                X = sweep(csr, B[:, :p].contiguous(), lower=c.lower)
                held(X, x64[:, :p], bnd[:, :p], "f32", (kind, mode, n, p))


# ---- c. bit identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_workgroups_per_cu_do_not_change_a_bit(dtype):
    # sptrsm.hip "the result does not depend on it": `persistent_blocks(n_cu, wg_per_cu, n)` only deals the rows to other waves
    for mode in ("lower", "upper"):
        c = case("pattern", R.N_WIDTHS, dtype, mode, max(R.WIDTHS))
        csr = arrays(c.api, dtype)
        B = dense(c.B, dtype)
        for p in (1, 8, 65):
            Bp = B[:, :p].contiguous()
            X1 = sweep(csr, Bp, lower=c.lower, wg_per_cu=1)
            for w in (2, 4, 8):
                assert same_bits(sweep(csr, Bp, lower=c.lower, wg_per_cu=w), X1), (mode, p, w)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_same_column_lanes_same_bits(dtype):
    # sptrsm.hip `k = base + ep`, `c = tile * CL + cl`: a row's summation order is fixed by CL, a column's tile by c / CL alone
    c = case("pattern", R.N_WIDTHS, dtype, "lower", max(R.WIDTHS))
    csr = arrays(c.api, dtype)
    B = dense(c.B, dtype)
    X = {p: sweep(csr, B[:, :p].contiguous(), lower=True) for p in (3, 4, 5, 8, 64, 65, 128, 200)}
    assert same_bits(X[8][:, :5], X[5])            # CL = 8, dead column lanes
    assert same_bits(X[4][:, :3], X[3])            # CL = 4
    for p in (65, 128, 200):
        assert same_bits(X[p][:, :64], X[64]), p          # tile 0 of several (wgc = 1, counters per tile) against the single-tile grid
    assert same_bits(X[200][:, 64:128], sweep(csr, B[:, 64:128].contiguous(), lower=True))          # tile 1: `tile * CL + cl`
    assert same_bits(X[200][:, 128:192], sweep(csr, B[:, 128:192].contiguous(), lower=True))        # tile 2


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_index_width_and_layout_do_not_change_a_bit(dtype):
    # sptrsm.hip `template <typename V, typename I, …>`: both index instantiations; sparse_solve.py _TriOperand: COO and CSR operands
    from torchsparsegradutils_amd import sparse_triangular_solve

    for mode in ("lower", "lower_T"):
        c = case("pattern", R.N_WIDTHS, dtype, mode, max(R.WIDTHS))
        B = dense(c.B[:, :9], dtype)
        kw = dict(upper=c.upper, unitriangular=c.unit, transpose=c.transpose)
        X32 = sparse_triangular_solve(sparse_csr(c.api, dtype, torch.int32), B, **kw)
        X64 = sparse_triangular_solve(sparse_csr(c.api, dtype, torch.int64), B, **kw)
        ptr, idx, val = arrays(c.api, dtype, torch.int64)
        rows = torch.repeat_interleave(torch.arange(c.n, device=DEV), ptr[1:] - ptr[:-1])
        coo = torch.sparse_coo_tensor(torch.stack([rows, idx]), val, (c.n, c.n), is_coalesced=True)          # (CSR order is coalesced order)
        Xcoo = sparse_triangular_solve(coo, B, **kw)
        assert same_bits(X64, X32) and same_bits(Xcoo, X32), mode
    c = case("pattern", R.N_WIDTHS, dtype, "upper", max(R.WIDTHS))
    B = dense(c.B[:, :65], dtype)
    assert same_bits(sweep(arrays(c.api, dtype, torch.int64), B, lower=False), sweep(arrays(c.api, dtype, torch.int32), B, lower=False))


# ---- d. strides ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_strided_right_hand_sides_solve_to_the_same_bits(dtype):
    # sptrsm.hip `B[row * P.ldb + c * P.bcs]`; _backend.strided2d: transposed views and row-major windows are read in place
    c = case("pattern", 257, dtype, "lower", 65)
    csr = arrays(c.api, dtype)
    n = c.n
    filler = dense(c.G, dtype)
    for p in (1, 5, 65):
        Bc = dense(c.B[:, :p], dtype)
        want = sweep(csr, Bc, lower=True)
        held(want, c.forward()[0][:, :p], c.forward()[1][:, :p], dtype, ("contiguous", p))

        W = Bc.t().contiguous()                                   # (p, n): B = W.t(), unit row stride, column stride n
        Bt = W.t()
        assert p == 1 or Bt.stride() == (1, n)
        assert same_bits(sweep(csr, Bt, lower=True), want), ("transposed view", p)

        W = torch.cat([filler[:, :3], Bc, filler[:, :4]], 1).contiguous()          # a window of a wider matrix: ldb = p + 7
        Bw = W[:, 3:3 + p]
        assert Bw.stride(0) == p + 7 and Bw.data_ptr() != W.data_ptr()
        assert same_bits(sweep(csr, Bw, lower=True), want), ("window", p)

        W = torch.stack([Bc, filler[:, :p]], 1).reshape(2 * n, p).contiguous()     # every other row: ldb = 2p
        Be = W[::2]
        assert Be.stride(0) == 2 * p and torch.equal(Be, Bc)
        assert same_bits(sweep(csr, Be, lower=True), want), ("row stride 2p", p)

        W = torch.stack([Bc, filler[:, :p]], 2).reshape(n, 2 * p).contiguous()     # every other column: strided2d has to copy
        Bo = W[:, ::2]
        assert torch.equal(Bo, Bc) and be().strided2d(Bo)[0].data_ptr() != Bo.data_ptr()
        assert same_bits(sweep(csr, Bo, lower=True), want), ("copied", p)

        if p > 1:
            W = torch.cat([Bc.t(), filler[:6, :p].t()], 1).contiguous()            # transposed view of a window: column stride n + 6
            Bv = W[:, :n].t()
            assert Bv.stride() == (1, n + 6)
            assert same_bits(sweep(csr, Bv, lower=True), want), ("transposed window", p)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_solution_window_through_the_c_abi_leaves_its_guard_columns_alone(dtype):
    # sptrsm.hip `X + row * P.ldx + c` and sptrsm_common.h sptrsm_fill_kernel `x + r * ldx + c`: ldx > p, 4- and 2-byte stores
    b = be()
    lib = b.load_library()
    c = case("pattern", 257, dtype, "lower", 65)
    ptr, idx, val = arrays(c.api, dtype)
    n, dev = c.n, torch.device(DEV)
    for p in (5, 65):
        Bc = dense(c.B[:, :p], dtype)
        want = sweep((ptr, idx, val), Bc, lower=True)
        wide = torch.full((n, p + 7), 3.0, dtype=TORCH[dtype], device=DEV)
        Xw = wide[:, 3:3 + p]
        work = torch.empty((lib.tsgu_sptrsm_work_bytes(n, p),), dtype=torch.uint8, device=DEV)
        b.launch("tsgu_csr_sptrsm", dev, b.vtype_of(val), b.itype_of(ptr), n, idx.numel(), ptr, idx, None, val, 1, 0, Bc, p, 1,
                 Xw, p + 7, p, work, 1)
        torch.cuda.synchronize()
        assert int(work[512:516].view(torch.int32).item()) == 0          # (the error word: no wait ran out)
        assert same_bits(Xw, want), p
        assert bool((wide[:, :3] == 3.0).all()) and bool((wide[:, 3 + p:] == 3.0).all()), p


# ---- e. limits of the tile rule --------------------------------------------------------------------------------------------------
def test_last_allowed_width_and_the_first_refused():
    # sptrsm.hip `if (tiles > 64) return TSGU_ERR_TOO_LARGE`, `blocks = blocks / tiles; if (blocks < 1) blocks = 1`,
    # `class_ticket[(slot * 64 + tile) * 16]` up to tile 63
    c = case("pattern", 65, "f32", "lower", 4096)
    csr = arrays(c.api, "f32")
    B = dense(c.B, "f32")
    x64, bnd = c.forward()
    X = sweep(csr, B, lower=True)
    held(X, x64, bnd, "f32", 4096)
    assert same_bits(X[:, :64], sweep(csr, B[:, :64].contiguous(), lower=True))
    assert same_bits(X[:, 4032:], sweep(csr, B[:, 4032:].contiguous(), lower=True))          # the last tile
    with pytest.raises(RuntimeError, match="tsgu_csr_sptrsm"):
        sweep(csr, torch.cat([B, B[:, :1]], 1), lower=True)
    assert same_bits(sweep(csr, B[:, :64].contiguous(), lower=True), X[:, :64])          # (and the next solve is served as ever)


# ---- f. non-finite values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_non_finite_values_travel_along_the_dependencies_and_nowhere_else(dtype):
    # sptrsm.hip `if (x != x) xb = S::kCanon`: a NaN — the tag's own bits included — is published as a value that reads as ready;
    # `dsum = entry_sum(diag)` of a row without a stored diagonal is 0: inf / NaN, not a wait
    n, p = 257, 8
    c = case("pattern", n, dtype, "lower", 65)
    ptr, idx, val = c.api
    seeds = [(20, 1), (60, 3), (100, 6)]
    no_diag = 200
    holed = R.strip_diagonal(ptr, idx, val, rows=[no_diag])
    assert holed[0][-1] == ptr[-1] - 1 and (val != 0).all()
    reach = np.zeros((n, p), dtype=bool)
    for r, col in seeds:
        reach[r, col] = True
    reach[no_diag, :] = True
    for i in range(n):
        deps = idx[ptr[i]:ptr[i + 1]]
        reach[i] |= reach[deps[deps < i]].any(0)
    assert reach.sum() > 100 and (~reach).sum() > 500 and (~reach[no_diag + 1:]).any()          # both sets are worth comparing

    Bc = dense(c.B[:, :p], dtype)
    clean = sweep(arrays(c.api, dtype), Bc, lower=True)
    assert bool(torch.isfinite(clean).all())
    Bn = Bc.clone()
    Bn[20, 1] = float("nan")
    Bn[60, 3] = float("inf")
    bits(Bn)[100, 6] = TAG[dtype]
    assert bool(torch.isnan(Bn[100, 6])) and int(bits(Bn)[100, 6]) == TAG[dtype]
    X = sweep(arrays(holed, dtype), Bn, lower=True)          # (returns: no dependency wait runs out)
    where = torch.from_numpy(reach).to(DEV)
    assert torch.equal(~torch.isfinite(X), where)
    assert torch.equal(bits(X)[~where], bits(clean)[~where])
    assert not bool((bits(X) == TAG[dtype]).any())
    assert bool(torch.isinf(X[60, 3])) and bool(torch.isnan(X[20, 1])) and bool(torch.isnan(X[100, 6]))


# ---- g. the width tuner ----------------------------------------------------------------------------------------------------------
def test_width_tuner_measures_once_and_changes_no_bit(monkeypatch):
    # sparse_solve.py `_sweep_width`: trial solves at a pattern's third solve, then the memo; width 1 in deterministic mode
    import torchsparsegradutils_amd  # noqa: F401
    from torchsparsegradutils_amd import _pattern, sparse_triangular_solve

    ss = sys.modules["torchsparsegradutils_amd.sparse_solve"]
    b = be()
    n, p = 4096, 8
    csr = R.shallow(n)
    csr = (csr[0], csr[1], R.round_to(csr[2], "f32"))
    B = dense(R.round_to(np.random.default_rng(3).standard_normal((n, p)), "f32"), "f32")
    monkeypatch.setattr(ss, "SWEEP_TUNE", True)
    calls = []
    real = b.csr_sptrsm

    def counted(*a, **k):
        calls.append(k.get("wg_per_cu"))
        return real(*a, **k)

    monkeypatch.setattr(b, "csr_sptrsm", counted)
    _pattern.wait_for_plans()          # (a trial beside a plan build is put off to the next solve)
    A = sparse_csr(csr, "f32")
    key = (True, False, torch.float32, p)
    X, per_solve = [], []
    for _ in range(4):
        calls.clear()
        X.append(sparse_triangular_solve(A, B, upper=False))
        per_solve.append(list(calls))
    memo = _pattern.from_csr(A).core.own["sweep_width"]
    assert isinstance(memo[key], int) and memo[key] in ss.SWEEP_WIDTHS
    assert per_solve[0] == [1] and per_solve[1] == [1]
    assert len(per_solve[2]) > 1 and set(per_solve[2][:-1]) == set(ss.SWEEP_WIDTHS) and per_solve[2][-1] == memo[key]
    assert per_solve[3] == [memo[key]]          # exactly one launch, at the remembered width
    for x in X[1:]:
        assert same_bits(x, X[0])
    x64 = R.solve64(*csr, host(B), True, False)
    held(X[0], x64, R.bound(*csr, x64, True, False, R.U["f32"]), "f32", "shallow")

    _pattern.clear_cache()
    A2 = sparse_csr(csr, "f32")
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(4):
            calls.clear()
            assert same_bits(sparse_triangular_solve(A2, B, upper=False), X[0])
            assert calls == [1]
    finally:
        torch.use_deterministic_algorithms(was)
    assert "sweep_width" not in _pattern.from_csr(A2).core.own          # nothing was measured, nothing is remembered
