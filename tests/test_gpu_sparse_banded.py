"""sparse_banded_triangular_solve (csrc/band_impl.h) on the GPU against the float64 / long-double substitution of tests/_trsm_ref.py and
its componentwise bound: every mode, template width (3: padded), column tiling (65: a second tile), row counts around the chunk, every
carry level at a small n, gradients in the caller's layout, bit identities, non-finite values and the refusals.

Inputs are rounded to the value type first; a reference is computed once per (width, n, dtype, mode) at the widest p and shared."""

import functools

import numpy as np
import pytest
import torch

import _trsm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH = {"f32": torch.float32, "f64": torch.float64}
WIDTHS = (1, 2, 3, 4, 8)
P_MAX = 65


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def band(w, n):
    return R.chain(n) if w == 1 else R.pattern(n, R.SEED, band=w)


class BandCase(R.Case):
    """R.Case on a band of width w instead of one of R.PATTERNS."""

    def __init__(self, w, n, dtype, mode, p):
        ptr, idx, val = band(w, n)
        base = (ptr, idx, R.round_to(val, dtype))
        self.dtype, self.mode, self.n, self.p = dtype, mode, n, p
        self.unit, self.transpose, self.upper = mode == "lower_unit", mode == "lower_T", mode == "upper"
        self.api = R.to_upper(*base) if self.upper else R.strip_diagonal(*base) if self.unit else base
        self.eff = R.transpose_csr(*self.api) if self.transpose else self.api
        self.lower = mode in ("lower", "lower_unit")
        rng = np.random.default_rng(R.SEED + 1000)
        self.B = R.round_to(rng.standard_normal((n, p)), dtype)
        self.G = R.round_to(rng.standard_normal((n, p)), dtype)
        self._fwd = self._bwd = None
        self.kw = dict(upper=self.upper, unitriangular=self.unit, transpose=self.transpose)


@functools.lru_cache(maxsize=None)
def case(w, n, dtype, mode):
    return BandCase(w, n, dtype, mode, P_MAX)


def dense(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(TORCH[dtype]).to(DEV)          # (exact: rounded already)


def sparse_csr(csr, dtype, itype=torch.int32):
    ptr, idx, val = csr
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(ptr).to(itype).to(DEV), torch.from_numpy(idx).to(itype).to(DEV), dense(val, dtype), (n, n))


def host(x):
    return x.detach().cpu().to(torch.float64).numpy()


def held(x, x64, bnd, dtype, what):
    r, e = R.ratio(host(x), x64, bnd), R.rel_err(host(x), x64)
    print(f"banded {what}: {r:.3f} of the bound, relative error {e:.2e}")
    assert r <= 1.0, (what, r)
    assert e < R.NORMWISE[dtype], (what, e)


def solve():
    from torchsparsegradutils_amd import sparse_banded_triangular_solve

    return sparse_banded_triangular_solve


# ---- 1. forward and gradB: every mode, width and value type ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_forward_and_gradb_within_the_componentwise_bound(dtype, w, mode):
    c = case(w, 1031, dtype, mode)
    A = sparse_csr(c.api, dtype)
    (x64, bnd), (g64, gbnd) = c.forward(), c.backward()
    for p in (1, 5, 8, 65):
        B = dense(c.B[:, :p], dtype).requires_grad_(True)
        X = solve()(A, B, **c.kw)
        assert X.shape == (c.n, p) and X.dtype == TORCH[dtype]
        held(X, x64[:, :p], bnd[:, :p], dtype, (dtype, w, mode, p, "forward"))
        X.backward(dense(c.G[:, :p], dtype))
        held(B.grad, g64[:, :p], gbnd[:, :p], dtype, (dtype, w, mode, p, "gradB"))


# ---- 2. row counts around the chunk, and every carry level ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("w", WIDTHS)
def test_row_counts_and_carry_levels(w, mode):
    from torchsparsegradutils_amd import _backend as be

    p = 5
    for dtype in ("f32", "f64"):
        rows = be.band_geometry(TORCH[dtype], 1031, p, w)[0]
        runs = [(n, None, None) for n in (1, 2, w, w + 1, rows - 1, rows, rows + 1, 2 * rows + 1)]
        runs += [(n, 4, None) for n in (1, 2, w, w + 1, 3, 4, 5, 9)] + [(1031, 4, 4)]
        assert be.band_geometry(TORCH[dtype], 1031, p, w, 4, 4) == (4, 4, 32)          # 258 chunks → 65 → 17: two group levels and the top
        for n, cr, gc in runs:
            c = case(w, n, dtype, mode)
            A = sparse_csr(c.api, dtype)
            X = be.csr_band_sptrsm(A.crow_indices(), A.col_indices(), A.values(), dense(c.B[:, :p], dtype), n, w, lower=not c.upper,
                                   unit=c.unit, transpose=c.transpose, chunk_rows=cr, group_chunks=gc)
            x64, bnd = c.forward()
            held(X, x64[:, :p], bnd[:, :p], dtype, (dtype, w, mode, n, cr, gc))


# ---- 3. gradA in the caller's layout ---------------------------------------------------------------------------------------------------
def dense_grads(D, B, G, upper, transpose):
    """float64 dense autograd of the same solve: (x, gradA dense, gradB)."""
    D, B = D.clone().requires_grad_(True), B.clone().requires_grad_(True)
    M = D.transpose(-1, -2) if transpose else D
    x = torch.linalg.solve_triangular(M, B, upper=upper != transpose)
    gA, gB = torch.autograd.grad(x, (D, B), G)
    return x.detach(), gA, gB


@pytest.mark.parametrize("mode", ("lower", "upper", "lower_T"))
@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_grada_layouts_batches_and_bit_identities(dtype, mode):
    w, n, p, batch = 4, 67, 5, 3
    c = case(w, n, dtype, mode)
    ptr, idx, val = c.api
    vals = np.stack([R.round_to(val * (1.0 + 0.125 * b), dtype) for b in range(batch)])
    Bs = np.stack([R.round_to(np.roll(c.B[:, :p], b, axis=0), dtype) for b in range(batch)])
    G = np.stack([c.G[:, :p]] * batch)
    D64 = torch.stack([torch.from_numpy(R.dense(ptr, idx, v)) for v in vals])
    x64, gA64, gB64 = dense_grads(D64, torch.from_numpy(Bs), torch.from_numpy(G), c.upper, c.transpose)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    out = {}
    for layout in ("csr", "coo"):
        for itype in (torch.int32, torch.int64):
            for batched in (False, True):
                if batched:
                    crow, col = (torch.from_numpy(a).to(itype).to(DEV).repeat(batch, 1) for a in (ptr, idx))
                    A = torch.sparse_csr_tensor(crow, col, dense(vals, dtype), (batch, n, n))
                    B, Gd = dense(Bs, dtype), dense(G, dtype)
                else:
                    A = sparse_csr((ptr, idx, vals[0]), dtype, itype)
                    B, Gd = dense(Bs[0], dtype), dense(G[0], dtype)
                if layout == "coo":
                    if itype == torch.int32:
                        continue          # (COO indices are int64)
                    A = A.to_sparse_coo()
                A, B = A.requires_grad_(True), B.requires_grad_(True)
                X = solve()(A, B, **c.kw)
                gA, gB = torch.autograd.grad(X, (A, B), Gd)
                assert gA.layout == A.layout and gA.shape == A.shape
                gv = (gA.values() if layout == "csr" else gA.coalesce().values()).reshape(batch if batched else 1, -1)
                items = range(batch) if batched else range(1)
                for b in items:
                    xb = R.solve64(*c.eff[:2], R.transpose_csr(ptr, idx, vals[b])[2] if c.transpose else vals[b], Bs[b], c.lower, c.unit)
                    xd, gd = (X[b], gB[b]) if batched else (X, gB)
                    assert R.rel_err(host(xd), xb) < R.NORMWISE[dtype]
                    assert R.rel_err(host(gd), gB64[b].numpy()) < R.NORMWISE[dtype]
                    assert R.rel_err(host(gv[b]), gA64[b].numpy()[rows, idx]) < R.NORMWISE[dtype]
                out[layout, itype, batched] = (X.detach(), gv, gB)
    for batched in (False, True):
        ref = out["csr", torch.int32, batched]
        for key in (("csr", torch.int64, batched), ("coo", torch.int64, batched)):
            assert all(torch.equal(a, b) for a, b in zip(ref, out[key])), key


# ---- 4. determinism and non-finite values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("lower", "upper", "lower_T"))
@pytest.mark.parametrize("w", (1, 4))
def test_two_calls_agree_and_a_missing_diagonal_poisons_its_reach_only(w, mode):
    c = case(w, 257, "f32", mode)
    n, p = c.n, 5
    B = dense(c.B[:, :p], "f32")
    A = sparse_csr(c.api, "f32")
    assert torch.equal(solve()(A, B, **c.kw), solve()(A, B, **c.kw))
    bad = R.strip_diagonal(*c.api, rows=[40])
    eff = R.transpose_csr(*bad) if c.transpose else bad
    with np.errstate(all="ignore"):
        reach = ~np.isfinite(R.solve64(*eff, c.B[:, :p], c.lower, False))          # the substitution itself says which rows depend on row 40
    assert reach[40].all() and 0 < reach.sum() < n * p
    X = solve()(sparse_csr(bad, "f32"), B, **c.kw)
    assert np.array_equal(~np.isfinite(host(X)), reach)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_alone():
    wide = sparse_csr(R.pattern(64, R.SEED, band=9), "f32")
    B = dense(np.ones((64, 2)), "f32")
    with pytest.raises(ValueError, match=r"9 wide.*8.*sparse_triangular_solve"):
        solve()(wide, B, upper=False)
    crow, col = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV), torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="strictly ascending"):
        solve()(torch.sparse_csr_tensor(crow, col, torch.ones(3, device=DEV), (2, 2)), B[:2], upper=False)
    c = case(2, 65, "f32", "lower")
    x64, bnd = c.forward()
    held(solve()(sparse_csr(c.api, "f32"), dense(c.B[:, :2], "f32"), **c.kw), x64[:, :2], bnd[:, :2], "f32", "after the refusals")
