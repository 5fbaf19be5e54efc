"""The quadrature kernel and the Rademacher fill (csrc/quadrature.hip), one launch at a time through `_backend`, against the float64
mirror (tests/_quadrature_ref.py: the header's T, the length rule, numpy.linalg.eigh).

The bound is QL's backward error pushed through f on the spectrum:

    |out - ref| <= 64 · r · 2⁻⁵³ · (‖T‖_∞ / λ_min + max_j |f(λ_j)|)     (times |scale|)

— the computed (λ_j, τ_j) are exact for a T + E with ‖E‖ <= c·r·ε·‖T‖; a node moves by at most ‖E‖, f' on the spectrum is at most
1/λ_min for log (and 1/λ_min² · λ_min for the relative change of 1/λ), and the weights change the sum by a multiple of max|f|.  The
constant 64 is the margin.  The mirror rounds fp32 inputs as the kernel reads them (both start from the same float32 array).  The
kernel's arithmetic is float64 but `out` is in the value type: for fp32 the one final rounding of the result, |ref|·2⁻²⁴, is added
to the bound (the float64 bound alone is below half an fp32 ulp of the result, which no fp32 output can meet).

kind 1: random Jacobi matrices with a prescribed spectrum in [1, 1e3]; r in {1, 2, 3, 31, 64, cap} (cap and every r above 100 take
the `work` form, the others LDS), p in {1, 3, 64, 65, 256} (a partial wave, one wave, one lane of a second workgroup, four).
kind 0: the true fp32 CG histories of the three test matrices at 64 steps (clustered ghost eigenvalues), and one launch of mixed
lengths.  Invariants that need no mirror: fn = 3 gives 1, fn = 2 gives T[0][0], a negative eigenvalue gives info < 0 and NaN for
fn 0 / 1 and finite values for fn 2 / 3.
"""

import numpy as np
import pytest
import torch

import _quadrature_ref as QR
from torchsparsegradutils_amd import _backend, _cpu

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
NP = {torch.float32: np.float32, torch.float64: np.float64}


def _cap():
    return _backend.quadrature_geometry()[0]


@pytest.fixture(scope="module")
def jacobi_bank():
    """(d, e) of 8 Jacobi matrices per size: the columns of a launch cycle through them."""
    rng = np.random.default_rng(11)
    bank = {}
    for r in (1, 2, 3, 31, 64, _cap()):
        bank[r] = [QR.jacobi(np.exp(rng.uniform(0.0, np.log(1e3), r)), rng) for _ in range(8)]
    return bank


def _entries(bank, r, p):
    coef = np.zeros((r, 2, p))
    for c in range(p):
        d, e = bank[r][c % len(bank[r])]
        coef[:, 0, c] = d * (1.0 + 0.01 * (c // len(bank[r])))          # (later cycles: shifted copies, still positive definite)
        coef[: r - 1, 1, c] = e
        coef[r - 1, 1, c] = 3.0                                          # the last off-diagonal is ignored
    return coef


def _launch(coef_np, td, kind, fn, scale_np=None):
    coef = torch.from_numpy(np.ascontiguousarray(coef_np)).to(td).to(DEV)
    scale = None if scale_np is None else torch.from_numpy(scale_np).to(td).to(DEV)
    out, info = _backend.tridiag_quadrature(coef, kind, fn, scale=scale)
    assert out.dtype == td and info.dtype == torch.int32
    return out.cpu().double().numpy(), info.cpu().numpy(), coef.cpu().double().numpy()


def _check(got, info, coef64, td, kind, fn, scale_np=None):
    """Against the mirror on the rounded inputs; fp32 outputs carry their own final rounding."""
    scale64 = None if scale_np is None else scale_np.astype(NP[td]).astype(np.float64)
    want, winfo, bound = QR.quadrature(coef64, kind, fn, scale64)
    assert np.array_equal(info, winfo)
    ok = ~np.isnan(want)
    assert np.all(np.isnan(got[~ok]))
    slack = np.abs(want[ok]) * 2.0 ** -24 if td == torch.float32 else 0.0
    err = np.abs(got[ok] - want[ok])
    ratio = float((err / np.maximum(bound[ok] + slack, 1e-300)).max()) if ok.any() else 0.0
    print(f"{td} kind {kind} fn {fn} r {coef64.shape[0]} p {coef64.shape[2]}: max |out - ref| / bound = {ratio:.3e}")
    assert np.all(err <= bound[ok] + slack)
    return want, winfo


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("r", [1, 2, 3, 31, 64, "cap"])
def test_entries_against_the_mirror(jacobi_bank, r, td):
    r = _cap() if r == "cap" else r
    for p in (1, 3, 64, 65, 256):
        coef = _entries(jacobi_bank, r, p)
        scale = np.linspace(0.5, 3.0, p)
        for fn in range(4):
            got, info, c64 = _launch(coef, td, _backend.QUAD_ENTRIES, fn, scale if fn == 0 else None)
            _check(got, info, c64, td, _backend.QUAD_ENTRIES, fn, scale if fn == 0 else None)
            assert np.all(info == r)
            if fn == _backend.QUAD_ONE:
                assert np.allclose(got, 1.0, rtol=0, atol=64 * r * QR.U + (2.0 ** -24 if td == torch.float32 else 0))
            if fn == _backend.QUAD_IDENTITY:
                assert np.allclose(got, c64[0, 0], rtol=64 * r * QR.U * 1e3 + (2.0 ** -23 if td == torch.float32 else 0), atol=0)


@pytest.fixture(scope="module")
def histories():
    return {name: QR.cg_history(make(), np.eye(make().shape[0]), 64, np.float32) for name, make in QR.MATRICES.items()}


@pytest.mark.parametrize("name", list(QR.MATRICES))
def test_cg_histories_against_the_mirror(histories, name):
    hist = histories[name]
    exact = float(np.linalg.slogdet(QR.MATRICES[name]())[1])
    for td in DTYPES:                # (fp64: the same numbers in the wider container)
        for fn in range(4):
            got, info, c64 = _launch(hist, td, _backend.QUAD_CG, fn)
            want, winfo = _check(got, info, c64, td, _backend.QUAD_CG, fn)
            assert winfo.min() >= 1 and winfo.max() <= 64
            if fn == _backend.QUAD_LOG and td == torch.float64:
                print(f"{name}: lengths {winfo.min()}..{winfo.max()}, |Σ out - slogdet| = {abs(got.sum() - exact):.3e}")
                assert abs(got.sum() - exact) <= 2e-5 * abs(exact)
    # the repeat of a launch gives the same bits
    a = _launch(hist, torch.float32, 0, 0)[0]
    assert np.array_equal(a, _launch(hist, torch.float32, 0, 0)[0])


def test_mixed_lengths_in_one_launch(histories):
    hist = histories["lap7x9"].copy()                    # 63 columns, 64 rows
    hist[:, :, 5] = 0.0                                  # an all-zero column: r_c = 0
    for c, row in ((8, 1), (9, 7), (10, 20), (40, 3)):   # alpha turns 0 at different rows
        hist[row:, :, c] = 0.0
    hist[11, 1, 12] = 0.0                                # a beta = 0 in the middle: only the leading block counts
    hist[5, 0, 13] = np.inf                              # alpha not finite
    hist[6, 0, 14] = -1.0                                # alpha not positive
    hist[9, 1, 15] = np.nan                              # beta not finite: ends after its row
    hist[10, 1, 16] *= 1e-18                             # an off-diagonal 1e-9 times its neighbours (beta is its square)
    for td in DTYPES:
        for fn in range(4):
            got, info, c64 = _launch(hist, td, _backend.QUAD_CG, fn)
            want, winfo = _check(got, info, c64, td, _backend.QUAD_CG, fn)
            assert [int(winfo[c]) for c in (5, 8, 9, 10, 40, 12, 13, 14, 15)] == [0, 1, 7, 20, 3, 12, 5, 6, 10]
            assert got[5] == 0.0
    # the same through the leading columns of a wider array, and against the torch-op path
    out, info = _backend.tridiag_quadrature(torch.from_numpy(hist).to(DEV), 0, 0, p=20)
    ref, rinfo = _cpu.tridiag_quadrature(torch.from_numpy(hist), 0, 0, p=20)
    assert torch.equal(info.cpu(), rinfo) and out.shape == (20,)
    assert np.all(np.abs(out.cpu().numpy() - ref.numpy()) <= 2.0 ** -22 * (1 + np.abs(ref.numpy())))


@pytest.mark.parametrize("td", DTYPES)
def test_a_negative_eigenvalue_is_reported(jacobi_bank, td):
    r, p = 31, 65
    coef = _entries(jacobi_bank, r, p)
    bad = [0, 7, 64]
    coef[:, 0, bad] -= 40.0                              # spectrum in [1, 1e3] shifted down: some eigenvalues turn negative
    for fn in range(4):
        got, info, c64 = _launch(coef, td, _backend.QUAD_ENTRIES, fn)
        lam_min = [np.linalg.eigvalsh(QR.dense_t(c64[:, 0, c], c64[: r - 1, 1, c])).min() for c in bad]
        assert max(lam_min) < 0
        good = np.setdiff1d(np.arange(p), bad)
        assert np.all(info[good] == r) and np.all(np.isfinite(got[good]))
        if fn <= _backend.QUAD_RECIPROCAL:
            assert np.all(info[bad] == -r) and np.all(np.isnan(got[bad]))
        else:
            assert np.all(info[bad] == r) and np.all(np.isfinite(got[bad]))
            if fn == _backend.QUAD_ONE:
                assert np.allclose(got[bad], 1.0, atol=1e-6)
            else:
                assert np.allclose(got[bad], c64[0, 0, bad], rtol=1e-6)


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("shape", [(1, 1), (1000, 3), (4099, 65)])
def test_rademacher_fill_equals_the_cpu_function(shape, td):
    n, p = shape
    for seed in (0, 7, -3, (1 << 40) + 1):
        got = _backend.rademacher_fill(n, p, seed, td, DEV)
        assert got.dtype == td and got.shape == (n, p) and got.is_cuda
        assert torch.equal(got.cpu(), _cpu.rademacher_fill(n, p, seed, td)), (shape, seed)
        assert np.array_equal(got.cpu().double().numpy(), QR.rademacher(seed, n, p))
