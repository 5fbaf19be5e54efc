"""`sparse_inv_sqrt_mm` / `sparse_sqrt_mm` on the GPU, end to end, against dense float64 (`eigh` for the values and `grad_B`, the
gradient formula with dense solves for `grad_A`) and against the package's CPU path.

Bound (fp64, tolerance 1e-12, N = 12).  The result is r(A) B with every shifted solve stopped at a residual of at most `tolerance`
relative to the column: the rule contributes its own error on the exact spectrum, e_rule = max_j |r(λ_j) √λ_j − 1| (computed here),
and the solves Σ_q ω_q tolerance / (λ_min + σ_q) ≈ tolerance / √λ_min per unit of ‖b‖, that is tolerance·√κ relative to
‖A^{-1/2} b‖ ≥ ‖b‖ / √λ_max.  The test allows 10·(e_rule + tolerance·√κ), in the 2-norm per column (Frobenius for the values of
`grad_A`, whose two factors each carry the solver's error).

fp32 (tolerance 1e-5) has no derived margin: the error of the package's CPU torch-op path in fp32 on the same inputs against the
float64 dense result is measured in the test, and the GPU's error may be at most 4 times that (two correct fp32 runs with different
summation orders).  Both are printed; DESIGN.md §6 has the figures of one run.

History of that check: with the stop kernel on every iteration the fused loop froze a column at the iteration MINRES's residual
estimate reached the tolerance (17 and 14 iterations on the 6 × 7 and 4 × 5 × 3 lattices: forward errors 2.40e-6 and 2.73e-6), while
the unfused `minres` of the CPU path tests every 10 iterations, ran to 20 and reached the fp32 floor (1.42e-7, 8.34e-8): ratios of
17 and 33, and the check failed on those two matrices (it held on 12 × 11 × 10, where both stopped after 30: 3.84e-6 / 3.83e-6).
The stop kernel now runs every 10th iteration, just before the host reads the stop word, and the check holds on all three.
"""

import numpy as np
import pytest
import torch

import _ciq_ref as CR
from torchsparsegradutils_amd import sparse_inv_sqrt_mm, sparse_sqrt_mm
from torchsparsegradutils_amd.sparse_sqrt import _ciq_rule
from torchsparsegradutils_amd.utils._operator import LAST_SOLVE

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = torch.float64
NAMES = list(CR.MATRICES) + list(CR.LARGE)
N_QUAD = 12


def _sparse(M, layout, dtype, device):
    crow, col, val = CR.csr_arrays(M)
    n = M.shape[0]
    if layout == "csr":
        S = torch.sparse_csr_tensor(torch.from_numpy(crow).to(torch.int32), torch.from_numpy(col).to(torch.int32),
                                    torch.from_numpy(val).to(dtype), (n, n))
    else:
        rows = np.repeat(np.arange(n), np.diff(crow))
        S = torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, col))), torch.from_numpy(val).to(dtype), (n, n)).coalesce()
    return S.to(device)


@pytest.fixture(scope="module")
def cases():
    """name -> dict of the float64 truth, computed once and never written to."""
    rng = np.random.default_rng(21)
    out = {}
    for name, make in {**CR.MATRICES, **CR.LARGE}.items():
        M = make()
        n = M.shape[0]
        inv_sqrt, lam = CR.dense_power(M, -0.5)
        sqrt, _ = CR.dense_power(M, 0.5)
        B, G = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
        bounds = (float(lam[0]), float(lam[-1]))
        sigma, omega = _ciq_rule(*bounds, N_QUAD)
        crow, col, _ = CR.csr_arrays(M)
        rows = np.repeat(np.arange(n), np.diff(crow))
        out[name] = dict(M=M, lam=lam, bounds=bounds, B=B, G=G, fwd=inv_sqrt @ B, sqrt=sqrt @ B, gB=inv_sqrt @ G,
                         gA=CR.grad_a_dense(M, B, G, sigma, omega)[rows, col], kappa=float(lam[-1] / lam[0]),
                         e_rule=CR.scalar_error(sigma, omega, lam))
    return out


def _col_err(got, want):
    got = got.detach().cpu().double().numpy()
    return float((np.linalg.norm(got - want, axis=0) / np.linalg.norm(want, axis=0)).max())


def _run(case, layout, dtype, device, tolerance, **kw):
    S = _sparse(case["M"], layout, dtype, device).requires_grad_(True)
    B = torch.from_numpy(case["B"]).to(dtype).to(device).requires_grad_(True)
    out, info = sparse_inv_sqrt_mm(S, B, bounds=case["bounds"], tolerance=tolerance, num_quad=N_QUAD, return_info=True, **kw)
    out.backward(torch.from_numpy(case["G"]).to(dtype).to(device))
    gA = S.grad.values() if layout == "csr" else S.grad._values()
    return out, B.grad, gA, info


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_fp64_against_dense_and_the_cpu_path(cases, name, layout):
    c = cases[name]
    tol = 1e-12
    bound = 10.0 * (c["e_rule"] + tol * np.sqrt(c["kappa"]))
    out, gB, gA, info = _run(c, layout, F64, DEV, tol)
    assert info["fused"] is True and info["converged"] is True and info["iterations"] <= c["M"].shape[0] + 1
    assert info["residual_estimates"].shape == (3,) and float(info["residual_estimates"].max()) <= tol
    assert LAST_SOLVE.info["sparse_inv_sqrt_mm"]["fused"] is True
    errs = {"forward": _col_err(out, c["fwd"]), "grad_B": _col_err(gB, c["gB"]),
            "grad_A": float(np.linalg.norm(gA.cpu().numpy() - c["gA"]) / np.linalg.norm(c["gA"]))}
    cpu_out, cpu_gB, cpu_gA, cpu_info = _run(c, layout, F64, "cpu", tol)
    assert cpu_info["fused"] is False
    errs["forward vs cpu"] = _col_err(out, cpu_out.detach().numpy())
    errs["grad_B vs cpu"] = _col_err(gB, cpu_gB.numpy())
    errs["grad_A vs cpu"] = float(np.linalg.norm(gA.cpu().numpy() - cpu_gA.numpy()) / np.linalg.norm(cpu_gA.numpy()))
    print(f"{name} {layout}: iterations {info['iterations']}, e_rule {c['e_rule']:.2e}, kappa {c['kappa']:.1f}, bound {bound:.2e}: "
          + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bound, (k, v, bound)
    S = _sparse(c["M"], layout, F64, DEV)
    Bd = torch.from_numpy(c["B"]).to(DEV)
    sq = sparse_sqrt_mm(S, Bd, bounds=c["bounds"], tolerance=tol, num_quad=N_QUAD)
    # A·(r(A) b): the rule's part is A^{1/2}(r(A) A^{1/2} − I) b, e_rule relative; a residual of norm tolerance·‖b‖ in shift q adds
    # ω_q A (A + σ_q)⁻¹ of it, and Σ_q ω_q λ / (λ + σ_q) = λ r(λ) ≈ √λ ≤ √λ_max, against ‖A^{1/2} b‖ ≥ √λ_min ‖b‖: the same bound
    assert _col_err(sq, c["sqrt"]) <= bound
    vec = sparse_inv_sqrt_mm(S, Bd[:, 0].contiguous(), bounds=c["bounds"], tolerance=tol, num_quad=N_QUAD)
    assert vec.shape == (c["M"].shape[0],) and _col_err(vec.unsqueeze(1), c["fwd"][:, :1]) <= bound


@pytest.mark.parametrize("name", NAMES)
def test_fp32_against_the_cpu_paths_own_error(cases, name):
    c = cases[name]
    tol = 1e-5
    out, gB, gA, info = _run(c, "csr", torch.float32, DEV, tol)
    cpu_out, cpu_gB, cpu_gA, _ = _run(c, "csr", torch.float32, "cpu", tol)
    assert info["fused"] is True and info["converged"] is True
    pairs = {
        "forward": (_col_err(out, c["fwd"]), _col_err(cpu_out, c["fwd"])),
        "grad_B": (_col_err(gB, c["gB"]), _col_err(cpu_gB, c["gB"])),
        "grad_A": (float(np.linalg.norm(gA.cpu().double().numpy() - c["gA"]) / np.linalg.norm(c["gA"])),
                   float(np.linalg.norm(cpu_gA.double().numpy() - c["gA"]) / np.linalg.norm(c["gA"]))),
    }
    print(f"{name} fp32 (iterations {info['iterations']}): " + ", ".join(f"{k} gpu {g:.2e} cpu {h:.2e}" for k, (g, h) in pairs.items()))
    for k, (g, h) in pairs.items():
        assert g <= 4.0 * h, (k, g, h)


def test_a_column_does_not_depend_on_its_neighbours(cases):
    c = cases["lap12x11x10"]
    tol = 1e-12
    bound = 10.0 * (c["e_rule"] + tol * np.sqrt(c["kappa"]))
    S = _sparse(c["M"], "csr", F64, DEV)
    B = torch.from_numpy(c["B"]).to(DEV)
    kw = dict(bounds=c["bounds"], tolerance=tol, num_quad=N_QUAD)
    with torch.no_grad():
        all3 = sparse_inv_sqrt_mm(S, B, **kw)
        alone = sparse_inv_sqrt_mm(S, B[:, 1:2].contiguous(), **kw)
        again = sparse_inv_sqrt_mm(S, B, **kw)
    assert torch.equal(all3, again), "the same call gives the same bits"
    assert _col_err(all3[:, 1:2], alone.cpu().numpy()) <= bound
    zero = B.clone()
    zero[:, 2] = 0
    with torch.no_grad():
        z = sparse_inv_sqrt_mm(S, zero, **kw)
    assert torch.equal(z[:, 2], torch.zeros_like(z[:, 2])) and _col_err(z[:, :2], c["fwd"][:, :2]) <= bound


def test_estimated_bounds_and_max_iter(cases):
    c = cases["lap12x11x10"]
    S = _sparse(c["M"], "csr", F64, DEV)
    B = torch.from_numpy(c["B"]).to(DEV)
    out, info = sparse_inv_sqrt_mm(S, B, tolerance=1e-12, return_info=True)
    lo, hi = info["bounds"]
    assert lo <= c["lam"][0] and hi >= c["lam"][-1] and info["converged"] is True
    # the rule for the estimated interval, on the exact spectrum
    sigma, omega = _ciq_rule(lo, hi, N_QUAD)
    bound = 10.0 * (CR.scalar_error(sigma, omega, c["lam"]) + 1e-12 * np.sqrt(c["kappa"]))
    assert _col_err(out, c["fwd"]) <= bound
    out3, info3 = sparse_inv_sqrt_mm(S, B, bounds=c["bounds"], tolerance=1e-12, max_iter=3, return_info=True)
    assert info3["converged"] is False and info3["iterations"] == 3 and out3.shape == B.shape
    assert float(info3["residual_estimates"].min()) > 1e-12 and bool(torch.isfinite(out3).all())


def test_no_grad_allocates_no_solution_block(cases):
    c = cases["lap12x11x10"]
    n, p, Sq = c["M"].shape[0], 64, N_QUAD                              # (wide enough for 11 planes to dwarf the small arrays)
    S = _sparse(c["M"], "csr", torch.float32, DEV)
    B = torch.randn(n, p, device=DEV)
    kw = dict(bounds=c["bounds"], tolerance=1e-5, num_quad=Sq)
    with torch.no_grad():
        sparse_inv_sqrt_mm(S, B, **kw)                                  # plans, library state
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = sparse_inv_sqrt_mm(S, B, **kw)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(DEV) - base
    plane = n * p * 4
    # 2 S + 6 planes of state (w twice, z twice, the product, the sum, the result, one spare) and the small arrays: scal, partial rows,
    # fold rows, flags (a few hundred KiB at most; the allocator rounds each to 512 bytes)
    small = 1 << 20
    print(f"peak {peak} bytes = {peak / plane:.2f} planes; the state is {2 * Sq + 6} planes, a solution block would add {Sq}")
    assert peak <= (2 * Sq + 6) * plane + small
    assert (2 * Sq + 6) * plane + small < (3 * Sq + 5) * plane, "the bound separates the two"
    del out
