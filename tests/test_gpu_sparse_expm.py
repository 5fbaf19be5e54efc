"""`sparse_expm_mm` on the GPU, end to end, against the dense float64 exponential (`eigh` for the values, `grad_B` and `grad_t`,
the Daleckii–Krein formula for `grad_A`: tests/_expm_ref.py) and against the package's CPU path.

Bound (fp64, tolerance 1e-12, Gershgorin bounds).  With S = e^{max(t·lo, t·hi)} the expansion is cut where, before rounding,
‖y − exp(tA) b‖₂ ≤ tolerance·S·‖b‖₂ per column.  The test allows ten times that plus the error the torch-op path makes on the same
inputs (its rounding: the same K steps in another summation order):

  values    10·tolerance·S·‖b_c‖ per column c and time
  grad_B    μ_0 = Σ_j p_j(A) G_j, the same polynomial applied to G: Σ_j 10·tolerance·S_j·‖g_jc‖ per column
  grad_t    ⟨g, A y⟩ with the exact A: |error| ≤ ‖g_jc‖·max(|lo|, |hi|)·(the value bound of column c)
  grad_A    the derivative of the tail r = Σ_{k>K} c_k T_k(Â): by Daleckii–Krein its Frobenius norm is at most max|r'|·‖G Bᵀ‖_F, and
            max|r'| ≤ a·Σ_{k>K} |c_k|·k².  The ratio ive_{k+1}/ive_k is below |z|/(2k + 2) ≤ 1/2 once k ≥ |z| (K > |z| in every case
            here, asserted), so Σ_{k>K} |c_k| k² ≤ (K+1)²·|c_{K+1}|·Σ_i (1+i)²/2^i = 12·(K+1)²·|c_{K+1}| and |c_{K+1}| ≤ tolerance·S:
            10·12·(K+1)²·a·tolerance·Σ_j S_j·‖G_j‖_F·‖B‖_F over the stored entries.

fp32 (tolerance 1e-6) has no derived margin: the error of the torch-op path in fp32 on the same inputs against float64 is
measured in the test, and the GPU's error may be at most 4 times that, floored at the truncation bounds above themselves (ONE times
them, not the ten of the fp64 test: two correct fp32 runs of the same K steps with different summation orders).  For the values and
`grad_B` the floor is of the size of the fp32 errors, so the 4× rule is what binds; the floors of `grad_A` and `grad_t` carry the
worst-case factors 12·(K+1)² and max(|lo|, |hi|)·‖g‖ and stay far above the fp32 errors — there the fp32 arithmetic is held by the
one-launch bounds of tests/test_gpu_expm_steps.py and by the fp64 run of the same loops.  All figures are printed; DESIGN.md §6 has
those of one run.
"""

import numpy as np
import pytest
import torch

import _expm_ref as ER
from torchsparsegradutils_amd import sparse_expm_mm
from torchsparsegradutils_amd.sparse_expm import _SDDMM_WIDTH, _entry
from torchsparsegradutils_amd.utils._operator import LAST_SOLVE

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = torch.float64
NAMES = ["lap6x5x4", "random200"]

# name -> (times as nested lists or a float, how t is passed, p, chunk override)
CONFIGS = {
    "negative float": (-0.7, "float", 3, None),
    "positive 0-d": (0.4, "tensor", 3, None),
    "three times": ([-1.0, 0.3, -0.1], "tensor", 3, None),
    "per channel": ([[-0.9, 0.2, -0.05, 0.5, -0.4]], "tensor", 5, None),
    "p = 300": (-0.5, "float", 300, None),
    "chunk = 1": ([-0.6, 0.25], "tensor", 3, 1),
    "chunk = 4": ([-0.6, 0.25], "tensor", 3, 4),
}


def _sparse(M, layout, dtype, device):
    crow, col, val = ER.csr_arrays(M)
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
    """(name, config) -> dict of the float64 truth, computed once and never written to."""
    out = {}
    for name in NAMES:
        M = ER.MATRICES[name]()
        n = M.shape[0]
        lo, hi = ER.gershgorin(M)
        for cfg, (times, _, p, _) in CONFIGS.items():
            rng = np.random.default_rng(len(out) + 11)
            T = 1 if np.ndim(times) == 0 else len(times)
            out[name, cfg] = ER.make_case(M, rng.standard_normal((n, p)), rng.standard_normal((T, n, p)), times, lo, hi)
    return out


def _run(c, cfg, layout, dtype, device, tolerance):
    times, how, p, chunk = CONFIGS[cfg]
    A = _sparse(c["M"], layout, dtype, device).requires_grad_(True)
    B = torch.from_numpy(c["B"]).to(dtype).to(device).requires_grad_(True)
    t = torch.tensor(times, dtype=dtype, device=device, requires_grad=True) if how == "tensor" else float(times)
    out, info = _entry(A, B, t, None, tolerance, 4096, True, chunk=chunk)
    G = torch.from_numpy(c["G"]).to(dtype).to(device)
    out.backward(G.reshape(out.shape))
    gA = A.grad.values() if layout == "csr" else A.grad._values()
    gt = None if how != "tensor" else t.grad.detach().cpu().double().numpy()
    return (out.detach().cpu().double().numpy().reshape(c["Y"].shape), B.grad.cpu().double().numpy(), gA.cpu().double().numpy(), gt, info)


def _errors(c, res):
    return ER.errors(c, res[0], res[1], res[2], res[3])


def _truncation(c, K, a, tolerance, factor=10.0):
    return ER.error_bounds(c, K, a, tolerance, factor)


def _common(c, cfg, info):
    p = CONFIGS[cfg][2]
    K = info["terms"]
    rho = 0.5 * (c["hi"] - c["lo"])
    assert K > np.abs(c["t2"]).max() * rho, "the grad_A bound needs K > |z|"
    assert info["bounds"] == pytest.approx((c["lo"], c["hi"]), rel=1e-5)
    if CONFIGS[cfg][3] is None:
        assert info["chunk"] == max(1, min(K + 1, 64, _SDDMM_WIDTH // p))
    else:
        assert info["chunk"] == CONFIGS[cfg][3]
    return K, 1.0 / rho


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("name", NAMES)
def test_fp64_against_dense_and_the_cpu_path(cases, name, layout, cfg):
    c = cases[name, cfg]
    tol = 1e-12
    gpu = _run(c, cfg, layout, F64, DEV, tol)
    info = gpu[4]
    assert info["fused"] is True and LAST_SOLVE.info["sparse_expm_mm"]["fused"] is True
    K, a = _common(c, cfg, info)
    if cfg == "p = 300":
        assert info["chunk"] == 3 and K + 1 > 2 * 3, "many chunk boundaries are crossed"
    cpu = _run(c, cfg, layout, F64, "cpu", tol)
    assert cpu[4]["fused"] is False and cpu[4]["terms"] == K
    e_gpu, e_cpu, trunc = _errors(c, gpu), _errors(c, cpu), _truncation(c, K, a, tol)
    for key, err in e_gpu.items():
        allowed = trunc[key] + e_cpu[key]
        print(f"{name} {layout} {cfg} K {K} chunk {info['chunk']}: {key} gpu {float(err.max()):.2e} cpu {float(e_cpu[key].max()):.2e} "
              f"truncation bound {float(np.max(trunc[key])):.2e}")
        assert np.all(err <= allowed), (key, float((err / allowed).max()))
    again = _run(c, cfg, layout, F64, DEV, tol)
    for x, y in zip(gpu[:4], again[:4]):
        assert (x is None and y is None) or np.array_equal(x, y), "two calls give the same bits"


@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("name", NAMES)
def test_fp32_against_the_cpu_paths_own_error(cases, name, layout, cfg):
    c = cases[name, cfg]
    tol = 1e-6
    gpu = _run(c, cfg, layout, torch.float32, DEV, tol)
    cpu = _run(c, cfg, layout, torch.float32, "cpu", tol)
    info = gpu[4]
    assert info["fused"] is True and cpu[4]["terms"] == info["terms"]
    K = info["terms"]
    a = 2.0 / (info["bounds"][1] - info["bounds"][0])
    e_gpu, e_cpu, trunc = _errors(c, gpu), _errors(c, cpu), _truncation(c, K, a, tol, factor=1.0)
    for key, err in e_gpu.items():
        allowed = np.maximum(4.0 * e_cpu[key], trunc[key])
        print(f"{name} fp32 {layout} {cfg} K {K}: {key} gpu {float(err.max()):.2e} cpu {float(e_cpu[key].max()):.2e} "
              f"truncation bound {float(np.max(trunc[key])):.2e}")
        assert np.all(err <= allowed), (key, float((err / allowed).max()))


@pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["f32", "f64"])
def test_zero_time_the_one_by_one_matrix_and_given_bounds(cases, dtype):
    c = cases["lap6x5x4", "negative float"]
    A = _sparse(c["M"], "csr", dtype, DEV)
    B = torch.from_numpy(c["B"]).to(dtype).to(DEV)
    assert torch.equal(sparse_expm_mm(A, B, 0.0), B), "t = 0 returns B's bits"
    z = sparse_expm_mm(A, B, torch.zeros(2, dtype=dtype, device=DEV))
    assert z.shape == (2,) + B.shape and torch.equal(z[0], B) and torch.equal(z[1], B)
    vec = sparse_expm_mm(A, B[:, 0].contiguous(), -0.7, tolerance=1e-6 if dtype == torch.float32 else 1e-12)
    assert vec.shape == (B.size(0),)
    rel = np.linalg.norm(vec.cpu().double().numpy() - c["Y"][0, :, 0]) / np.linalg.norm(c["B"][:, 0])
    assert rel <= (1e-5 if dtype == torch.float32 else 1e-11)
    # given bounds: the true spectrum needs fewer terms than Gershgorin's interval and gives the same result
    lam = np.linalg.eigvalsh(c["M"])
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    tight, info_t = sparse_expm_mm(A, B, -0.7, bounds=(float(lam[0]), float(lam[-1])), tolerance=tol, return_info=True)
    loose, info_l = sparse_expm_mm(A, B, -0.7, tolerance=tol, return_info=True)
    assert info_t["terms"] <= info_l["terms"] and info_t["fused"] and info_t["bounds"] == (float(lam[0]), float(lam[-1]))
    nb = np.linalg.norm(c["B"], axis=0)
    for got in (tight, loose):
        err = np.linalg.norm(got.cpu().double().numpy() - c["Y"][0], axis=0)
        assert np.all(err <= (1e-5 if dtype == torch.float32 else 1e-11) * nb)
    # the 1 x 1 matrix: Gershgorin's interval is a point, the result e^{t a_11} b
    one = _sparse(ER.MATRICES["one"](), "coo", dtype, DEV)
    b = torch.tensor([[2.0, -3.0]], dtype=dtype, device=DEV)
    got, info = sparse_expm_mm(one, b, 0.5, return_info=True)
    assert info["terms"] == 0 and info["bounds"] == (0.75, 0.75)
    want = np.exp(0.375) * np.array([[2.0, -3.0]])
    assert np.abs(got.cpu().double().numpy() - want).max() <= 4 * float(torch.finfo(dtype).eps) * 3.0 * np.exp(0.375)


@pytest.mark.parametrize("dtype", [torch.float32, F64], ids=["f32", "f64"])
def test_a_gradient_does_not_depend_on_which_others_are_asked_for(cases, dtype):
    """Only A, only B or only t requiring a gradient: the same bits as when all three do (the backward skips work, not steps)."""
    cfg = "chunk = 4"
    c = cases["lap6x5x4", cfg]
    times = CONFIGS[cfg][0]
    G = torch.from_numpy(c["G"]).to(dtype).to(DEV)

    def run(need_a, need_b, need_t):
        A = _sparse(c["M"], "csr", dtype, DEV).requires_grad_(need_a)
        B = torch.from_numpy(c["B"]).to(dtype).to(DEV).requires_grad_(need_b)
        t = torch.tensor(times, dtype=dtype, device=DEV, requires_grad=need_t)
        out = _entry(A, B, t, None, 1e-6, 4096, False, chunk=4)
        out.backward(G)
        return (A.grad.values() if need_a else None, B.grad, t.grad)

    full = run(True, True, True)
    for k, only in enumerate(((True, False, False), (False, True, False), (False, False, True))):
        got = run(*only)
        assert torch.equal(got[k], full[k]), ("grad_A", "grad_B", "grad_t")[k]
        assert all(g is None for j, g in enumerate(got) if j != k)
