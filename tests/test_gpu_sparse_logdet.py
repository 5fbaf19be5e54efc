"""`sparse_logdet` / `sparse_inv_quad_logdet` on the GPU through the public interface, against numpy in float64.

probes = I and 48 steps make the quadrature exact on the three test matrices (every column's Krylov space is exhausted before
that), so what is left is the arithmetic of the CG coefficients:

    fp32   |logdet - slogdet| <= 2e-5 |logdet|     about 5·n·ε₃₂ at n <= 96; fp32 coefficients emulated on the CPU give 6e-8
    fp64   |logdet - slogdet| <= 1e-9 |logdet|

A gradient entry is an entry of U = A⁻¹ I from the same run: CG leaves a column at a normalised residual below `cg_tolerance`, so it
is within cg_tolerance / λ_min of inv(A), plus the format's floor 64·ε·‖A⁻¹‖_max.  For B the same per column, scaled by the
column: e_x = |b|₂ cg_tolerance / λ_min + 64 ε ‖A⁻¹‖_max |b|₁ bounds every entry of x_j - x*_j.

COO index tensors are int64 in torch, so the layouts are CSR int32, CSR int64 and COO int64.
"""

import warnings

import numpy as np
import pytest
import torch

import _quadrature_ref as QR
from torchsparsegradutils_amd import sparse_inv_quad_logdet, sparse_logdet

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
VALUE_BOUND = {torch.float32: 2e-5, torch.float64: 1e-9}
CG_TOL = {torch.float32: 1e-4, torch.float64: 1e-10}
LAYOUTS = [("csr", torch.int32), ("csr", torch.int64), ("coo", torch.int64)]


def _sparse(M, layout, itype, td):
    crow, col, val = QR.csr_arrays(M)
    n = M.shape[0]
    v = torch.from_numpy(val).to(td).to(DEV)
    if layout == "csr":
        return torch.sparse_csr_tensor(torch.from_numpy(crow).to(itype).to(DEV), torch.from_numpy(col).to(itype).to(DEV), v, (n, n))
    rows = np.repeat(np.arange(n), np.diff(crow))
    return torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, col))).to(DEV), v, (n, n)).coalesce()


@pytest.fixture(scope="module")
def matrices():
    out = {}
    for name, make in QR.MATRICES.items():
        M = make()
        inv = np.linalg.inv(M)
        out[name] = (M, float(np.linalg.slogdet(M)[1]), inv, float(np.linalg.eigvalsh(M)[0]))
    return out


def _same_indices(g, S, itype):
    assert g.layout == S.layout
    if S.layout == torch.sparse_csr:
        assert g.crow_indices().dtype == itype and g.col_indices().dtype == itype
        assert torch.equal(g.crow_indices(), S.crow_indices()) and torch.equal(g.col_indices(), S.col_indices())
    else:
        assert torch.equal(g._indices(), S._indices())


@pytest.mark.parametrize("td", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout,itype", LAYOUTS)
@pytest.mark.parametrize("name", list(QR.MATRICES))
def test_identity_probes(matrices, name, layout, itype, td):
    M, exact, inv, lam_min = matrices[name]
    n = M.shape[0]
    S = _sparse(M, layout, itype, td).requires_grad_(True)
    tol = CG_TOL[td]
    ld, info = sparse_logdet(S, probes=torch.eye(n, dtype=td, device=DEV), lanczos_steps=48, cg_tolerance=tol, return_info=True)
    assert ld.shape == () and ld.dtype == td and ld.is_cuda
    rel = abs(float(ld) - exact) / abs(exact)
    print(f"{name} {layout} {itype} {td}: |logdet - slogdet| / |logdet| = {rel:.3e}; lengths {int(info['lengths'].min())}.."
          f"{int(info['lengths'].max())}; iterations {info['iterations']}")
    assert rel <= VALUE_BOUND[td]
    ld.backward()
    _same_indices(S.grad, S, itype)
    mask = M != 0
    g = S.grad.to_dense().double().cpu().numpy()
    bound = tol / lam_min + 64 * EPS[td] * np.abs(inv).max()
    err = np.abs(g - inv)[mask].max()
    print(f"    max gradient error on the pattern {err:.3e}, bound {bound:.3e}")
    assert err <= bound and np.all(g[~mask] == 0)


@pytest.mark.parametrize("td", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout,itype", [("csr", torch.int32), ("coo", torch.int64)])
def test_inv_quad_logdet(matrices, layout, itype, td):
    M, exact, inv, lam_min = matrices["rand96"]
    n = M.shape[0]
    Bn = np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32).astype(np.float64)
    X = inv @ Bn
    S = _sparse(M, layout, itype, td).requires_grad_(True)
    B = torch.from_numpy(Bn).to(td).to(DEV).requires_grad_(True)
    tol, eps = CG_TOL[td], EPS[td]
    iq, ld = sparse_inv_quad_logdet(S, B, probes=torch.eye(n, dtype=td, device=DEV), lanczos_steps=48, cg_tolerance=tol)
    assert iq.shape == (3,) and abs(float(ld) - exact) <= VALUE_BOUND[td] * abs(exact)
    b1, b2 = np.abs(Bn).sum(0), np.linalg.norm(Bn, axis=0)
    ex = b2 * tol / lam_min + 64 * eps * np.abs(inv).max() * b1           # per entry of x_j - x*_j
    want_iq = (Bn * X).sum(0)
    err = np.abs(iq.detach().double().cpu().numpy() - want_iq)
    print(f"{layout} {td}: inv_quad errors {err}, bounds {b1 * ex + 64 * eps * (np.abs(Bn) * np.abs(X)).sum(0)}")
    assert np.all(err <= b1 * ex + 64 * eps * (np.abs(Bn) * np.abs(X)).sum(0))
    w = np.array([0.5, -2.0, 1.0])
    (iq * torch.from_numpy(w).to(td).to(DEV)).sum().backward()
    assert np.all(np.abs(B.grad.double().cpu().numpy() - 2 * X * w) <= 2 * np.abs(w) * ex + 64 * eps * np.abs(2 * X * w))
    _same_indices(S.grad, S, itype)
    want = -(X * w) @ X.T
    xmax = np.abs(X).max(0)
    bound = float((np.abs(w) * ex * (2 * xmax + ex)).sum()) + 64 * eps * np.abs(want).max()
    mask = M != 0
    assert np.abs(S.grad.to_dense().double().cpu().numpy() - want)[mask].max() <= bound
    # a 1-D B gives a scalar, and both gradients at once
    S.grad = None
    iq1, ld1 = sparse_inv_quad_logdet(S, B.detach()[:, 0], probes=torch.eye(n, dtype=td, device=DEV), lanczos_steps=48, cg_tolerance=tol)
    assert iq1.shape == () and abs(float(iq1) - want_iq[0]) <= b1[0] * ex[0] + 64 * eps * (np.abs(Bn) * np.abs(X)).sum(0)[0]
    (ld1 + iq1).backward()
    both = inv - np.outer(X[:, 0], X[:, 0])
    bound = tol / lam_min + 64 * eps * np.abs(inv).max() + ex[0] * (2 * xmax[0] + ex[0]) + 64 * eps * np.abs(both).max()
    assert np.abs(S.grad.to_dense().double().cpu().numpy() - both)[mask].max() <= bound


@pytest.mark.parametrize("td", [torch.float32, torch.float64])
def test_the_fused_loop_runs_and_its_fallback_agrees(matrices, monkeypatch, td):
    """The forward takes the fused two-launch CG loop; where that declines, the tensor-op loop feeds the same kernel (kind 0) and
    meets the same bounds."""
    import importlib

    from torchsparsegradutils_amd.utils._operator import LAST_SOLVE

    lcg = importlib.import_module("torchsparsegradutils_amd.utils.linear_cg")      # (the package exports the function under this name)

    M, exact, inv, lam_min = matrices["lap7x9"]
    S = _sparse(M, "csr", torch.int32, td)
    kw = dict(probes=torch.eye(63, dtype=td, device=DEV), lanczos_steps=48, cg_tolerance=CG_TOL[td], return_info=True)
    ld, info = sparse_logdet(S, **kw)
    assert LAST_SOLVE.info["sparse_logdet"]["fused"] is True
    monkeypatch.setattr(lcg, "TWO_LAUNCH", False)
    ld2, info2 = sparse_logdet(S, **kw)
    assert LAST_SOLVE.info["sparse_logdet"]["fused"] is False
    print(f"{td}: fused {float(ld):.9f}, tensor-op loop {float(ld2):.9f}, exact {exact:.9f}")
    assert abs(float(ld2) - exact) <= VALUE_BOUND[td] * abs(exact) and abs(float(ld) - exact) <= VALUE_BOUND[td] * abs(exact)
    assert int(info2["lengths"].min()) >= 1 and int(info2["lengths"].max()) <= 48


def test_same_seed_on_cpu_and_gpu():
    M = QR.laplacian5(32, 32, 0.5)
    kw = dict(num_probes=64, seed=5)
    Sc = _sparse(M, "csr", torch.int64, torch.float64).cpu()
    cpu30 = float(sparse_logdet(Sc, lanczos_steps=30, **kw))
    cpu60 = float(sparse_logdet(Sc, lanczos_steps=60, **kw))
    gpu30 = float(sparse_logdet(_sparse(M, "csr", torch.int32, torch.float32), lanczos_steps=30, **kw))
    print(f"seed 5: cpu fp64 {cpu30:.6f} (60 steps: {cpu60:.6f}), gpu fp32 {gpu30:.6f}")
    assert abs(gpu30 - cpu30) <= 2e-5 * abs(cpu30) + abs(cpu30 - cpu60)


@pytest.mark.parametrize("td", [torch.float32, torch.float64])
def test_more_than_256_columns(td):
    n = 300
    M = QR.random_dominant(n, 4, 0.3, seed=2)
    exact = float(np.linalg.slogdet(M)[1])
    S = _sparse(M, "csr", torch.int32, td)
    eye = torch.eye(n, dtype=td, device=DEV)
    kw = dict(lanczos_steps=48, cg_tolerance=CG_TOL[td], return_info=True)
    ld, info = sparse_logdet(S, probes=eye, **kw)
    assert len(info["iterations"]) == 2 and info["estimates"].shape == (n,) and info["residual_norms"].shape == (n,)
    bound = 5 * n * EPS[td] if td == torch.float32 else VALUE_BOUND[td]      # (the fp32 bound's own rule, 5·n·ε₃₂, at n = 300: 8.9e-5)
    print(f"n = 300 {td}: |logdet - slogdet| / |logdet| = {abs(float(ld) - exact) / abs(exact):.3e}")
    assert abs(float(ld) - exact) <= bound * abs(exact)
    parts = [sparse_logdet(S, probes=eye[:, a:b].contiguous(), **kw)[1]["estimates"] for a, b in ((0, 256), (256, n))]
    chunks = torch.cat(parts)
    assert float((info["estimates"] - chunks).abs().max()) <= VALUE_BOUND[td] * float(chunks.abs().max())
    assert abs(float(ld) - float(chunks.sum())) <= VALUE_BOUND[td] * abs(exact)


@pytest.mark.parametrize("td", [torch.float32, torch.float64])
def test_an_indefinite_matrix_raises(td):
    M = QR.laplacian5(8, 8, 0.5) - 5.0 * np.eye(64)
    assert np.linalg.eigvalsh(M)[0] < 0 < np.linalg.eigvalsh(M)[-1]
    S = _sparse(M, "csr", torch.int32, td)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError, match=r"sparse_logdet: A is not positive definite \(a Lanczos tridiagonal has a non-positive "
                                               r"eigenvalue\)"):
            sparse_logdet(S, probes=torch.eye(64, dtype=td, device=DEV), lanczos_steps=48)
        with pytest.raises(RuntimeError, match="A is not positive definite"):
            sparse_logdet(S, num_probes=16, lanczos_steps=30)


def test_rademacher_estimate_within_four_standard_errors():
    M = QR.laplacian5(32, 32, 0.5)
    exact = float(np.linalg.slogdet(M)[1])
    S = _sparse(M, "csr", torch.int32, torch.float32)
    est, info = sparse_logdet(S, num_probes=64, lanczos_steps=30, seed=0, return_info=True)
    stderr = float(info["stderr"])
    print(f"Rademacher fp32: estimate {float(est):.4f}, exact {exact:.4f}, stderr {stderr:.4f}, |error| / stderr "
          f"{abs(float(est) - exact) / stderr:.3f}")
    assert abs(float(est) - exact) <= 4 * stderr
    assert float(sparse_logdet(S, num_probes=64, lanczos_steps=30, seed=0)) == float(est)
