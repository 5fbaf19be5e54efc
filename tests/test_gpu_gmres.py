"""`gmres` / `gmres_t` on the GPU: the fused Arnoldi kernels (csrc/gmres.hip) through the public interface.

Two small nonsymmetric matrices (tests/_gmres_ref.py): upwind convection-diffusion on a 6 x 5 x 4 lattice (n = 120) and a random
sparse matrix plus a diagonal shift (n = 97).  Tolerances are chosen on the CPU so that every stopping decision of the float64
mirror is at least 1 % away from its threshold: there the fused path, the torch-op path and the mirror take the same decisions and
the iteration counts must be equal.

Bounds (derived): a returned column has a true residual of at most threshold_c by construction (a column is finished only on the
recomputed residual), so |x - x*| <= |A^-1|_2 threshold_c, and two paths differ by at most the sum of their bounds; the float64
evaluation of the residual of the returned x may exceed the threshold by the rounding of the kernel's own evaluation,
gamma_{r+1}(u) (| |A| |x| | + |b|) with r the longest row plus one for the subtraction.
"""

import sys

import numpy as np
import pytest
import torch

import _gmres_ref as GR
from torchsparsegradutils_amd import _backend, sparse_fsai, sparse_generic_solve, sparse_ilu0
from torchsparsegradutils_amd.utils import GMRESSettings, _graph, gmres, gmres_t, last_solve_info

gmres_mod = sys.modules["torchsparsegradutils_amd.utils.gmres"]      # (the package attribute of that name is the function)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64]
MATRICES = {"convdiff": GR.convdiff, "random": GR.random_shifted}
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


@pytest.fixture(scope="module")
def cases():
    """name -> (A float64, B float64 (n, 3) with a zero column, |A^-1|_2, exact solution, reltol kept away from thresholds)."""
    out = {}
    for name, make in MATRICES.items():
        A = make()
        rng = np.random.default_rng(11)
        B = rng.standard_normal((A.shape[0], 3))
        B[:, 1] = 0.0
        inv_norm = 1.0 / np.linalg.svd(A, compute_uv=False)[-1]
        out[name] = (A, B, inv_norm, np.linalg.solve(A, B), {m: GR.pick_reltol(A, B, m) for m in (5, 30)})
    return out


def _sparse(A, td, layout="csr"):
    t = torch.from_numpy(A).to(td).to(DEV).to_sparse_coo().coalesce()
    return t.to_sparse_csr() if layout == "csr" else t


def _unfused(fn):
    gmres_mod.ENABLE_FUSED = False
    try:
        return fn()
    finally:
        gmres_mod.ENABLE_FUSED = True


def _threshold(A, B, reltol):
    return reltol * np.linalg.norm(B, axis=0)          # x0 = 0, abstol = 0


@pytest.mark.parametrize("td", DTYPES)
@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("m", [5, 30])
def test_fused_against_unfused_and_the_mirror(cases, name, td, m):
    A, B, inv_norm, Xs, tols = cases[name]
    tol = tols[m]
    As, Bt = _sparse(A, td), torch.from_numpy(B).to(td).to(DEV)
    st = GMRESSettings(restart=m, reltol=tol, abstol=0.0)
    x = gmres(As, Bt, settings=st)
    info = last_solve_info("gmres")
    assert info["fused"] and info["restart"] == m
    x2 = gmres(As, Bt, settings=st)
    assert torch.equal(x, x2), "the same call twice must give the same bits"
    xu = _unfused(lambda: gmres(As, Bt, settings=st))
    info_u = last_solve_info("gmres")
    assert not info_u["fused"]
    _, its, _, margin = GR.solve(A, B, m, abstol=0.0, reltol=tol)
    assert margin >= 0.01
    print(f"[gmres] {name} {td} m={m}: iterations fused {info['iterations'].tolist()} unfused {info_u['iterations'].tolist()} "
          f"mirror {its.tolist()}")
    assert info["iterations"].tolist() == info_u["iterations"].tolist() == its.tolist()
    assert its[1] == 0 and not x[:, 1].any(), "a zero column: x = 0, zero iterations"
    thr = _threshold(A, B, tol)
    Af, xf, xuf = A.astype(np.float64), x.double().cpu().numpy(), xu.double().cpu().numpy()
    Ar, Br = (torch.from_numpy(A).to(td).double().numpy(), torch.from_numpy(B).to(td).double().numpy())      # what the kernels saw
    Xr = np.linalg.solve(Ar, Br)
    err, err_u = np.linalg.norm(xf - Xr, axis=0), np.linalg.norm(xuf - Xr, axis=0)
    inv_r = 1.0 / np.linalg.svd(Ar, compute_uv=False)[-1]
    longest = int((Af != 0).sum(axis=1).max())
    slack = GR.gamma(longest + 1, U[td]) * (np.linalg.norm(np.abs(Ar) @ np.abs(xf), axis=0) + np.linalg.norm(Br, axis=0))
    res = np.linalg.norm(Br - Ar @ xf, axis=0)
    print(f"[gmres] residual / (threshold + slack) = {(res / np.where(thr + slack > 0, thr + slack, 1)).max():.3f}, "
          f"error / bound = {(err / np.where(thr > 0, inv_r * (thr + slack), 1)).max():.3f}")
    assert (res <= thr + slack).all()
    assert (err <= inv_r * (thr + slack)).all()
    assert (np.linalg.norm(xf - xuf, axis=0) <= 2 * inv_r * (thr + slack)).all()
    assert (err_u <= inv_r * (thr + slack)).all()


@pytest.mark.parametrize("td", DTYPES)
def test_coo_transpose_and_preconditioner_objects(cases, td):
    A, B, inv_norm, Xs, tols = cases["convdiff"]
    tol = 1e-4 if td == torch.float32 else 1e-9
    Bt = torch.from_numpy(B).to(td).to(DEV)
    csr, coo = _sparse(A, td), _sparse(A, td, "coo")
    st = GMRESSettings(restart=30, reltol=tol, abstol=0.0)
    x = gmres(csr, Bt, settings=st)
    assert torch.equal(x, gmres(coo, Bt, settings=st)), "CSR and COO operands walk the same plan"
    thr = torch.from_numpy(_threshold(A, B, tol)).to(DEV)
    Ad = torch.from_numpy(A).to(td).double().to(DEV)
    longest = int((A != 0).sum(axis=1).max())

    def residual_ok(x, M):
        xd = x.double()
        slack = GR.gamma(longest + 1, U[td]) * (torch.linalg.vector_norm(M.abs() @ xd.abs(), dim=0)
                                                + torch.linalg.vector_norm(Bt.double(), dim=0))
        res = torch.linalg.vector_norm(Bt.double() - M @ xd, dim=0)
        assert bool((res <= thr + slack).all()), (res / (thr + slack)).tolist()

    residual_ok(x, Ad)
    xt = gmres_t(csr, Bt, settings=st)
    residual_ok(xt, Ad.t())
    assert torch.equal(xt, gmres(csr, Bt, settings=st._replace(transpose=True)))
    At = _sparse(np.ascontiguousarray(A.T), td)
    residual_ok(gmres(At, Bt, settings=st), Ad.t())
    for make in (sparse_fsai, sparse_ilu0):
        M = make(csr)
        for tr in (False, True):
            xp = gmres(csr, Bt, settings=st._replace(precon=M, transpose=tr))
            residual_ok(xp, Ad.t() if tr else Ad)
            print(f"[gmres] {make.__name__} transpose={tr} {td}: iterations {last_solve_info('gmres')['iterations'].tolist()}")
            xf = gmres(csr, Bt, settings=st._replace(precon=M, transpose=tr, flexible=True))
            residual_ok(xf, Ad.t() if tr else Ad)


@pytest.mark.parametrize("td", DTYPES)
def test_capture_gives_the_same_bits(cases, td):
    A, B, *_ = cases["random"]
    Bt = torch.from_numpy(B).to(td).to(DEV)
    As = _sparse(A, td)
    # an unreachable tolerance: the solve runs until maxiter, long enough for a capture (restart 4: cycles 2 ... are replays)
    st = GMRESSettings(restart=4, reltol=0.0, abstol=0.0, maxiter=120)
    saved = _graph.MIN_ITERS
    try:
        _graph.MIN_ITERS = 8
        before = _graph.STATS["captures"]
        x = gmres(As, Bt, settings=st)
        assert _graph.STATS["captures"] == before + 1, _graph.STATS
        its = last_solve_info("gmres")["iterations"].tolist()
        _graph.MIN_ITERS = 0
        y = gmres(As, Bt, settings=st)
        assert _graph.STATS["captures"] == before + 1
    finally:
        _graph.MIN_ITERS = saved
    assert torch.equal(x, y) and its == last_solve_info("gmres")["iterations"].tolist()
    assert its[1] == 0 and max(its) > 8, "the solve must run past the first, eager cycles"


def test_257_columns_run_in_slabs(cases):
    A, B, *_ = cases["convdiff"]
    td = torch.float32
    rng = np.random.default_rng(3)
    Bw = torch.from_numpy(rng.standard_normal((A.shape[0], 257))).to(td).to(DEV)
    As = _sparse(A, td)
    st = GMRESSettings(restart=30, reltol=1e-4, abstol=0.0)
    X = gmres(As, Bw, settings=st)
    assert X.shape == Bw.shape
    assert torch.equal(X[:, :256], gmres(As, Bw[:, :256].contiguous(), settings=st)), "a slab does not depend on the columns outside it"
    assert torch.equal(X[:, 256], gmres(As, Bw[:, 256].contiguous(), settings=st))
    Ad = torch.from_numpy(A).to(td).double().to(DEV)
    res = torch.linalg.vector_norm(Bw.double() - Ad @ X.double(), dim=0)
    longest = int((A != 0).sum(axis=1).max())
    slack = GR.gamma(longest + 1, U[td]) * (torch.linalg.vector_norm(Ad.abs() @ X.double().abs(), dim=0)
                                            + torch.linalg.vector_norm(Bw.double(), dim=0))
    assert bool((res <= 1e-4 * torch.linalg.vector_norm(Bw.double(), dim=0) + slack).all())


def test_an_offset_right_hand_side_and_restart_above_the_cap(cases):
    A, B, *_ = cases["convdiff"]
    td = torch.float32
    n = A.shape[0]
    As = _sparse(A, td)
    big = torch.zeros(n + 1, dtype=td, device=DEV)
    big[1:] = torch.from_numpy(B[:, 0]).to(td).to(DEV)
    b = big[1:]                                              # contiguous, 4 bytes past a 16-byte boundary
    assert b.is_contiguous() and b.data_ptr() % 16 != 0
    st = GMRESSettings(restart=30, reltol=1e-4, abstol=0.0)
    x = gmres(As, b, settings=st)
    assert last_solve_info("gmres")["fused"] and last_solve_info("gmres")["finished"] is True
    assert torch.equal(x, gmres(As, b.clone(), settings=st)), "an operand at an odd offset is copied, not refused"
    x0 = torch.zeros(n + 1, dtype=td, device=DEV)[1:]
    assert torch.equal(x, gmres(As, b, initial_guess=x0, settings=st))
    # restart above the kernels' cap: the torch-op path, not an error
    cap = _backend.gmres_geometry(td, n, 1)[0]
    assert n > cap + 1
    y = gmres(As, b, settings=st._replace(restart=cap))
    assert last_solve_info("gmres")["fused"] is True
    z = gmres(As, b, settings=st._replace(restart=cap + 1))
    info = last_solve_info("gmres")
    assert info["fused"] is False and info["restart"] == cap + 1
    Ad = torch.from_numpy(A).to(td).double().to(DEV)
    longest = int((A != 0).sum(axis=1).max())
    for sol in (x, y, z):
        slack = GR.gamma(longest + 1, U[td]) * (torch.linalg.vector_norm(Ad.abs() @ sol.double().abs()) + b.double().norm())
        assert float((b.double() - Ad @ sol.double()).norm()) <= 1e-4 * float(b.double().norm()) + float(slack)
    # a solve cut off above its threshold says so
    gmres(As, b, settings=st._replace(maxiter=3))
    assert last_solve_info("gmres")["finished"] is False and last_solve_info("gmres")["iterations"].tolist() == [3]


def test_autograd_pair_on_a_nonsymmetric_matrix(cases):
    A, B, inv_norm, *_ = cases["convdiff"]
    td = torch.float64
    As = _sparse(A, td).requires_grad_(True)
    Bt = torch.from_numpy(B[:, [0, 2]]).to(DEV).requires_grad_(True)
    Ad = torch.from_numpy(A).to(DEV).requires_grad_(True)
    Bd = Bt.detach().clone().requires_grad_(True)
    tol = 1e-12
    st = GMRESSettings(restart=30, reltol=tol, abstol=0.0)
    W = torch.from_numpy(np.random.default_rng(2).standard_normal((A.shape[0], 2))).to(DEV)
    x = sparse_generic_solve(As, Bt, solve=gmres, transpose_solve=gmres_t, settings=st)
    (x * W).sum().backward()
    xd = torch.linalg.solve(Ad, Bd)
    (xd * W).sum().backward()
    thr_x = tol * torch.linalg.vector_norm(Bd.detach(), dim=0)
    thr_g = tol * torch.linalg.vector_norm(W, dim=0)
    ex = torch.linalg.vector_norm(x.detach() - xd.detach(), dim=0)
    eg = torch.linalg.vector_norm(Bt.grad - Bd.grad, dim=0)
    # what the comparison adds to |A^-1| threshold: the rounding of the kernel's own residual evaluation (as in the tests above),
    # and the error of the dense reference, LU with partial pivoting on a diagonally dominant matrix (no growth):
    # |x^ - x*| <= gamma_{3n}(u) kappa_2(A) |x*|  (Higham, Accuracy and Stability, 9.4 and 9.14)
    n, u = A.shape[0], 2.0 ** -53
    longest = int((A != 0).sum(axis=1).max())
    kappa = inv_norm * float(np.linalg.svd(A, compute_uv=False)[0])
    Aabs = Ad.detach().abs()

    def slack_of(M, sol, rhs, exact):
        own = GR.gamma(longest + 1, u) * (torch.linalg.vector_norm(M @ sol.abs(), dim=0) + torch.linalg.vector_norm(rhs, dim=0))
        return inv_norm * own + GR.gamma(3 * n, u) * kappa * torch.linalg.vector_norm(exact, dim=0)

    u_slack = slack_of(Aabs, x.detach(), Bd.detach(), xd.detach())
    g_slack = slack_of(Aabs.t(), Bt.grad, W, Bd.grad)
    assert bool((ex <= inv_norm * thr_x + u_slack).all())
    assert bool((eg <= inv_norm * thr_g + g_slack).all()), (eg, inv_norm * thr_g)
    gA = As.grad
    assert gA.layout == torch.sparse_csr and torch.equal(gA.crow_indices(), As.crow_indices()) and \
        torch.equal(gA.col_indices(), As.col_indices()), "the pattern is preserved"
    rows = torch.repeat_interleave(torch.arange(A.shape[0], device=DEV), As.crow_indices().diff())
    cols = As.col_indices().long()
    ref = Ad.grad[rows, cols]
    # |g_i x_j - g*_i x*_j| <= |g_i - g*_i| |x_j| + |g*_i| |x_j - x*_j|, summed over the right-hand sides, with the column norms above
    gs, xs = Bd.grad.abs(), xd.detach().abs()
    bound = ((inv_norm * thr_g + g_slack) * xs[cols] + gs[rows] * (inv_norm * thr_x + u_slack)).sum(dim=1) \
        + (inv_norm * thr_g + g_slack).mul(inv_norm * thr_x + u_slack).sum()
    assert bool(((gA.values() - ref).abs() <= bound).all()), ((gA.values() - ref).abs() / bound).max()
