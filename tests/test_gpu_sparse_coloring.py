"""`sparse_coloring`, the coloured `sparse_ilu0` / `sparse_ic0` and `sparse_sgs` on an MI355X: the colouring from the kernels equals the
sequential reference (tests/_coloring_ref.py) exactly for both index types and every group width, the check entry, the factors
bit for bit, the applications within the bound derived in `_coloring_ref`'s docstring, graph capture, and the Krylov loops.
Needs an MI355X: `pytest -m gpu`."""

import warnings

import numpy as np
import pytest
import torch

import _coloring_ref as CR
import _factor_ref as FR
import _trsm_ref as TR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {"f32": np.float32, "f64": np.float64}
TD = {"f32": torch.float32, "f64": torch.float64}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_extension():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def csr(ptr, idx, val=None, idt=torch.int32, dtype=torch.float64):
    n = len(ptr) - 1
    val = np.ones(len(idx)) if val is None else val
    return torch.sparse_csr_tensor(torch.as_tensor(ptr).to(idt).to(DEV), torch.as_tensor(idx).to(idt).to(DEV),
                                   torch.as_tensor(np.asarray(val)).to(dtype).to(DEV), (n, n))


# ---- the colouring ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("idt", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("name", list(CR.PATTERNS))
def test_colouring_equals_the_reference(name, idt):
    from torchsparsegradutils_amd import _backend, _pattern, sparse_coloring

    ptr, idx, ref = CR.case(name)
    k = int(ref.max()) + 1
    M = csr(ptr, idx, idt=idt)
    g = _pattern.from_csr(M)
    lists = _pattern._color_lists(g)
    assert (lists[2] is None) == (name not in ("one_sided300", "random1031"))
    clash = None
    if any(CR.neighbours(ptr, idx)):
        clash = ref.copy()
        i = next(i for i, a in enumerate(CR.neighbours(ptr, idx)) if a)
        clash[i] = clash[min(CR.neighbours(ptr, idx)[i])]
    for group in _backend.color_geometry()[0]:
        colors = _pattern.greedy_colors(g, group=group)
        assert colors.dtype == torch.int32 and np.array_equal(colors.cpu().numpy(), ref), (name, group)
        assert int(_backend.csr_color_check(*lists, colors, len(ref), k, group=group)) == 0
        assert int(_backend.csr_color_check(*lists, colors, len(ref), k - 1, group=group)) == int(np.argmax(ref == k - 1)) + 1
        if clash is not None:
            got = int(_backend.csr_color_check(*lists, torch.as_tensor(clash, device=DEV), len(ref), k, group=group))
            assert got == CR.first_clash(ptr, idx, clash, k) > 0, (name, group)
    c = sparse_coloring(M)
    perm, inverse, offsets = CR.permutation(ref)
    assert np.array_equal(c.colors.cpu().numpy(), ref) and c.n_colors == k and c.offsets == tuple(offsets)
    assert np.array_equal(c.perm.cpu().numpy(), perm) and np.array_equal(c.inverse.cpu().numpy(), inverse)


def test_permute_and_user_colours():
    from torchsparsegradutils_amd import sparse_coloring

    ptr, idx = FR.stencil(5, 4, 3, 7)
    val = np.random.default_rng(1).standard_normal(len(idx))
    M = csr(ptr, idx, val)
    c = sparse_coloring(M)
    assert torch.equal(c.permute(M).to_dense(), M.to_dense()[c.perm][:, c.perm])
    coo = M.to_sparse_coo()
    assert torch.equal(sparse_coloring(coo).colors, c.colors) and torch.equal(c.permute(coo).to_dense(), c.permute(M).to_dense())
    v = torch.as_tensor(val, device=DEV).requires_grad_(True)
    (grad,) = torch.autograd.grad(c.permute(torch.sparse_csr_tensor(M.crow_indices(), M.col_indices(), v, M.shape)).values().sum(), v)
    assert torch.equal(grad, torch.ones_like(grad))
    x, y, z = (a.ravel() for a in np.meshgrid(np.arange(5), np.arange(4), np.arange(3), indexing="ij"))
    rb = (x + y + z) % 2
    user = sparse_coloring(M, colors=torch.as_tensor(rb, device=DEV))
    assert user.n_colors == 2 and user.offsets == (0, 30, 60)
    bad = rb.copy()
    bad[17] = 1 - bad[17]
    low = CR.first_clash(ptr, idx, bad, 2) - 1
    with pytest.raises(ValueError, match=f"row {low} has a neighbour of its own colour"):
        sparse_coloring(M, colors=torch.as_tensor(bad, device=DEV))


# ---- the factors ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_factors_are_those_of_the_permuted_matrix(dtype):
    from torchsparsegradutils_amd import SparseColoredIC0, SparseColoredILU0, sparse_coloring, sparse_ic0, sparse_ilu0

    for name in ("lap27_4x4x4", "convdiff7_5x4x3"):
        ptr, idx, val, sym = CR.problem(name)
        val = TR.round_to(val, dtype)
        M = csr(ptr, idx, val, dtype=TD[dtype])
        c = sparse_coloring(M)
        pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, val, c.inverse.cpu().numpy())
        ilu = sparse_ilu0(M, ordering="multicolor")
        assert isinstance(ilu, SparseColoredILU0) and int(ilu.info) == 0
        want = FR.ilu0(pptr, pidx, pval, dtype=NP[dtype])[0]
        assert np.array_equal(ilu.values.cpu().numpy().view(np.uint8), want.view(np.uint8)), name
        if sym:
            ic = sparse_ic0(M, ordering=c)
            assert isinstance(ic, SparseColoredIC0) and torch.equal(ic.values, sparse_ic0(c.permute(M)).values)
            assert torch.equal(ic.U.to_dense(), ic.L.to_dense().t())


# ---- applications -----------------------------------------------------------------------------------------------------------------------

def _object(kind, M, **kw):
    import torchsparsegradutils_amd as tsgu

    return {"ilu0": tsgu.sparse_ilu0, "ic0": tsgu.sparse_ic0, "sgs": tsgu.sparse_sgs}[kind](M, **kw)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind,name", CR.APPLICATIONS)
def test_applications_within_the_bound(kind, name, dtype):
    ptr, idx, val, _ = CR.problem(name)
    n = len(ptr) - 1
    M = _object(kind, csr(ptr, idx, TR.round_to(val, dtype), dtype=TD[dtype]), ordering="multicolor")
    inverse, perm = M.coloring.inverse.cpu().numpy(), M.coloring.perm.cpu().numpy()
    if kind == "sgs":
        pptr, pidx, pval, _ = CR.permute_csr(ptr, idx, TR.round_to(val, dtype), inverse)
    else:
        pptr, pidx, _, _ = CR.permute_csr(ptr, idx, None, inverse)
        pval = M.values.cpu().numpy().astype(np.float64)
    real = np.longdouble if dtype == "f64" else np.float64
    rng = np.random.default_rng(6)
    worst = 0.0
    for shape in ((n,), (n, 3), (n, 17)):
        R = TR.round_to(rng.standard_normal(shape), dtype)
        Rt = torch.as_tensor(R.astype(NP[dtype]), device=DEV)
        for transpose in (False, True):
            first, second = CR.stages(kind, pptr, pidx, pval, transpose)
            x64, bnd = CR.application(first, second, R.reshape(n, -1)[perm], TR.U[dtype], real=real)
            for X in (M.solve(Rt, transpose=transpose), (M.T(Rt) if transpose else M(Rt))):
                assert X.shape == Rt.shape and X.dtype == Rt.dtype and X.device == Rt.device
                r = TR.ratio(X.cpu().numpy().reshape(n, -1)[perm], x64, bnd)
                worst = max(worst, r)
                assert np.isfinite(r) and r <= 1.0, (kind, name, dtype, shape, transpose, r)
    print(f"{kind} {name} {dtype}: worst error / bound = {worst:.3f}")


def test_sgs_refresh_equals_a_fresh_build():
    from torchsparsegradutils_amd import sparse_sgs

    ptr, idx, val, _ = CR.problem("convdiff7_5x4x3")
    M = sparse_sgs(csr(ptr, idx, val))
    new = csr(ptr, idx, FR.dominant_values(ptr, idx, 99))
    R = torch.randn(60, 2, dtype=torch.float64, device=DEV)
    assert M.refresh(new) is M
    fresh = sparse_sgs(new)
    assert torch.equal(M(R), fresh(R)) and torch.equal(M.T(R), fresh.T(R))


@pytest.mark.parametrize("kind", ["ilu0", "ic0", "sgs"])
def test_a_captured_application_replays_the_same_bits(kind):
    ptr, idx, val, _ = CR.problem("lap27_4x4x4")
    M = _object(kind, csr(ptr, idx, val, dtype=torch.float32), ordering="multicolor")
    R = torch.randn(64, 5, dtype=torch.float32, device=DEV)
    eager = M(R).clone()                                   # (also builds every lazy part of the plan outside the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M(R)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M(R)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- in the Krylov loops ---------------------------------------------------------------------------------------------------------------

def _rel_residual(Mat, x, b):
    return float(torch.linalg.norm(Mat @ x - b) / torch.linalg.norm(b))


@pytest.mark.parametrize("kind", ["ilu0", "ic0", "sgs"])
def test_krylov_loops_reach_their_tolerance(kind):
    import torchsparsegradutils_amd as tsgu
    from torchsparsegradutils_amd.utils import BICGSTABSettings, GMRESSettings, bicgstab, gmres, last_solve_info, linear_cg

    b = torch.randn(120, 2, dtype=torch.float64, device=DEV)
    ptr, idx, val, _ = CR.problem("lap7_6x5x4")
    S = csr(ptr, idx, val)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = linear_cg(S, b, tolerance=1e-10, eps=1e-20, stop_updating_after=1e-20, max_iter=200, max_tridiag_iter=0,
                      preconditioner=_object(kind, S, ordering="multicolor"))
    assert last_solve_info("linear_cg")["tolerance_reached"] and _rel_residual(S.to_dense(), x, b) < 1e-8
    if kind == "ic0":
        return
    ptr, idx, val, _ = CR.problem("convdiff7_5x4x3")
    N = csr(ptr, idx, val)
    b = b[:60].contiguous()
    M = _object(kind, N, ordering="multicolor")
    x = bicgstab(N, b, settings=BICGSTABSettings(reltol=1e-10, precon=M))
    assert _rel_residual(N.to_dense(), x, b) < 1e-8
    x = gmres(N, b, settings=GMRESSettings(reltol=1e-10, precon=M))
    assert _rel_residual(N.to_dense(), x, b) < 1e-8
    Ng = csr(ptr, idx, val).requires_grad_(True)
    x = tsgu.sparse_generic_solve(Ng, b, solve=lambda A_, B_: bicgstab(A_, B_, settings=BICGSTABSettings(reltol=1e-12, precon=M)),
                                  transpose_solve=lambda A_, B_: bicgstab(A_.to_dense().t().contiguous(), B_,
                                                                          settings=BICGSTABSettings(reltol=1e-12, precon=M.T)))
    x.sum().backward()
    assert _rel_residual(N.to_dense(), x.detach(), b) < 1e-8 and Ng.grad is not None


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_coloured_preconditioners_save_iterations_on_the_anisotropic_lattice(dtype):
    """CG to a relative residual of 1e-4 on the 8 x 8 x 8 lattice with coefficients 1:1:1000: the package's CPU path takes 16
    iterations without a preconditioner, 13 with coloured IC(0) and 12 with SGS, in float32 and in float64
    (tests/test_coloring_cpu.py prints them)."""
    import torchsparsegradutils_amd as tsgu

    ptr, idx, val = CR.lattice7(8, 8, 8, (1.0, 1.0, 1000.0))
    S = csr(ptr, idx, val, dtype=TD[dtype])
    D = S.to_dense()
    b = torch.randn(512, dtype=TD[dtype], generator=torch.Generator().manual_seed(0)).to(DEV)
    plain = CR.cg_iterations(D, b, None)
    ic = CR.cg_iterations(D, b, tsgu.sparse_ic0(S, ordering="multicolor"))
    sgs = CR.cg_iterations(D, b, tsgu.sparse_sgs(S))
    print(f"CG to 1e-4 on the 8x8x8 1:1:1000 lattice ({dtype}): plain {plain}, coloured IC(0) {ic}, SGS {sgs}")
    assert ic < plain and sgs < plain
