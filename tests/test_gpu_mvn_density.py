"""The sparse multivariate normal's density on the GPU (csrc/mvn.hip + the solve / transposed product it is built on): the golden
and encoder_mvn.npz comparisons of tests/test_mvn_density_cpu.py through the HIP path, the encoder's real shape (N = 262 144)
against a float64 evaluation with torch's CPU sparse ops, memory, reproducibility and graph capture.  Needs an MI355X: `pytest -m gpu`.

Tolerances are the project's own (tests/test_gpu_next_rows.py, rsample on the same inputs): max|got − want| / max|want| below 1e-5
in float32 and 1e-12 in float64 for values, the same bounds normwise for every gradient."""

import warnings

import pytest
import torch

import _golden as G
import _mvn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_extension():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield
    _backend.poll_errors(block=True)


def _leaf(A):
    return A.detach().requires_grad_(True)


# --------------------------------------------------------------------------- the Native class against the reference's golden vectors
@pytest.mark.parametrize("iname", ["i32", "i64"])
@pytest.mark.parametrize("vn", ["f32", "f64"])
def test_native_matches_the_reference_golden(vn, iname):
    import torchsparsegradutils_amd.distributions.sparse_multivariate_normal as smn
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormalNative

    z = G.load("mvn_native.npz")
    dt = torch.float32 if vn == "f32" else torch.float64
    tol = R.TOL[dt]
    L = torch.sparse_csr_tensor(G.t(z[f"{vn}_{iname}_crow"], DEV), G.t(z[f"{vn}_{iname}_col"], DEV), G.t(z[vn + "_val"], DEV), (96, 96))
    loc, x, eps = G.t(z[vn + "_loc"], DEV), G.t(z[vn + "_x"], DEV), G.t(z[vn + "_eps"], DEV)
    dist = SparseMultivariateNormalNative(loc, L)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lp1, lp7, var = dist.log_prob(x[0]), dist.log_prob(x), dist.variance
    assert lp1.shape == () and lp7.shape == (7,) and var.shape == (96,) and lp7.dtype == dt and lp7.is_cuda
    errs = {"lp1": R.rel(lp1, z[vn + "_lp1"]), "lp7": R.rel(lp7, z[vn + "_lp7"]), "variance": R.rel(var, z[vn + "_variance"])}
    with pytest.warns(UserWarning, match="covariance_matrix requires converting sparse matrix to dense"):
        errs["covariance"] = R.rel(dist.covariance_matrix, z[vn + "_covariance"])
    orig = smn._standard_normal
    smn._standard_normal = lambda shape, dtype, device: eps.reshape(shape)
    try:
        errs["sample"] = R.rel(dist.rsample((7,)), z[vn + "_sample"])
    finally:
        smn._standard_normal = orig
    print(vn, iname, errs)
    assert all(e < tol for e in errs.values()), errs


# --------------------------------------------------------------------------- encoder_mvn.npz: four forms against dense float64
@pytest.mark.parametrize("batched", [False, True], ids=["unbatched", "B2"])
@pytest.mark.parametrize("itype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("vn", ["f32", "f64"])
def test_density_and_gradients_match_dense_float64(vn, form, layout, itype, batched):
    dt = torch.float32 if vn == "f32" else torch.float64
    tol = R.TOL[dt]
    o = R.operands(vn, batched, DEV)
    A = _leaf(R.as_layout(o["Lfull"] if form.endswith("llt") else o["Ls"], layout, itype))
    diag, loc, value = _leaf(o["diag"]), _leaf(o["loc"]), _leaf(o["value"][form])
    dist = R.distribution(form, A, diag, loc)
    lp, ent = dist.log_prob(value), dist.entropy()
    want_lp, want_ent, want_var, want_g = R.dense_truth(form, A, diag, loc, value)
    assert lp.shape == value.shape[:-1] and lp.dtype == dt and lp.is_cuda and ent.shape == ((2,) if batched else ())
    leaves = [A, loc, value] + ([diag] if form.endswith("ldlt") else [])
    grads = torch.autograd.grad((lp * R.weights(lp.shape, dt).to(DEV)).sum(), leaves)
    gA = grads[0]
    errs = {"log_prob": R.rel(lp, want_lp), "entropy": R.rel(ent, want_ent),
            "g_factor": R.rel_norm(R.dense64(gA), want_g["factor"]), "g_loc": R.rel_norm(grads[1], want_g["loc"]),
            "g_value": R.rel_norm(grads[2], want_g["value"])}
    if form.endswith("ldlt"):
        errs["g_diag"] = R.rel_norm(grads[3], want_g["diag"])
    if form.startswith("scale"):
        errs["variance"] = R.rel(dist.variance, want_var)
    print(vn, form, layout, itype, batched, errs)
    assert all(e < tol for e in errs.values()), errs
    # the factor's gradient: the factor's own layout, index tensors and index dtype
    assert gA.layout == A.layout and gA.shape == A.shape
    if layout == "csr":
        assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and gA.col_indices().data_ptr() == A.col_indices().data_ptr()
        assert gA.col_indices().dtype == itype
    else:
        assert gA._indices().data_ptr() == A._indices().data_ptr()      # (torch keeps COO indices in int64 whatever they were built from)


def test_variance_gradients_on_the_gpu():
    o = R.operands("f64", False, DEV)
    for ldlt in (False, True):
        A, D = _leaf(o["Ls"] if ldlt else o["Lfull"]), _leaf(o["diag"])
        dist = R.distribution("scale_ldlt" if ldlt else "scale_llt", A, D, o["loc"])
        w = torch.linspace(-1.0, 2.0, R.N, dtype=torch.float64, device=DEV)
        gA, gD = torch.autograd.grad((dist.variance * w).sum(), (A, D), allow_unused=True)
        Ld = A.detach().cpu().to_dense().requires_grad_(True)
        Dd = o["diag"].cpu().clone().requires_grad_(True)
        LI = Ld + torch.eye(R.N, dtype=torch.float64) if ldlt else Ld
        var = (LI @ torch.diag(Dd) @ LI.T).diagonal() if ldlt else (Ld @ Ld.T).diagonal()
        (var * w.cpu()).sum().backward()
        assert R.rel_norm(R.dense64(gA), Ld.grad * (Ld.detach() != 0)) < 1e-12
        if ldlt:
            assert R.rel_norm(gD, Dd.grad) < 1e-12


def test_diagonal_semantics_on_the_gpu():
    g = torch.Generator().manual_seed(3)
    n = 300
    strict = torch.tril(0.1 * torch.randn(n, n, generator=g, dtype=torch.float64), -1) * (torch.rand(n, n, generator=g) < 0.05)
    d = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    loc, x = torch.zeros(n, dtype=torch.float64, device=DEV), torch.ones(3, n, dtype=torch.float64, device=DEV)
    d_missing = d.clone()
    d_missing[17] = 0.0
    L = (strict + torch.diag(d_missing)).to_sparse_csr().to(DEV)
    prec = R.distribution("prec_llt", L, None, loc, validate_args=False)
    assert bool((prec.log_prob(x) == float("-inf")).all()) and prec.entropy() == float("inf")
    assert R.distribution("scale_llt", L, None, loc, validate_args=False).entropy() == float("-inf")
    d_neg = d.clone()
    d_neg[2] = -d_neg[2]
    Ln = (strict + torch.diag(d_neg)).to_sparse_csr().to(DEV)
    for form in ("scale_llt", "prec_llt"):
        dist = R.distribution(form, Ln, None, loc, validate_args=False)
        assert bool(dist.log_prob(x).isnan().all()) and bool(dist.entropy().isnan())
    bad = (strict + torch.diag(d)).to_sparse_csr().to(DEV)
    with pytest.raises(ValueError, match="First input should be strictly triangular"):
        R.distribution("prec_ldlt", bad, d.to(DEV), loc, validate_args=True).log_prob(x)


def test_other_value_dtypes_raise_typeerror():
    """bf16 is not offered for the density (the reductions are compiled for fp32 and fp64): TypeError before any launch."""
    o = R.operands("f32", False, DEV)
    L = torch.sparse_csr_tensor(o["Lfull"].crow_indices(), o["Lfull"].col_indices(), o["Lfull"].values().bfloat16(), (R.N, R.N))
    dist = R.distribution("scale_llt", L, None, o["loc"].bfloat16(), validate_args=False)
    for call in (lambda: dist.log_prob(torch.zeros(R.N, dtype=torch.bfloat16, device=DEV)), dist.entropy, lambda: dist.variance):
        with pytest.raises(TypeError, match="float32 and float64"):
            call()


# --------------------------------------------------------------------------- the encoder's real shape, N = 262 144
def _big(form):
    crow, col, val, D, loc, value = R.stencil_factor(form, device=DEV)
    n = loc.numel()
    A = torch.sparse_csr_tensor(crow, col, val, (n, n))
    return crow, col, val, D, loc, value, A


@pytest.mark.parametrize("form", R.FORMS)
def test_encoder_shape_float32_against_float64_sparse_truth(form):
    """float32 on the GPU against the float64 closed forms of `_mvn_ref.sparse_truth` (torch's CPU sparse solve / products)."""
    crow, col, val, D, loc, value, A = _big(form)
    A, Dl, locl, valuel = _leaf(A), _leaf(D), _leaf(loc), _leaf(value)
    dist = R.distribution(form, A, Dl, locl, validate_args=False)
    w = R.weights((8,), torch.float32).to(DEV)
    lp, ent = dist.log_prob(valuel), dist.entropy()
    leaves = [A, valuel, locl] + ([Dl] if form.endswith("ldlt") else [])
    grads = torch.autograd.grad((lp * w).sum(), leaves)
    want_lp, want_ent, want_g = R.sparse_truth(form, crow, col, val, D, loc, value, w)
    gA = grads[0]
    errs = {"log_prob": R.rel(lp, want_lp), "entropy": R.rel(ent, want_ent),
            "g_factor": R.rel_norm(gA.values(), want_g["factor"]), "g_value": R.rel_norm(grads[1], want_g["value"]),
            "g_loc": R.rel_norm(grads[2], -want_g["value"].sum(0))}
    if form.endswith("ldlt"):
        errs["g_diag"] = R.rel_norm(grads[3], want_g["diag"])
    print(form, errs)
    assert all(e < 1e-5 for e in errs.values()), errs
    assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and gA.col_indices().dtype == torch.int32


@pytest.mark.parametrize("form", R.FORMS)
def test_nothing_densifies_at_the_encoder_shape(form):
    """Peak allocation of log_prob + backward after one warm-up call (plans, transposed pattern, work areas are cached by then),
    measured as test_rsample_sequence_makes_no_device_copies_of_the_noise does: below 8 x (bytes of the factor's values and indices
    + bytes of value), about 0.3 GB — the dense factor alone would be 275 GB."""
    crow, col, val, D, loc, value, A = _big(form)
    A, Dl, locl, valuel = _leaf(A), _leaf(D), _leaf(loc), _leaf(value)
    dist = R.distribution(form, A, Dl, locl, validate_args=False)
    leaves = [A, valuel, locl] + ([Dl] if form.endswith("ldlt") else [])

    def step():
        return torch.autograd.grad(dist.log_prob(valuel).sum(), leaves)

    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    grads = step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    bound = 8 * (val.numel() * 4 + col.numel() * 4 + crow.numel() * 4 + value.numel() * 4)
    print(form, "peak extra bytes", extra, "bound", bound)
    assert extra < bound, (form, extra, bound)
    assert all(bool(torch.isfinite(g.values() if g.is_sparse_csr else g).all()) for g in grads)


@pytest.mark.parametrize("form", R.FORMS)
def test_two_calls_give_the_same_bits(form):
    from torchsparsegradutils_amd import wait_for_plans

    crow, col, val, D, loc, value, A = _big(form)
    A, Dl, locl, valuel = _leaf(A), _leaf(D), _leaf(loc), _leaf(value)
    dist = R.distribution(form, A, Dl, locl, validate_args=False)
    w = R.weights((8,), torch.float32).to(DEV)
    leaves = [A, valuel, locl] + ([Dl] if form.endswith("ldlt") else [])

    def step():
        lp, ent = dist.log_prob(valuel), dist.entropy()
        gs = torch.autograd.grad((lp * w).sum() + ent, leaves)
        return [lp, ent] + [g.values() if g.is_sparse_csr else g for g in gs]

    for _ in range(4):                 # (the pattern's plans and launch widths settle during its first calls)
        step()
        wait_for_plans()
    first, second = step(), step()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_entropy_and_log_determinant_kernels_capture_into_a_graph():
    for form in ("scale_llt", "prec_ldlt"):
        crow, col, val, D, loc, value, A = _big(form)
        dist = R.distribution(form, A, D, loc, validate_args=False)
        want = dist.entropy()                       # warm-up: the diagonal positions are cached with the pattern
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = dist.entropy()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), form


def test_rsample_is_unchanged_by_a_log_prob_call():
    o = R.operands("f32", False, DEV)
    z = G.load("encoder_mvn.npz")
    eps = G.t(z["f32_eps"], DEV)
    for form in R.FORMS:
        dist = R.distribution(form, o["Lfull"] if form.endswith("llt") else o["Ls"], o["diag"], o["loc"])
        before = dist._transform(eps)
        assert R.rel(before, z[f"f32_{form}_x"]) < 1e-5
        dist.log_prob(o["value"][form])
        assert torch.equal(dist._transform(eps), before)
