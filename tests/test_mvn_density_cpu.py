"""The sparse multivariate normal's density on CPU operands (the torch-op twins of csrc/mvn.hip in _cpu.py; the same autograd
functions, plans and shape handling as the GPU path): `log_prob`, `entropy`, `variance` of `SparseMultivariateNormal` for all four
parameterisations and `SparseMultivariateNormalNative` against the reference's golden vectors
(tests/golden/make_golden_mvn.py).  No GPU needed."""

import json
import os
import warnings

import pytest
import torch

import _golden as G
import _mvn_ref as R


def _leaf(A):
    return A.detach().requires_grad_(True)


# --------------------------------------------------------------------------- SparseMultivariateNormalNative against the reference
@pytest.mark.parametrize("iname", ["i32", "i64"])
@pytest.mark.parametrize("vn", ["f32", "f64"])
def test_native_matches_the_reference_golden(vn, iname):
    import torchsparsegradutils_amd.distributions.sparse_multivariate_normal as smn
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormalNative

    z = G.load("mvn_native.npz")
    dt = torch.float32 if vn == "f32" else torch.float64
    tol = R.TOL[dt]
    L = torch.sparse_csr_tensor(G.t(z[f"{vn}_{iname}_crow"]), G.t(z[f"{vn}_{iname}_col"]), G.t(z[vn + "_val"]), (96, 96))
    loc, x, eps = G.t(z[vn + "_loc"]), G.t(z[vn + "_x"]), G.t(z[vn + "_eps"])
    dist = SparseMultivariateNormalNative(loc, L)
    assert dist.batch_shape == () and dist.event_shape == (96,) and dist.has_rsample
    assert dist.mean is loc and dist.mode is loc and dist.scale_tril is L
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # nothing densifies: none of the reference's memory warnings
        lp1, lp7, var = dist.log_prob(x[0]), dist.log_prob(x), dist.variance
    assert lp1.shape == () and lp7.shape == (7,) and var.shape == (96,) and lp7.dtype == dt
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
    assert dist.rsample().shape == (96,) and dist.rsample((2, 3)).shape == (2, 3, 96)


def test_native_constructor_errors_verbatim():
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormalNative

    with open(os.path.join(G.GOLDEN, "mvn_native_errors.json")) as f:
        want = json.load(f)
    loc, L = torch.zeros(4), torch.eye(4).to_sparse_csr()
    cases = {
        "loc_not_1d": lambda: SparseMultivariateNormalNative(torch.zeros(2, 4), L),
        "not_csr": lambda: SparseMultivariateNormalNative(loc, torch.eye(4).to_sparse_coo()),
        "batched": lambda: SparseMultivariateNormalNative(loc, torch.stack([torch.eye(4)] * 2).to_sparse_csr()),
        "not_square": lambda: SparseMultivariateNormalNative(loc, torch.ones(4, 5).to_sparse_csr()),
        "size_mismatch": lambda: SparseMultivariateNormalNative(torch.zeros(5), L),
    }
    assert set(cases) == set(want)
    for name, fn in cases.items():
        with pytest.raises(Exception) as info:
            fn()
        assert type(info.value).__name__ == want[name]["type"] and str(info.value) == want[name]["message"], name


def test_distributions_module_exports_both_names():
    import torchsparsegradutils_amd.distributions as d

    assert sorted(d.__all__) == ["SparseMultivariateNormal", "SparseMultivariateNormalNative"]


# --------------------------------------------------------------------------- the four parameterisations against dense float64
@pytest.mark.parametrize("batched", [False, True], ids=["unbatched", "B2"])
@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("vn", ["f32", "f64"])
def test_density_and_gradients_match_dense_float64(vn, form, layout, batched):
    dt = torch.float32 if vn == "f32" else torch.float64
    tol = R.TOL[dt]
    o = R.operands(vn, batched)
    A = _leaf(R.as_layout(o["Lfull"] if form.endswith("llt") else o["Ls"], layout, torch.int64))
    diag, loc, value = _leaf(o["diag"]), _leaf(o["loc"]), _leaf(o["value"][form])
    dist = R.distribution(form, A, diag, loc)
    lp, ent = dist.log_prob(value), dist.entropy()
    want_lp, want_ent, want_var, want_g = R.dense_truth(form, A, diag, loc, value)
    assert lp.shape == value.shape[:-1] and lp.dtype == dt and ent.shape == dist.batch_shape == ((2,) if batched else ())
    leaves = [A, loc, value] + ([diag] if form.endswith("ldlt") else [])
    grads = torch.autograd.grad((lp * R.weights(lp.shape, dt)).sum(), leaves)
    gA = grads[0]
    errs = {"log_prob": R.rel(lp, want_lp), "entropy": R.rel(ent, want_ent),
            "g_factor": R.rel_norm(R.dense64(gA), want_g["factor"]), "g_loc": R.rel_norm(grads[1], want_g["loc"]),
            "g_value": R.rel_norm(grads[2], want_g["value"])}
    if form.endswith("ldlt"):
        errs["g_diag"] = R.rel_norm(grads[3], want_g["diag"])
    if form.startswith("scale"):
        var = dist.variance
        assert var.shape == loc.shape
        errs["variance"] = R.rel(var, want_var)
        assert R.rel(dist.stddev, want_var.sqrt()) < tol
    else:
        with pytest.raises(NotImplementedError, match="not a sparse operation"):
            dist.variance
    print(vn, form, layout, batched, errs)
    assert all(e < tol for e in errs.values()), errs
    # the factor's gradient: the factor's own layout, index tensors and index dtype
    assert gA.layout == A.layout and gA.shape == A.shape
    if layout == "csr":
        assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr()
        assert gA.col_indices().data_ptr() == A.col_indices().data_ptr()
    else:
        assert gA._indices().data_ptr() == A._indices().data_ptr()


@pytest.mark.parametrize("form", ["scale_llt", "prec_ldlt"])
def test_int32_csr_factor_keeps_int32_in_its_gradient(form):
    o = R.operands("f64", False)
    A = _leaf(R.as_layout(o["Lfull"] if form.endswith("llt") else o["Ls"], "csr", torch.int32))
    dist = R.distribution(form, A, o["diag"], o["loc"])
    lp = dist.log_prob(o["value"][form])
    (gA,) = torch.autograd.grad(lp.sum(), (A,))
    want_lp, _, _, want_g = R.dense_truth(form, A, o["diag"], o["loc"], o["value"][form], w=torch.ones(7))
    assert R.rel(lp, want_lp) < 1e-12 and R.rel_norm(R.dense64(gA), want_g["factor"]) < 1e-12
    assert gA.crow_indices().dtype == torch.int32 and gA.col_indices().dtype == torch.int32
    assert gA.col_indices().data_ptr() == A.col_indices().data_ptr()


def test_variance_gradients_match_dense_float64():
    o = R.operands("f64", False)
    for ldlt in (False, True):
        A = _leaf(o["Ls"] if ldlt else o["Lfull"])
        D = _leaf(o["diag"])
        dist = R.distribution("scale_ldlt" if ldlt else "scale_llt", A, D, o["loc"])
        w = torch.linspace(-1.0, 2.0, R.N, dtype=torch.float64)
        gA, gD = torch.autograd.grad((dist.variance * w).sum(), (A, D), allow_unused=True)
        Ld = A.detach().to_dense().requires_grad_(True)
        Dd = o["diag"].clone().requires_grad_(True)
        if ldlt:
            LI = Ld + torch.eye(R.N, dtype=torch.float64)
            var = (LI @ torch.diag(Dd) @ LI.T).diagonal()
        else:
            var = (Ld @ Ld.T).diagonal()
        (var * w).sum().backward()
        assert R.rel_norm(R.dense64(gA), Ld.grad * (A.detach().to_dense() != 0)) < 1e-12
        if ldlt:
            assert R.rel_norm(gD, Dd.grad) < 1e-12


# --------------------------------------------------------------------------- shapes and validation
def test_value_shapes():
    o = R.operands("f64", False)
    ob = R.operands("f64", True)
    x = o["value"]["prec_ldlt"]                      # (7, 240)
    xb = ob["value"]["prec_ldlt"]                    # (5, 2, 240)
    for form in R.FORMS:
        dist = R.distribution(form, o["Lfull"] if form.endswith("llt") else o["Ls"], o["diag"], o["loc"])
        full = dist.log_prob(x)
        assert full.shape == (7,)
        assert dist.log_prob(x[0]).shape == () and torch.allclose(dist.log_prob(x[0]), full[0], rtol=1e-13, atol=0)
        two = dist.log_prob(x[:6].reshape(2, 3, R.N))                # a two-dimensional sample shape
        assert two.shape == (2, 3) and torch.allclose(two.reshape(6), full[:6], rtol=1e-13, atol=0)
        distb = R.distribution(form, ob["Lfull"] if form.endswith("llt") else ob["Ls"], ob["diag"], ob["loc"])
        fullb = distb.log_prob(xb)
        assert fullb.shape == (5, 2) and distb.entropy().shape == (2,)
        assert distb.log_prob(xb[0]).shape == (2,) and torch.allclose(distb.log_prob(xb[0]), fullb[0], rtol=1e-13, atol=0)
        twob = distb.log_prob(xb[:4].reshape(2, 2, 2, R.N))
        assert twob.shape == (2, 2, 2) and torch.allclose(twob.reshape(4, 2), fullb[:4], rtol=1e-13, atol=0)
        # item b of the batch is the unbatched distribution of item b's parameters
        if form == "prec_ldlt":
            Lb0 = ob["Ls"].to_dense()[1].to_sparse_csr()
            single = R.distribution(form, Lb0, ob["diag"][1], ob["loc"][1])
            assert torch.allclose(single.log_prob(xb[:, 1]), fullb[:, 1], rtol=1e-12, atol=0)


def test_validate_args_rejects_a_wrong_event_size():
    o = R.operands("f64", False)
    dist = R.distribution("scale_llt", o["Lfull"], None, o["loc"], validate_args=True)
    with pytest.raises(ValueError):
        dist.log_prob(torch.zeros(7, R.N - 1, dtype=torch.float64))
    assert dist.log_prob(torch.zeros(7, R.N, dtype=torch.float64)).shape == (7,)


def test_other_value_dtypes_raise_typeerror():
    o = R.operands("f32", False)
    L = torch.sparse_csr_tensor(o["Lfull"].crow_indices(), o["Lfull"].col_indices(), o["Lfull"].values().bfloat16(), (R.N, R.N))
    dist = R.distribution("scale_llt", L, None, o["loc"].bfloat16(), validate_args=False)
    for call in (lambda: dist.log_prob(torch.zeros(R.N, dtype=torch.bfloat16)), dist.entropy, lambda: dist.variance):
        with pytest.raises(TypeError, match="float32 and float64"):
            call()


# --------------------------------------------------------------------------- diagonal semantics
def _small_lower(n=12, seed=3):
    g = torch.Generator().manual_seed(seed)
    dense = torch.tril(0.3 * torch.randn(n, n, generator=g, dtype=torch.float64), -1)
    dense = dense * (torch.rand(n, n, generator=g) < 0.5)
    return dense, 1.0 + torch.rand(n, generator=g, dtype=torch.float64)


def test_missing_and_negative_diagonal_follow_the_dense_formula():
    strict, d = _small_lower()
    n = strict.size(0)
    loc, x = torch.zeros(n, dtype=torch.float64), torch.ones(3, n, dtype=torch.float64)
    # row 5 stores no diagonal entry: log 0 = -inf in the log-determinant, as L.to_dense().diagonal().log().sum()
    d_missing = d.clone()
    d_missing[5] = 0.0
    L = (strict + torch.diag(d_missing)).to_sparse_csr()
    assert L.values().numel() == int((strict != 0).sum()) + n - 1
    assert L.to_dense().diagonal().log().sum() == float("-inf")
    prec = R.distribution("prec_llt", L, None, loc, validate_args=False)
    assert bool((prec.log_prob(x) == float("-inf")).all()) and prec.entropy() == float("inf")       # Σ^-1 singular: −½ logdet Σ = −inf
    scale = R.distribution("scale_llt", L, None, loc, validate_args=False)
    assert scale.entropy() == float("-inf")
    # a negative stored diagonal: NaN, no exception
    d_neg = d.clone()
    d_neg[2] = -d_neg[2]
    Ln = (strict + torch.diag(d_neg)).to_sparse_csr()
    for form in ("scale_llt", "prec_llt"):
        dist = R.distribution(form, Ln, None, loc, validate_args=False)
        assert bool(dist.log_prob(x).isnan().all()) and bool(dist.entropy().isnan())
    # COO and the batched block-diagonal plan find the same positions
    Lb = torch.stack([(strict + torch.diag(d)), (strict + torch.diag(d_missing))]).to_sparse_coo()
    ent = R.distribution("scale_llt", Lb, None, torch.zeros(2, n, dtype=torch.float64), validate_args=False).entropy()
    assert ent.shape == (2,) and bool(ent[0].isfinite()) and ent[1] == float("-inf")


def test_ldlt_factor_with_a_stored_diagonal_is_rejected_under_validate_args():
    strict, d = _small_lower()
    n = strict.size(0)
    loc, x = torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    D = 0.5 + d
    bad = (strict + torch.diag(d)).to_sparse_csr()
    msg = "First input should be strictly triangular"
    for form in ("scale_ldlt", "prec_ldlt"):
        dist = R.distribution(form, bad, D, loc, validate_args=True)
        with pytest.raises(ValueError, match=msg):
            dist.log_prob(x)
        with pytest.raises(ValueError, match=msg):
            dist.entropy()
        ok = R.distribution(form, strict.to_sparse_csr(), D, loc, validate_args=True)
        assert bool(ok.log_prob(x).isfinite())


# --------------------------------------------------------------------------- gradcheck
@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("form", R.FORMS)
def test_gradcheck_float64_on_a_12_row_factor(form, layout):
    strict, d = _small_lower()
    n = strict.size(0)
    dense = strict + (torch.diag(d) if form.endswith("llt") else 0)
    A = dense.to_sparse_csr()
    crow, col = A.crow_indices(), A.col_indices()
    coo = A.to_sparse_coo().coalesce().indices()
    g = torch.Generator().manual_seed(11)
    vals = A.values().clone().requires_grad_(True)
    D = (0.5 + torch.rand(n, generator=g, dtype=torch.float64)).requires_grad_(True)
    loc = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(3, n, generator=g, dtype=torch.float64).requires_grad_(True)

    def fn(vals, D, loc, x):
        if layout == "csr":
            F = torch.sparse_csr_tensor(crow, col, vals, (n, n))
        else:
            F = torch.sparse_coo_tensor(coo, vals, (n, n), is_coalesced=True)
        dist = R.distribution(form, F, D, loc, validate_args=False)
        out = [dist.log_prob(x), dist.entropy()]
        if form.startswith("scale"):
            out.append(dist.variance)
        return tuple(out)

    assert torch.autograd.gradcheck(fn, (vals, D, loc, x), eps=1e-6, atol=1e-7, rtol=1e-6)
