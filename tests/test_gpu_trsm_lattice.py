"""The line-sweep triangular solve (csrc/sptrsm_lattice.hip) on the GPU.  Needs an MI355X: `pytest -m gpu`.

The kernel sums every row in the order and lane geometry of the sync-free sweep, so its contract is BIT identity: every case solves
once with the family on and once with it off (`sparse_solve.ENABLE_TRSM_LATTICE`) and compares integer bit patterns (NaN and inf
count).  Every case also records which `_backend` entry ran, so that a geometry that silently falls back fails.  Accuracy at full
size uses the componentwise bound of tests/test_gpu_round5.py (same formula, same constants)."""

import numpy as np
import pytest
import torch

import _golden as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS32 = float(np.finfo(np.float32).eps)
SHAPE = (16, 20, 24)          # 7 680 rows; every factor below has nnz >= PACK_MIN_NNZ


@pytest.fixture(scope="module", autouse=True)
def _need_gpu_and_extension():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield
    _backend.poll_errors(block=True)


@pytest.fixture(autouse=True)
def _fresh_pattern_cache():
    """Every case meets its pattern at first sight (lower and upper halves share a geometry: the cache would otherwise count them
    as one geometry that keeps arriving with new content and postpone their plans)."""
    from torchsparsegradutils_amd import _pattern

    _pattern.clear_cache()
    yield


@pytest.fixture
def ran(monkeypatch):
    """List of the solve entries of `_backend` in launch order: "lattice" / "syncfree"."""
    from torchsparsegradutils_amd import _backend as be

    log = []
    for fn, tag in (("csr_sptrsm_lattice", "lattice"), ("csr_sptrsm", "syncfree")):
        orig = getattr(be, fn)

        def wrapped(*args, _orig=orig, _tag=tag, **kw):
            log.append(_tag)
            return _orig(*args, **kw)

        monkeypatch.setattr(be, fn, wrapped)
    return log


def _switch(monkeypatch, on):
    import torchsparsegradutils_amd.sparse_solve as ss

    monkeypatch.setattr(ss, "ENABLE_TRSM_LATTICE", on)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _pattern(part, shape=SHAPE, points=27, periodic=False, itype=torch.int32):
    from torchsparsegradutils_amd import _ops
    from torchsparsegradutils_amd.utils import synthetic

    crow, col = synthetic.box_stencil(*shape, periodic=(periodic,) * 3, points=points, part=part, index_dtype=itype, device=DEV)
    assert col.numel() >= _ops.PACK_MIN_NNZ
    return crow, col


def _values(crow, col, dtype, seed=0):
    """Values as tools/mvnbench.py makes them: small off the diagonal, 1 … 2 on it."""
    n = crow.numel() - 1
    g = torch.Generator(device=DEV).manual_seed(seed)
    val = 0.03 * torch.randn(col.numel(), device=DEV, generator=g, dtype=dtype)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (crow[1:] - crow[:-1]).long())
    on_diag = col.long() == rows
    val[on_diag] = 1.0 + torch.rand(int(on_diag.sum()), device=DEV, generator=g, dtype=dtype)
    return val


def _rhs(n, p, dtype, seed=1, batch=None):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(((batch,) if batch else ()) + (n, p), device=DEV, generator=g, dtype=dtype)


def _on_off(monkeypatch, ran, fn, want_on="lattice"):
    """fn() with the family on, then off: (result on, result off); asserts which kernels ran."""
    from torchsparsegradutils_amd import wait_for_plans

    _switch(monkeypatch, True)
    del ran[:]
    on = fn()
    wait_for_plans()
    assert ran and set(ran) == {want_on}, ran
    n_on = len(ran)
    _switch(monkeypatch, False)
    del ran[:]
    off = fn()
    assert ran == ["syncfree"] * n_on, ran
    return on, off


FLAGS = [(u, t, unit) for u in (False, True) for t in (False, True) for unit in (False, True)]


@pytest.mark.parametrize("upper,transpose,unit", FLAGS)
@pytest.mark.parametrize("p", [1, 3, 8, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bit_identity_csr_int32(dtype, p, upper, transpose, unit, monkeypatch, ran):
    from torchsparsegradutils_amd import sparse_triangular_solve

    part = ("strict_" if unit else "") + ("upper" if upper else "lower")
    crow, col = _pattern(part)
    n = crow.numel() - 1
    A = torch.sparse_csr_tensor(crow, col, _values(crow, col, dtype), (n, n))
    B = _rhs(n, p, dtype)
    on, off = _on_off(monkeypatch, ran, lambda: sparse_triangular_solve(A, B, upper=upper, unitriangular=unit, transpose=transpose))
    assert torch.equal(_bits(on), _bits(off))
    assert bool(torch.isfinite(on).all())


_SOME_FLAGS = [(False, False, False), (False, True, True), (True, False, True), (True, True, False)]
VARIANTS = [(v,) + f for v in ("csr_i64", "coo", "batched_csr", "batched_coo", "tview", "seven_point", "flat") for f in _SOME_FLAGS] \
    + [("whole_box", u, t, False) for u in (False, True) for t in (False, True)]      # (a whole box stores its diagonal: no unit cases)


@pytest.mark.parametrize("variant,upper,transpose,unit", VARIANTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_bit_identity_layouts_index_types_batches_and_views(dtype, variant, upper, transpose, unit, monkeypatch, ran):
    from torchsparsegradutils_amd import sparse_triangular_solve

    part = ("strict_" if unit else "") + ("upper" if upper else "lower")
    points = 27
    if variant == "whole_box":
        part = None
    if variant == "seven_point":
        points = 7
    shape = (28, 32, 32) if variant == "seven_point" else SHAPE
    if variant == "flat":
        shape = (140, 130, 5)      # 18 200 short lines: a ticket of the sweep is a group of two lines
    crow, col = _pattern(part, shape=shape, points=points, itype=torch.int64 if variant == "csr_i64" else torch.int32)
    n = crow.numel() - 1
    val = _values(crow, col, dtype)
    # (three items: the lattice detector samples rows around the middle of the matrix, and with two items of a TRIANGULAR factor it
    # meets the item boundary there — rows without an x-neighbour — and finds no lattice; such a batch stays on the sync-free kernel)
    batch = 3 if variant.startswith("batched") else None
    p = 8
    if batch:
        vals = torch.stack((val, _values(crow, col, dtype, seed=5), _values(crow, col, dtype, seed=6)))
        A = torch.sparse_csr_tensor(crow.repeat(batch, 1), col.repeat(batch, 1), vals, (batch, n, n))
        if variant == "batched_coo":
            A = A.to_sparse_coo().coalesce()
    else:
        A = torch.sparse_csr_tensor(crow, col, val, (n, n))
        if variant == "coo":
            A = A.to_sparse_coo().coalesce()
    B = _rhs(n, p, dtype, batch=batch)
    if variant == "tview":
        B = _rhs(p, n, dtype).t()          # unit row stride: consumed in place
        assert not B.is_contiguous()
    on, off = _on_off(monkeypatch, ran, lambda: sparse_triangular_solve(A, B, upper=upper, unitriangular=unit, transpose=transpose))
    assert on.shape == B.shape and torch.equal(_bits(on), _bits(off))


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_zero_diagonal_entry_and_empty_row_give_the_same_inf_and_nan_bits(dtype, transpose, monkeypatch, ran):
    from torchsparsegradutils_amd import sparse_triangular_solve

    crow, col = _pattern("lower")
    n = crow.numel() - 1
    val = _values(crow, col, dtype)
    # one factor with a stored zero on the diagonal …
    vz = val.clone()
    r = n // 2 + 7
    vz[int(crow[r + 1]) - 1] = 0.0           # (sorted columns: a lower row ends with its diagonal)
    Az = torch.sparse_csr_tensor(crow, col, vz, (n, n))
    # … and one with an empty row
    r2 = n // 3
    s, e = int(crow[r2]), int(crow[r2 + 1])
    keep = torch.ones(col.numel(), dtype=torch.bool, device=DEV)
    keep[s:e] = False
    crow2 = crow.clone()
    crow2[r2 + 1:] -= e - s
    Ae = torch.sparse_csr_tensor(crow2, col[keep].contiguous(), val[keep].contiguous(), (n, n))
    B = _rhs(n, 8, dtype)
    for A in (Az, Ae):
        on, off = _on_off(monkeypatch, ran, lambda: sparse_triangular_solve(A, B, upper=False, transpose=transpose))
        assert torch.equal(_bits(on), _bits(off))
        assert not bool(torch.isfinite(on).all()), "the zero pivot must show"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_autograd_forward_and_adjoint_run_on_the_lattice_kernel(dtype, monkeypatch, ran):
    from torchsparsegradutils_amd import sparse_triangular_solve

    crow, col = _pattern("lower")
    n = crow.numel() - 1
    val = _values(crow, col, dtype)
    B0 = _rhs(n, 8, dtype)
    Gr = _rhs(n, 8, dtype, seed=9)

    def step():
        A = torch.sparse_csr_tensor(crow, col, val, (n, n)).requires_grad_(True)
        B = B0.clone().requires_grad_(True)
        x = sparse_triangular_solve(A, B, upper=False)
        gA, gB = torch.autograd.grad(x, (A, B), Gr)
        return x.detach(), gA.values().detach(), gB

    on, off = _on_off(monkeypatch, ran, step)        # two solves each: the forward and the adjoint
    for a, b in zip(on, off):
        assert torch.equal(_bits(a), _bits(b))


def _encoder_factor(dtype, diag, seed=0):
    from torchsparsegradutils_amd import _ops
    from torchsparsegradutils_amd.encoders import PairwiseEncoder

    shape = (1,) + SHAPE
    enc = PairwiseEncoder(1.75, shape, diag=diag, upper=False, layout=torch.sparse_csr, indices_dtype=torch.int32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = 0.03 * torch.randn((len(enc.offsets),) + shape, device=DEV, generator=g, dtype=dtype)
    if diag:
        w[0] = 1.0 + torch.rand(shape, device=DEV, generator=g, dtype=dtype)
    A = enc(w)
    assert A.values().numel() >= _ops.PACK_MIN_NNZ
    return A, SHAPE[0] * SHAPE[1] * SHAPE[2]


@pytest.mark.parametrize("form", ["scale_llt", "scale_ldlt", "prec_llt", "prec_ldlt"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_the_distribution_on_an_encoder_lattice(dtype, form, monkeypatch, ran):
    """`log_prob` of the covariance forms (LLᵀ, LDLᵀ) and `rsample` of the precision forms solve with the encoder's factor."""
    import torchsparsegradutils_amd.distributions.sparse_multivariate_normal as smn
    from torchsparsegradutils_amd.distributions import SparseMultivariateNormal

    ldlt, covariance = form.endswith("ldlt"), form.startswith("scale")
    A, n = _encoder_factor(dtype, diag=not ldlt)
    g = torch.Generator(device=DEV).manual_seed(2)
    loc = torch.randn(n, device=DEV, generator=g, dtype=dtype)
    kw = {"scale_tril" if covariance else "precision_tril": A}
    if ldlt:
        kw["diagonal"] = 0.5 + torch.rand(n, device=DEV, generator=g, dtype=dtype)
    dist = SparseMultivariateNormal(loc, validate_args=False, **kw)
    if covariance:
        value = loc + 1.5 * torch.randn(8, n, device=DEV, generator=g, dtype=dtype)
        on, off = _on_off(monkeypatch, ran, lambda: dist.log_prob(value))
    else:
        eps = torch.randn(8, n, device=DEV, generator=g, dtype=dtype)
        monkeypatch.setattr(smn, "_standard_normal", lambda shape, dtype, device: eps.reshape(shape))
        on, off = _on_off(monkeypatch, ran, lambda: dist.rsample((8,)))
    assert torch.equal(_bits(on), _bits(off)) and bool(torch.isfinite(on).all())


def test_full_size_every_element_within_the_componentwise_bound(monkeypatch, ran):
    """The 64³ truncated 27-point lower factor (N = 262 144), 8 columns, fp32: EVERY element within the componentwise
    forward-substitution bound (n_r + 4)·eps·[M(T)⁻¹|T||x|] of the fp64 solution, and rel_err < 1e-5 — the formula and constants of
    tests/test_gpu_round5.py::test_c3_full_size_every_element_within_the_componentwise_bound."""
    from oracle import oracle
    from torchsparsegradutils_amd import sparse_triangular_solve

    _switch(monkeypatch, True)
    n, p = 64 ** 3, 8
    crow, col = _pattern("lower", shape=(64, 64, 64))
    val = _values(crow, col, torch.float32)
    B = _rhs(n, p, torch.float32, seed=3)
    A = torch.sparse_csr_tensor(crow, col, val, (n, n))
    x = sparse_triangular_solve(A, B, upper=False).cpu().numpy().astype(np.float64)
    assert ran == ["lattice"], ran
    cn, on = crow.cpu().numpy(), col.cpu().numpy()
    v64 = val.cpu().numpy().astype(np.float64)
    x64 = oracle.csr_sptrsm(cn, on, v64, B.cpu().numpy().astype(np.float64), upper=False)
    rows = oracle.expand_rows(cn)
    absT = np.abs(v64)
    rhs = oracle.csr_spmm(cn, on, absT, np.abs(x64))                         # |T||x|
    comp = np.where(rows == on, absT, -absT)                                # M(T): |diagonal|, −|off-diagonal|
    bound = oracle.csr_sptrsm(cn, on, comp, rhs, upper=False)
    longest = int(np.diff(cn).max())
    worst = float((np.abs(x - x64) / ((longest + 4) * EPS32 * bound + 1e-300)).max())
    print("worst componentwise ratio", worst, "rel_err", G.rel_err(x, x64))
    assert worst <= 1.0, worst
    assert G.rel_err(x, x64) < 1e-5


@pytest.mark.parametrize("case", ["periodic", "banded", "bf16", "p128", "switch_off", "master_switch_off"])
def test_what_the_line_sweep_does_not_cover_stays_on_the_sync_free_kernel(case, monkeypatch, ran):
    from torchsparsegradutils_amd import _ops, sparse_triangular_solve
    from torchsparsegradutils_amd.utils import synthetic

    dtype, p = torch.float32, 8
    if case == "banded":
        crow, col, val = synthetic.banded_lower(16384, per_row=8, band=512, device=DEV)
        assert col.numel() >= _ops.PACK_MIN_NNZ
    else:
        if case == "periodic":
            # tril of the periodic box: the used entries of the face rows wrap around the lattice
            crow, col = _pattern(None, periodic=True)
            n = crow.numel() - 1
            rows = torch.repeat_interleave(torch.arange(n, device=DEV), (crow[1:] - crow[:-1]).long())
            keep = col.long() <= rows
            crow = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
            crow[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
            col = col[keep].contiguous()
            assert col.numel() >= _ops.PACK_MIN_NNZ
        else:
            crow, col = _pattern("lower")
        val = _values(crow, col, torch.float32)
    if case == "bf16":
        dtype = torch.bfloat16
    if case == "p128":
        p = 128
    n = crow.numel() - 1
    A = torch.sparse_csr_tensor(crow, col, val.to(dtype), (n, n))
    B = _rhs(n, p, torch.float32).to(dtype)
    _switch(monkeypatch, False)
    want = sparse_triangular_solve(A, B, upper=False)
    assert ran == ["syncfree"]
    del ran[:]
    _switch(monkeypatch, case != "switch_off")
    if case == "master_switch_off":
        monkeypatch.setattr(_ops, "ENABLE_LATTICE", False)
    got = sparse_triangular_solve(A, B, upper=False)
    assert ran == ["syncfree"], ran
    assert torch.equal(got.view(torch.int16) if dtype == torch.bfloat16 else _bits(got),
                       want.view(torch.int16) if dtype == torch.bfloat16 else _bits(want))


def test_a_captured_solve_replays_the_same_bits(monkeypatch, ran):
    """One linear chain (fill kernel, sweep) captured after the plan exists."""
    from torchsparsegradutils_amd import sparse_triangular_solve, wait_for_plans

    _switch(monkeypatch, True)
    crow, col = _pattern("lower")
    n = crow.numel() - 1
    A = torch.sparse_csr_tensor(crow, col, _values(crow, col, torch.float32), (n, n))
    B = _rhs(n, 8, torch.float32)
    eager = sparse_triangular_solve(A, B, upper=False).clone()
    wait_for_plans()
    assert ran == ["lattice"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = sparse_triangular_solve(A, B, upper=False)
    torch.cuda.current_stream().wait_stream(side)
    assert ran == ["lattice", "lattice"]
    B2 = _rhs(n, 8, torch.float32, seed=11)
    for rhs_now in (B.clone(), B2):
        B.copy_(rhs_now)
        graph.replay()
        torch.cuda.synchronize()
        want = sparse_triangular_solve(A, rhs_now, upper=False)
        assert torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(eager), _bits(sparse_triangular_solve(A, B.copy_(_rhs(n, 8, torch.float32)), upper=False)))
