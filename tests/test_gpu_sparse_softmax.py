"""sparse_softmax / sparse_log_softmax on the GPU against torch.sparse.softmax / log_softmax in float64 on the CPU.

The structural cases are those of the log-sum-exp kernels (tests/_lse_cases.py): the softmax kernels cut the entries the same
way, so the same row pointers reach every branch of the range / lane / wave / merge / fix-up logic.  Each case runs as CSR rows
(the pattern's own direction) and, stored as CSC, as rows through the cached transpose and its `perm`.

Bounds (derived, not measured; u = unit roundoff of the accumulator, 2^-24 for float32 and bfloat16, 2^-53 for float64, L = the
group's length, m its maximum, `tiny` the accumulator's smallest normal number — what an underflowing exp loses):
  softmax     |y - y64| <= (L + |v - m| + 8) u y64 + tiny        (v - m rounds once: |v - m| u in the exponent; the sum of L
                                                                  positive terms: L u; exp, the division, the oracle: a few u)
  log form    |y - y64| <= (L + 8) u max(1, |y64|) + u |v|
  gradient    |d - d64| <= (L + |v - m| + 16) u (|g_k| y_k + y_k sum_j |g_j| y_j) + tiny (|g_k| + sum_j |g_j|)
  log form    |d - d64| <= (L + |y_k| + 16) u (|g_k| + exp(y_k) sum_j |g_j|) + 2^-53 |v_k - y_k| exp(y_k) sum_j |g_j|
              (|y_k| = |v - m| + log s takes the place of |v - m|: it is the exponent exp() is taken of.  The last term is the
              oracle's own error: torch forms y as v - (m + log s), so its float64 y is off by up to 2^-53 |m + log s| =
              2^-53 |v_k - y_k| — the u |v| term of the value bound — and its backward multiplies that by exp(y_k) |sum_j g_j|.
              It matters for the float64 kernels only, which form (v - m) - log s and are closer to the exact value.)
bfloat16 results are the float32 path's results rounded once (bit for bit), hence within half a bfloat16 ulp (2^-8 relative)
of the oracle beyond the float32 bound.

The oracle is called with non-negative dims: the backward of torch.sparse.softmax on this torch reduces over nothing when it
is handed a negative dim (every entry its own group), which a dense computation contradicts.
"""

import functools

import numpy as np
import pytest
import torch

import _lse_cases as lc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH_DTYPE = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53, "bfloat16": 2.0 ** -24}
TINY = {"float32": float(np.finfo(np.float32).tiny), "float64": float(np.finfo(np.float64).tiny),
        "bfloat16": float(np.finfo(np.float32).tiny)}
U_BF16 = 2.0 ** -8          # unit roundoff of the bfloat16 storage format (8 significant bits)
CASE_NAMES = [c[0] for c in lc.structural_cases("float32")]
FORWARD_EVENTS = set(lc.EVENTS) - {"bwd_window_full", "bwd_unstaged"}      # (those two belong to the log-sum-exp backward)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _functions(log_form):
    import torchsparsegradutils_amd as t

    return (t.sparse_log_softmax, torch.sparse.log_softmax) if log_form else (t.sparse_softmax, torch.sparse.softmax)


def _rounded(values64, dtype):
    """The case's float64 values as the value type under test holds them (the oracle gets exactly these)."""
    return torch.from_numpy(np.asarray(values64)).to(TORCH_DTYPE[dtype])


@functools.lru_cache(maxsize=None)
def _case(dtype, name):
    for n, ptr, vals in lc.structural_cases(dtype):
        if n == name:
            rng = np.random.default_rng(7)
            return ptr, _rounded(vals, dtype), _rounded(rng.standard_normal(int(ptr[-1])), dtype)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle(dtype, name, log_form):
    """(y64, d64, group length, |v - m|, sum_j |g_j| y_j or sum_j |g_j|) per entry, in CSR order, from torch.sparse on the CPU."""
    ptr, val, g = _case(dtype, name)
    n, nnz = ptr.size - 1, int(ptr[-1])
    lens = np.diff(ptr)
    rows = np.repeat(np.arange(n), lens)
    idx = torch.from_numpy(np.stack([rows, lc.columns(ptr)]))
    shape = (n, lc.axis_len_of(ptr))
    C = torch.sparse_coo_tensor(idx, val.double(), shape, is_coalesced=True).requires_grad_(True)
    y = _functions(log_form)[1](C, 1)
    G = torch.sparse_coo_tensor(idx, g.double(), shape, is_coalesced=True)
    (d,) = torch.autograd.grad(y, C, G)
    y64, d64 = y.detach().coalesce().values().numpy(), d.coalesce().values().numpy()
    v, ga = val.double().numpy(), np.abs(g.double().numpy())
    L = np.repeat(lens, lens).astype(np.float64)
    if nnz:
        starts = ptr[:-1][lens > 0]
        with np.errstate(invalid="ignore"):
            m = np.repeat(np.maximum.reduceat(v, starts), lens[lens > 0])
            w = ga if log_form else ga * y64
            S = np.repeat(np.add.reduceat(w, starts), lens[lens > 0])
            dist = np.abs(v - m)
    else:
        dist = S = np.zeros(0)
    return y64, d64, L, dist, S


def _bounds(dtype, name, log_form):
    _, val, g = _case(dtype, name)
    y64, d64, L, dist, S = _oracle(dtype, name, log_form)
    u, tiny = U[dtype], TINY[dtype]
    v, ga = val.double().numpy(), np.abs(g.double().numpy())
    with np.errstate(invalid="ignore", over="ignore"):
        if log_form:
            by = (L + 8) * u * np.maximum(1.0, np.abs(y64)) + u * np.abs(v)
            bd = (L + np.abs(y64) + 16) * u * (ga + np.exp(y64) * S) + 2.0 ** -53 * np.abs(v - y64) * np.exp(y64) * S
        else:
            by = (L + dist + 8) * u * y64 + tiny
            bd = (L + dist + 16) * u * (ga * y64 + y64 * S) + tiny * (ga + S)
    return by, bd


def _matrix(dtype, name, through_perm, requires_grad=True):
    """The case as a CSR matrix on the GPU, or the same matrix stored as CSC (its rows then go through the transpose's perm);
    `order`: position of every CSR entry in the returned tensor's value array."""
    ptr, val, g = _case(dtype, name)
    n, nnz = ptr.size - 1, int(ptr[-1])
    shape = (n, lc.axis_len_of(ptr))
    crow = torch.from_numpy(ptr).to(torch.int32).to(DEV)
    col = torch.from_numpy(lc.columns(ptr)).to(torch.int32).to(DEV)
    if not through_perm:
        A = torch.sparse_csr_tensor(crow, col, val.to(DEV), shape)
        return A.requires_grad_(requires_grad), torch.arange(nnz, device=DEV), g.to(DEV)
    order = torch.argsort(col.to(torch.int64), stable=True)          # CSC order: by column, rows ascending inside
    ccol = torch.zeros(shape[1] + 1, dtype=torch.int32, device=DEV)
    ccol[1:] = torch.cumsum(torch.bincount(col.to(torch.int64), minlength=shape[1]), 0)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (crow[1:] - crow[:-1]).to(torch.int64), output_size=nnz)
    A = torch.sparse_csc_tensor(ccol, rows[order].to(torch.int32), val.to(DEV)[order], shape)
    back = torch.empty_like(order)
    back[order] = torch.arange(nnz, device=DEV)
    return A.requires_grad_(requires_grad), back, g.to(DEV)


def _run(dtype, name, through_perm, log_form):
    """(y, d) of the function under test in CSR order, as float64 numpy."""
    fn = _functions(log_form)[0]
    A, back, g = _matrix(dtype, name, through_perm)
    y = fn(A, -1)
    assert y.layout == A.layout and y.shape == A.shape and y.dtype == A.dtype
    G = torch.sparse_csc_tensor(y.ccol_indices(), y.row_indices(), torch.empty_like(g).index_copy_(0, back, g), y.shape) \
        if through_perm else torch.sparse_csr_tensor(y.crow_indices(), y.col_indices(), g, y.shape)
    (d,) = torch.autograd.grad(y, A, G)
    assert d.layout == A.layout
    return y.detach().values()[back], d.values()[back]


def _check(got, want, bound, what):
    got = got.double().cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        same = (got == want) | nan                       # (equal infinities, and the NaN already compared)
        worst = np.where(same, 0.0, err / np.where(bound > 0, bound, 1.0))
        bad = ~same & ~(err <= bound)
    k = int(np.argmax(worst)) if worst.size else 0
    print(f"{what}: worst error / bound = {worst.max() if worst.size else 0.0:.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} entries beyond the bound, worst at {k}: got {got[k]!r}, want {want[k]!r}, bound {bound[k]!r}"


@pytest.mark.parametrize("through_perm", [False, True], ids=["csr_rows", "csc_rows_perm"])
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_structural_cases_against_float64(dtype, name, through_perm):
    ptr = _case(dtype, name)[0]
    ev = lc.events(ptr, dtype) & FORWARD_EVENTS
    print(f"{dtype} {name}: events {sorted(ev)}")
    for log_form in (False, True):
        y, d = _run(dtype, name, through_perm, log_form)
        y64, d64 = _oracle(dtype, name, log_form)[:2]
        by, bd = _bounds(dtype, name, log_form)
        tag = f"{dtype} {name} {'log_softmax' if log_form else 'softmax'}"
        _check(y, y64, by, tag + " values")
        _check(d, d64, bd, tag + " gradient")


@pytest.mark.parametrize("dtype", lc.DTYPES)
def test_structural_cases_cover_the_forward_events(dtype):
    reached = set()
    for name, ptr, _ in lc.structural_cases(dtype):
        reached |= lc.events(ptr, dtype)
    assert FORWARD_EVENTS <= reached, sorted(FORWARD_EVENTS - reached)


@pytest.mark.parametrize("through_perm", [False, True], ids=["csr_rows", "csc_rows_perm"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_bf16_is_the_fp32_path_rounded_once(name, through_perm):
    """The bf16 kernels compute in fp32 and round when the result is stored: the same bits as the fp32 kernels' result rounded
    to bf16, forward (through the public functions) and backward (the backend entry on the same bf16 y and g), and therefore
    within half a bf16 ulp of the float64 oracle beyond the fp32 bound."""
    from torchsparsegradutils_amd import _backend as be

    for log_form in (False, True):
        fn = _functions(log_form)[0]
        A, back, g = _matrix("bfloat16", name, through_perm, requires_grad=False)
        wide = (torch.sparse_csc_tensor(A.ccol_indices(), A.row_indices(), A.values().float(), A.shape) if through_perm
                else torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values().float(), A.shape))
        y, y32 = fn(A, -1).values(), fn(wide, -1).values()
        assert y.dtype == torch.bfloat16
        assert _same_bf16_bits(y, y32.to(torch.bfloat16))
        y64 = _oracle("bfloat16", name, log_form)[0]
        by = _bounds("bfloat16", name, log_form)[0] + U_BF16 * np.abs(np.nan_to_num(y64, posinf=0.0, neginf=0.0))
        _check(y[back], y64, by, f"bfloat16 {name} {'log_softmax' if log_form else 'softmax'} values")

        ptr = torch.from_numpy(_case("bfloat16", name)[0]).to(torch.int32).to(DEV)
        n = ptr.numel() - 1
        yk, gk = y[back].contiguous(), g.contiguous()                 # in CSR order: the groups are ptr's, no perm
        cross = True
        d = be.segment_softmax_backward(ptr, None, yk, gk, n, log_form, cross)
        d32 = be.segment_softmax_backward(ptr, None, yk.float(), gk.float(), n, log_form, cross)
        assert _same_bf16_bits(d, d32.to(torch.bfloat16))


def _same_bf16_bits(a, b):
    """Bit for bit equal, NaN at the same positions (a NaN's sign and payload are not part of the result)."""
    assert a.dtype == b.dtype == torch.bfloat16
    nan = a.isnan()
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    return torch.equal(nan, b.isnan()) and torch.equal(torch.where(nan, zero, a).view(torch.int16), torch.where(nan, zero, b).view(torch.int16))


def _random_csr(n, m, density, dtype, index_dtype, seed, batch=None):
    g = torch.Generator().manual_seed(seed)
    shape = (n, m) if batch is None else (batch, n, m)
    mask = torch.rand((n, m), generator=g) < density
    mask[n // 3] = False
    mask[:, m // 4] = False
    D = torch.randn(shape, generator=g, dtype=torch.float64) * mask
    D = torch.where(mask.expand(shape), torch.where(D == 0, torch.ones_like(D), D), D)
    A = D.to(dtype).to_sparse_csr()
    return torch.sparse_csr_tensor(A.crow_indices().to(index_dtype), A.col_indices().to(index_dtype), A.values(), A.shape).to(DEV), mask


def _dense_oracle(A_cpu, mask, dim, log_form):
    """torch.sparse on the float64 COO of a 2-D CPU matrix: (dense values, dense gradient for the upstream gradient W)."""
    D = A_cpu.to_dense().double()
    idx = mask.nonzero().t()
    C = torch.sparse_coo_tensor(idx, D[mask], D.shape, is_coalesced=True).requires_grad_(True)
    y = _functions(log_form)[1](C, dim % 2)
    W = torch.randn(D.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (d,) = torch.autograd.grad(y, C, torch.sparse_coo_tensor(idx, W[mask], D.shape, is_coalesced=True))
    return y.detach().to_dense(), d.to_dense(), W


def _as_layout(A, layout):
    if layout == "csr":
        return A
    if layout == "csc":
        B = A.to_sparse_csc()
        return torch.sparse_csc_tensor(B.ccol_indices().to(A.crow_indices().dtype), B.row_indices().to(A.crow_indices().dtype),
                                       B.values(), A.shape)
    return A.to_sparse_coo().coalesce()


LAYOUT_CASES = [("coo", torch.int64), ("csr", torch.int32), ("csr", torch.int64), ("csc", torch.int32), ("csc", torch.int64)]


@pytest.mark.parametrize("layout,index_dtype", LAYOUT_CASES, ids=[f"{a}-{str(b)[6:]}" for a, b in LAYOUT_CASES])
def test_layouts_and_index_types_agree_with_the_oracle(layout, index_dtype):
    """One 300 x 200 float32 matrix (rows of about 20, columns of about 30 entries, an empty row and an empty column; torch's COO
    carries int64 indices only).  With L <= 64, |v - m| <= 16 and |y| <= 21 in the log form, the factors (L + |v - m| + 16) u and
    (L + |y| + 16) u of the bounds in the module docstring are below 1e-5: the check uses that figure."""
    A, mask = _random_csr(300, 200, 0.1, torch.float32, index_dtype, 11)
    assert int(mask.sum(0).max()) <= 64 and int(mask.sum(1).max()) <= 64
    B = _as_layout(A, layout)
    tiny = TINY["float32"]
    for dim in (-1, -2):
        for log_form in (False, True):
            y64, d64, W = _dense_oracle(A.cpu(), mask, dim, log_form)
            X = B.detach().requires_grad_(True)
            y = _functions(log_form)[0](X, dim)
            assert y.layout == B.layout
            (d,) = torch.autograd.grad(y, X, W.to(DEV).float())            # (a strided gradient: gathered at the stored positions)
            got_y, got_d = y.detach().to_dense().double().cpu(), d.to_dense().double().cpu()
            Wa = W.abs() * mask
            if log_form:
                by = 1e-5 * y64.abs().clamp(min=1.0) + 2.0 ** -24 * A.cpu().to_dense().double().abs()
                bd = 1e-5 * (Wa + y64.exp() * Wa.sum(dim, keepdim=True))
            else:
                by = 1e-5 * y64 + tiny
                bd = 1e-5 * (Wa * y64 + y64 * (Wa * y64).sum(dim, keepdim=True)) + tiny * (Wa + Wa.sum(dim, keepdim=True))
            assert ((got_y - y64).abs() <= by)[mask].all()
            assert ((got_d - d64).abs() <= bd)[mask].all()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_one_row(n):
    import torchsparsegradutils_amd as t

    v = torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    A = torch.sparse_csr_tensor(torch.tensor([0, n], dtype=torch.int32), torch.arange(n, dtype=torch.int32), v.float(), (1, n)).to(DEV)
    want = torch.softmax(v.float().double(), 0)
    y = t.sparse_softmax(A, -1).values().double().cpu()
    assert ((y - want).abs() <= (n + 16 + 8) * 2.0 ** -24 * want).all()
    ly = t.sparse_log_softmax(A, -1).values().double().cpu()
    assert ((ly - want.log()).abs() <= (n + 8) * 2.0 ** -24 * want.log().abs().clamp(min=1.0) + 2.0 ** -24 * v.abs()).all()
    # along the columns every group is one entry
    assert torch.equal(t.sparse_softmax(A, -2).values(), torch.ones(n, device=DEV))
    assert torch.equal(t.sparse_log_softmax(A, -2).values(), torch.zeros(n, device=DEV))


def test_one_entry_per_row():
    import torchsparsegradutils_amd as t

    A = torch.sparse_csr_tensor(torch.arange(9, dtype=torch.int32), torch.tensor([3, 1, 4, 1, 5, 2, 6, 0], dtype=torch.int32),
                                torch.randn(8), (8, 8)).to(DEV).requires_grad_(True)
    y = t.sparse_softmax(A, -1)
    assert torch.equal(y.values(), torch.ones(8, device=DEV))
    y.values().sum().backward()
    assert torch.equal(A.grad.values(), torch.zeros(8, device=DEV))


def test_rows_sum_to_one_and_the_two_forms_agree():
    import torchsparsegradutils_amd as t

    A, mask = _random_csr(300, 200, 0.1, torch.float32, torch.int32, 12)
    u = 2.0 ** -24
    for dim in (-1, -2):
        y = t.sparse_softmax(A, dim)
        ly = t.sparse_log_softmax(A, dim)
        sums = y.to_dense().double().sum(dim)
        L = mask.sum(dim).double().to(DEV)
        assert ((sums - (L > 0).double()).abs() <= (L + 8) * u).all()
        # both within their bound of the exact value: |exp(ly) - y| <= y (bound_log + bound_softmax) to first order, with
        # |ly| <= 16 + log 64 and |v - m| <= 16 here
        yv, lyv = y.values().double(), ly.values().double()
        assert ((lyv.exp() - yv).abs() <= ((64 + 8) * u * lyv.abs().clamp(min=1.0) + 8 * u + (64 + 16 + 8) * u) * yv).all()


def test_batched_input_equals_its_items_bit_for_bit():
    import torchsparsegradutils_amd as t

    A, _ = _random_csr(70, 50, 0.2, torch.float32, torch.int32, 13, batch=3)
    for dim in (-1, -2):
        for fn in (t.sparse_softmax, t.sparse_log_softmax):
            X = A.detach().requires_grad_(True)
            y = fn(X, dim)
            G = torch.randn(y.values().shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
            (d,) = torch.autograd.grad(y, X, torch.sparse_csr_tensor(y.crow_indices(), y.col_indices(), G, y.shape))
            for i in range(3):
                Xi = torch.sparse_csr_tensor(A.crow_indices()[i], A.col_indices()[i], A.values()[i], A.shape[1:]).requires_grad_(True)
                yi = fn(Xi, dim)
                (di,) = torch.autograd.grad(yi, Xi, torch.sparse_csr_tensor(yi.crow_indices(), yi.col_indices(), G[i], yi.shape))
                assert torch.equal(yi.values(), y.values()[i]) and torch.equal(di.values(), d.values()[i])


def test_two_runs_give_the_same_bits():
    for through_perm in (False, True):
        for log_form in (False, True):
            a = _run("float32", "main_randn3", through_perm, log_form)
            b = _run("float32", "main_randn3", through_perm, log_form)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_softmax_then_sparse_mm_on_the_cached_plan():
    """sparse_mm(sparse_softmax(A, -1), X).square().sum() on a truncated 27-point PairwiseEncoder pattern (6 x 6 x 6), 8 columns:
    gradients of A and X against the dense float64 computation, and the product ran on the plan cached for A's own pattern —
    the output carries A's index tensors, so it is the same cache entry."""
    import torchsparsegradutils_amd as t
    from torchsparsegradutils_amd import _ops, _pattern, sparse_matmul as sm
    from torchsparsegradutils_amd.encoders import PairwiseEncoder

    _pattern.clear_cache()
    enc = PairwiseEncoder(radius=1.8, volume_shape=(1, 6, 6, 6), diag=True, layout=torch.sparse_csr, indices_dtype=torch.int32,
                          device=torch.device(DEV))
    assert len(enc.offsets) == 27
    gen = torch.Generator(device=DEV).manual_seed(2)
    A = enc(torch.randn((27, 1, 6, 6, 6), device=DEV, generator=gen)).detach().requires_grad_(True)
    X = torch.randn((216, 8), device=DEV, generator=gen).requires_grad_(True)
    plan = sm._Operand(A.detach()).plan
    assert _ops.launched(plan, "fwd") is None
    Y = t.sparse_softmax(A, -1)
    assert Y.crow_indices().data_ptr() == A.crow_indices().data_ptr() and Y.col_indices().data_ptr() == A.col_indices().data_ptr()
    t.sparse_mm(Y, X).square().sum().backward()
    assert sm._Operand(Y.detach()).plan.core is plan.core
    got = _ops.launched(plan, "fwd", torch.float32, 8)
    assert got is not None and got[2] >= 1, got

    mask = A.detach().to_dense() != 0
    Ad = A.detach().to_dense().double().cpu().requires_grad_(True)
    Xd = X.detach().double().cpu().requires_grad_(True)
    Z = torch.where(mask.cpu(), Ad, torch.full_like(Ad, float("-inf")))
    (torch.softmax(Z, -1) @ Xd).square().sum().backward()
    # fp32 throughout: rows of 27, 8 columns, values of order one — 1e-4 of the gradient's scale is two orders above the bounds
    gA = A.grad.to_dense().double().cpu()
    assert ((gA - Ad.grad)[mask.cpu()].abs() <= 1e-4 * Ad.grad.abs().max()).all()
    assert ((X.grad.double().cpu() - Xd.grad).abs() <= 1e-4 * Xd.grad.abs().max()).all()
    _pattern.clear_cache()


def test_merge_and_fix_up_are_launched_only_for_crossing_groups(monkeypatch):
    from torchsparsegradutils_amd import _backend as be

    notes = []
    monkeypatch.setattr(be, "SOFTMAX_LAUNCHES", notes)
    n = 512          # 32 entries per row: no row crosses a multiple of 2048 (or of 1024)
    crow = (torch.arange(n + 1, dtype=torch.int32) * 32).to(DEV)
    col = (torch.arange(n * 32, dtype=torch.int32) % 32).to(DEV)
    A = torch.sparse_csr_tensor(crow, col, torch.randn(n * 32, device=DEV), (n, 32)).requires_grad_(True)
    fn = _functions(False)[0]
    fn(A, -1).values().sum().backward()
    assert notes == [("tsgu_segment_softmax", ("main",)), ("tsgu_segment_softmax_backward", ("main",))], notes
    del notes[:]
    _run("float32", "main_needles", False, False)
    assert notes == [("tsgu_segment_softmax", ("main", "merge", "fix")), ("tsgu_segment_softmax_backward", ("main", "merge", "fix"))], notes
