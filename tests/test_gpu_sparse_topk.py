"""sparse_topk_mm on the GPU against the numpy restatement (tests/_topk_ref.py).

Sizes come from the kernel's own constants (`_backend.topk_geometry`: the cap on k, R query rows per workgroup, T keys per tile, KC
columns per LDS stage): n in {1, R − 1, R + 1, 2R + 3}, m in {1, k − 1, T − 1, T + 1, 3T + 5}, d in {1, 3, 24, KC + 8, 2 KC + 8} (partial
MFMA fragments, one and two stage crossings), k in {1, 8, 33, cap}; every value appears, the widest d and k at n = R + 1.

Exact cases hold integers in [−3, 3]: every product and sum is exact in all three accumulators, the restatement is integer
arithmetic and crow, col and the values must be EQUAL (bfloat16 values: the exact score rounded once, as the op promises).

Bounds of the random cases (counted roundings, not measurements), eps the machine epsilon of the accumulator (float32 for float32
and bfloat16 operands):
  score    bound_i = (d + 2) eps max_j Σ_t |scale Q[i,t] K[j,t]| + eps max_j |key_bias[j]|: d roundings of the fma chain, the product with
           scale, the sum with the bias.  A bfloat16 value is rounded once more: 2^-8 (|score| + bound_i).
  order    a stored score may be below an allowed unstored one by two such errors at most.
  backward 8 eps Σ|terms| per element (terms: scale G[i,j] K[j,t] for dQ, scale G[i,j] Q[i,t] for dK, G[i,j] for d key_bias): the products'
           own sums in fma form and the rounding of scale·G in the accumulator's type.  A bfloat16 result is that float32 result
           rounded once: 2^-8 (|exact| + the bound) more, and nothing that grows with Σ|terms|.
  pipeline sparse_attention's own bounds (tests/_attention_ref.py::error_bounds) on the restatement's selection; bfloat16 as that op's
           own test holds it: the float32 bound + 2^-8 |oracle| (every result is the float32 path's, rounded once).
"""

import functools

import numpy as np
import pytest
import torch

import _attention_ref as ar
import _topk_ref as tr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.bfloat16: 2.0 ** -23}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _geometry(dtype):
    from torchsparsegradutils_amd import _backend

    cap, R, T, KC, _ = _backend.topk_geometry(dtype)
    return cap, R, T, KC


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


def _run(Q, K, k, dtype, key_bias=None, index_dtype=torch.int32, **kw):
    """The op on the GPU for float64 numpy operands cast to `dtype`: (crow, col, val as float64, the tensor)."""
    from torchsparsegradutils_amd import sparse_topk_mm

    q, kk = (torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV) for x in (Q, K))
    b = None if key_bias is None else torch.from_numpy(np.ascontiguousarray(key_bias)).to(dtype).to(DEV)
    A = sparse_topk_mm(q, kk, k, key_bias=b, index_dtype=index_dtype, **kw)
    assert A.layout == torch.sparse_csr and A.dtype == dtype and A.col_indices().dtype == index_dtype == A.crow_indices().dtype
    assert tuple(A.shape) == tuple(Q.shape[:-1]) + (K.shape[-2],)
    return A.crow_indices().cpu().numpy(), A.col_indices().cpu().numpy(), A.values().double().cpu().numpy(), A


def _as_stored(val, dtype):
    """Exact float64 scores as the op stores them: rounded once to the value type."""
    return torch.from_numpy(np.ascontiguousarray(val)).to(dtype).double().numpy()


def _assert_equal(got, S, k, ok, dtype, what):
    crow, col, val = got[:3]
    rc, rcol, rval = tr.select(S, k, ok)
    assert np.array_equal(crow, rc), f"{what}: crow"
    assert np.array_equal(col, rcol), f"{what}: col"
    assert np.array_equal(val, _as_stored(rval, dtype), equal_nan=True), f"{what}: values"


def _shapes(dtype):
    cap, R, T, KC = _geometry(dtype)
    return [(70, 333, 40, 16), (1, 1, 1, 1), (R - 1, 7, 3, 8), (R + 1, T - 1, 24, 33), (2 * R + 3, T + 1, KC + 8, 1),
            (R + 1, 3 * T + 5, 2 * KC + 8, cap), (1, cap - 1, 24, cap), (2 * R + 3, 3 * T + 5, 1, 33)]


# ---- 1. exact, with ties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", range(8))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_integer_data_gives_the_restatement_exactly(dtype, case):
    n, m, d, k = _shapes(dtype)[case]
    rng = np.random.default_rng(0)
    Q, K = _ints(rng, (n, d)), _ints(rng, (m, d))
    bias = _ints(rng, m) if case % 2 else None
    S = tr.scores(Q, K, 1.0, bias)
    ok = tr.allowed(n, m)
    assert np.array_equal(tr.select(S, k, ok)[0], tr.crow(n, m, k))
    if case == 0:
        ties = tr.boundary_ties(S, k, ok)
        print(f"rows with a tie across the k-th boundary: {int(ties.sum())} of {n}")
        assert ties.sum() * 4 >= n, "the case has lost its point: few rows have a tie across the k-th boundary"
    _assert_equal(_run(Q, K, k, dtype, key_bias=bias), S, k, ok, dtype, f"{(n, m, d, k)}")


# ---- 2. adversarial arrival orders --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 33, "cap"])
@pytest.mark.parametrize("order", ["rising", "falling", "equal", "one-hot"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_arrival_orders(dtype, order, k):
    cap, R, T, KC = _geometry(dtype)
    k = cap if k == "cap" else k
    n, m = R + 1, 3 * T + 5
    rng = np.random.default_rng(1)
    if order == "one-hot":
        d = 24
        Q = np.zeros((n, d))
        Q[np.arange(n), np.arange(n) % d] = 1.0
        K = ((7 * np.arange(m)[:, None] + 3 * np.arange(d)[None, :] ** 2) % 11 - 5).astype(np.float64)      # K[j, t] != K[t, j]
    else:
        d = 1
        Q = 1.0 + (np.arange(n)[:, None] % 3)
        ramp = np.arange(m, dtype=np.float64) - 90.0                # |.| <= 107: exact in bfloat16, as 3·107 is in its accumulator
        K = {"rising": ramp, "falling": -ramp, "equal": np.full(m, 2.0)}[order][:, None]
    S = tr.scores(Q, K)
    ok = tr.allowed(n, m)
    got = _run(Q, K, k, dtype)
    _assert_equal(got, S, k, ok, dtype, f"{order} k={k}")
    if order == "equal":
        assert np.array_equal(got[1].reshape(n, k), np.tile(np.arange(k), (n, 1))), "all keys equal: columns 0 ... k − 1"
    if order == "rising":
        assert np.array_equal(got[1].reshape(n, k), np.tile(np.arange(m - k, m), (n, 1)))


# ---- 3. random data -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(dtype, which):
    cap, R, T, KC = _geometry(dtype)
    n, m, d, k = [(2 * R + 3, 3 * T + 5, KC + 8, 33), (R + 1, T + 1, 2 * KC + 8, cap), (R - 1, 3 * T + 5, 24, 8)][which]
    gen = torch.Generator().manual_seed(3 + which)
    Q, K, bias = (torch.randn(s, generator=gen, dtype=torch.float64).to(dtype).double().numpy() for s in ((n, d), (m, d), (m,)))
    scale = 0.37
    S = tr.scores(Q, K, scale, bias)
    bound = (d + 2) * EPS[dtype] * (abs(scale) * (np.abs(Q) @ np.abs(K).T)).max(1) + EPS[dtype] * np.abs(bias).max()
    return (n, m, d, k), Q, K, bias, scale, S, bound


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_random_data_within_the_counted_roundings(dtype, which):
    (n, m, d, k), Q, K, bias, scale, S, bound = _random_case(dtype, which)
    crow, col, val, _ = _run(Q, K, k, dtype, key_bias=bias, scale=scale)
    assert np.array_equal(crow, tr.crow(n, m, k)), "crow is the closed form"
    worst_a = worst_c = 0.0
    for i in range(n):
        c, v = col[crow[i]:crow[i + 1]], val[crow[i]:crow[i + 1]]
        assert c.size == min(k, m) and np.all(np.diff(c) > 0) and c.min() >= 0 and c.max() < m, f"row {i}: structure"
        slack = bound[i] + (2.0 ** -8 * (np.abs(S[i, c]) + bound[i]) if dtype == torch.bfloat16 else 0.0)
        err = np.abs(v - S[i, c])
        worst_a = max(worst_a, float((err / slack).max()))
        assert np.all(err <= slack), f"row {i}: a stored value is outside the bound"
        rest = np.setdiff1d(np.arange(m), c)
        if rest.size:
            gap = S[i, rest].max() - S[i, c].min()
            worst_c = max(worst_c, float(gap / (2 * bound[i])))
            assert gap <= 2 * bound[i], f"row {i}: an unstored score beats a stored one by more than two errors"
    print(f"{(n, m, d, k)}: max |err| / bound = {worst_a:.3g}, max order gap / (2 bound) = {worst_c:.3g}")


# ---- 4. special values --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_infinities_and_nan(dtype):
    cap, R, T, KC = _geometry(dtype)
    n, m, d, k = R + 1, T + 1, 3, 8
    rng = np.random.default_rng(4)
    Q, K = _ints(rng, (n, d)), _ints(rng, (m, d))
    ok = tr.allowed(n, m)
    # −inf on all but five keys: three −inf entries per row, the lowest columns among them
    bias = np.full(m, -np.inf)
    finite = np.array([3, 17, 18, T - 1, T])
    bias[finite] = 0.0
    S = tr.scores(Q, K, 1.0, bias)
    got = _run(Q, K, k, dtype, key_bias=bias)
    _assert_equal(got, S, k, ok, dtype, "-inf")
    rows = got[1].reshape(n, k)
    assert np.all(np.isin(finite, rows[0])) and np.array_equal(np.setdiff1d(rows[0], finite), [0, 1, 2])
    # a NaN key row ranks first in every row, +inf behind it
    Kn = K.copy()
    Kn[T - 2] = np.nan
    bias = np.zeros(m)
    bias[[5, T]] = np.inf
    S = tr.scores(Q, Kn, 1.0, bias)
    assert np.isnan(S[:, T - 2]).all() and np.isnan(S).sum() == n
    for kk in (1, 2, k):
        got = _run(Q, Kn, kk, dtype, key_bias=bias)
        _assert_equal(got, S, kk, ok, dtype, f"NaN k={kk}")
        rows = got[1].reshape(n, kk)
        assert np.all((rows == T - 2).sum(1) == 1), "the NaN key is in every row"
        if kk >= 2:
            assert np.all((rows == 5).sum(1) == 1), "+inf follows, the lower column first"


# ---- 5. flags and batches -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [dict(causal=True), dict(exclude_self=True), dict(causal=True, exclude_self=True)],
                         ids=["causal", "exclude_self", "both"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_flags(dtype, flags):
    cap, R, T, KC = _geometry(dtype)
    rng = np.random.default_rng(5)
    for n, m in ((R + 1, 3 * T + 5), (T + 1, T + 1), (3 * T + 5, R + 1)):       # n < m, n = m, n > m (empty leading rows)
        d, k = 3, 8
        Q, K = _ints(rng, (n, d)), _ints(rng, (m, d))
        ok = tr.allowed(n, m, **flags)
        S = tr.scores(Q, K)
        assert np.array_equal(tr.select(S, k, ok)[0], tr.crow(n, m, k, **flags))
        got = _run(Q, K, k, dtype, **flags)
        _assert_equal(got, S, k, ok, dtype, f"{flags} {(n, m)}")
        if flags.get("causal") and n > m:
            assert got[0][n - m] == 0, "rows without an allowed column are empty"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_batches_and_index_types(dtype):
    cap, R, T, KC = _geometry(dtype)
    b, n, m, d, k = 3, R + 1, T + 1, 24, 8
    rng = np.random.default_rng(6)
    Q, K, bias = _ints(rng, (b, n, d)), _ints(rng, (b, m, d)), _ints(rng, (b, m))
    ok = tr.allowed(n, m, exclude_self=True)
    crow, col, val, A = _run(Q, K, k, dtype, key_bias=bias, exclude_self=True)
    crow64, col64, val64, A64 = _run(Q, K, k, dtype, key_bias=bias, exclude_self=True, index_dtype=torch.int64)
    assert np.array_equal(crow, crow64) and np.array_equal(col, col64) and np.array_equal(val, val64)
    assert crow.shape == (b, n + 1) and col.shape == val.shape == (b, n * k)
    for i in range(b):
        _assert_equal((crow[i], col[i], val[i]), tr.scores(Q[i], K[i], 1.0, bias[i]), k, ok, dtype, f"batch item {i}")
    assert not np.array_equal(col[0], col[1])


# ---- 6. backward ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [0.37, 1.0], ids=["scaled", "unit"])
@pytest.mark.parametrize("batched", [False, True], ids=["2d", "batched"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_backward_against_the_dense_composition(dtype, batched, scale):
    from torchsparsegradutils_amd import sparse_topk_mm

    cap, R, T, KC = _geometry(dtype)
    b, n, m, d, k = (3 if batched else 1), 2 * R + 3, 3 * T + 5, 24, 8
    gen = torch.Generator().manual_seed(7)
    Q, K, bias, G = (torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in ((b, n, d), (b, m, d), (b, m), (b, n, m)))
    if not batched:
        Q, K, bias, G = Q[0], K[0], bias[0], G[0]
    q, kk, bb = (x.to(DEV).requires_grad_(True) for x in (Q, K, bias))
    A = sparse_topk_mm(q, kk, k, scale=scale, key_bias=bb)
    dense = torch.autograd.grad(A, (q, kk, bb), G.to(DEV), retain_graph=True)                 # a dense cotangent is gathered
    mask = torch.zeros((b, n, m), dtype=torch.bool)
    crow, col = A.crow_indices().cpu().reshape(b, -1), A.col_indices().cpu().reshape(b, -1)
    at = []
    for i in range(b):
        rows = torch.repeat_interleave(torch.arange(n), crow[i].diff())
        mask[i, rows, col[i].long()] = True
        at.append(G.reshape(b, n, m)[i, rows, col[i].long()])
    Gs = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), torch.stack(at).reshape(A.values().shape).to(DEV), A.shape)
    sparse = torch.autograd.grad(A, (q, kk, bb), Gs)                                          # a cotangent on the result's own pattern
    Gm = torch.where(mask, G.double().reshape(b, n, m), torch.zeros((), dtype=torch.float64))
    Q3, K3 = Q.double().reshape(b, n, d), K.double().reshape(b, m, d)
    want = (scale * Gm @ K3, scale * Gm.transpose(1, 2) @ Q3, Gm.sum(1))
    terms = (abs(scale) * Gm.abs() @ K3.abs(), abs(scale) * Gm.abs().transpose(1, 2) @ Q3.abs(), Gm.abs().sum(1))
    for name, gd, gs, w, t in zip(("dQ", "dK", "d key_bias"), dense, sparse, want, terms):
        assert gd.dtype == dtype and torch.equal(gd, gs), f"{name}: dense and sparse cotangents agree bit for bit"
        bound = 8 * EPS[dtype] * t
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * (w.abs() + bound)
        err = (gd.double().cpu().reshape(w.shape) - w).abs()
        print(f"{name}: max |err| / bound = {float((err / bound.clamp(min=1e-300)).max()):.3g}")
        assert bool((err <= bound).all()), name


# ---- 7. pipeline ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_topk_feeds_sparse_attention(dtype):
    from torchsparsegradutils_amd import sparse_attention, sparse_topk_mm

    cap, R, T, KC = _geometry(dtype)
    n, m, d, k, scale = 2 * R + 3, 3 * T + 5, 16, 8, 0.25
    rng = np.random.default_rng(8)
    Q, K = _ints(rng, (n, d)), _ints(rng, (m, d))                    # exact scores: the selection is the restatement's
    gen = torch.Generator().manual_seed(8)
    V, dO = (torch.randn(s, generator=gen, dtype=torch.float64).to(dtype).double() for s in ((m, d), (n, d)))
    crow, col, _ = tr.select(tr.scores(Q, K), k, tr.allowed(n, m))
    mask = torch.zeros((n, m), dtype=torch.bool)
    mask[np.repeat(np.arange(n), np.diff(crow)), col] = True
    Qt, Kt = torch.from_numpy(Q), torch.from_numpy(K)
    B = torch.zeros((n, m), dtype=torch.float64)
    heads = tuple(ar.heads_view(x, False) for x in (Qt, Kt, V, dO))
    O, dQ, dK, dV, _, P = ar.dense_oracle(mask, B, *heads, scale, use_bias=False)
    acc = np.float64 if dtype == torch.float64 else np.float32
    bounds = ar.error_bounds(mask, B, *heads, scale, False, float(np.finfo(acc).eps) / 2, float(np.finfo(acc).tiny), P, O)
    assert bounds[5] < 2.0 ** -10
    q, kk, v = (x.to(dtype).to(DEV).requires_grad_(True) for x in (Qt, Kt, V))
    A = sparse_topk_mm(q, kk, k)
    out = sparse_attention(A, q, kk, v, scale=scale, values_as_bias=False)
    grads = torch.autograd.grad(out, (q, kk, v), dO.to(dtype).to(DEV))
    for name, g, w, bd in zip(("O", "dQ", "dK", "dV"), (out.detach(),) + grads, (O, dQ, dK, dV), bounds):
        w, bd = w.squeeze(-2), bd.squeeze(-2)
        if dtype == torch.bfloat16:
            assert g.dtype == torch.bfloat16
            bd = bd + 2.0 ** -8 * w.abs()
        err = (g.double().cpu() - w).abs()
        print(f"{name}: max |err| / bound = {float((err / bd.clamp(min=1e-300)).max()):.3g}")
        assert bool((err <= bd).all()), name


# ---- 8. no host synchronisation -------------------------------------------------------------------------------------------------------

def test_the_forward_is_captured_in_a_graph():
    from torchsparsegradutils_amd import sparse_topk_mm

    cap, R, T, KC = _geometry(torch.float32)
    n, m, d, k = R + 1, 3 * T + 5, 24, 8
    gen = torch.Generator().manual_seed(9)
    Q, K, bias = (torch.randn(s, generator=gen).to(DEV) for s in ((n, d), (m, d), (m,)))
    eager = sparse_topk_mm(Q, K, k, key_bias=bias, causal=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = sparse_topk_mm(Q, K, k, key_bias=bias, causal=True)
    held.values().zero_()
    held.col_indices().fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(held.crow_indices(), eager.crow_indices()) and torch.equal(held.col_indices(), eager.col_indices())
    assert torch.equal(held.values(), eager.values()), "the replay is bit-identical to the eager result"
