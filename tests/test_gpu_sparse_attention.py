"""sparse_attention on the GPU against the dense float64 oracle on the CPU (tests/_attention_ref.py), given exactly the rounded inputs.

Structural cases: the smallest patterns that reach every branch of the kernels' walk (csrc/attention_impl.h), built from the
kernels' own constants (`_backend.attention_geometry`: entry lanes EP, rows per workgroup RPB, staged slice S):
  short    37×23: rows of 0, 1, EP−1, EP, EP+1 entries and random ones; an empty column; 37 is no multiple of any RPB
  ragged   300×41: random rows, more than one workgroup, n ≠ m
  slices   workgroups whose entries number S−1, S (one slice, exactly) and S+1 (two), made of one long row and RPB−1 rows of one
           entry; rows of S−1, S, S+1 entries lying across slice boundaries; one row of three slices (2S+7 entries)
  hub      (3S+1)×41: column 0 is referenced by every row (the column pass walks it slice after slice), column 5 by none
Each runs stored as CSR (the row pass walks the pattern's own arrays, the column pass its transpose through `perm`) and as CSC
(the other way round), with int32 and int64 indices.

Bounds (derived, not measured): tests/_attention_ref.py::error_bounds, with u = 2^-24 (float32, bfloat16) or 2^-53 and
ρ_j = e_j + Σ_l p_l e_l + (3L + |t_j − max t| + 8) u the relative error of a probability (16 for the gradients), the counts of
the issue this operator was written to.  How the kernels' operation order meets them:
  * the logit is a dot of d terms in fma form (d roundings), one fma for scale and bias: e_j = (d + 2) u a_j covers it;
  * online softmax: an entry costs an exp, and either a rescale of the state (one multiplication) or a product, and one addition:
    3 roundings per entry of the lane's share of the row, so 3L/EP along a lane.  The arguments of the rescaling exps telescope
    (the running maximum only rises): together with the entry's own exp they round |t_j − max t| u in the exponent;
  * the EP entry lanes are merged by log2(EP) <= 2 butterfly steps of (exp, product, sum) = 3 roundings each; merging with a lane
    that holds no entry is exact (factor 1 and 0).  3L/EP + 3 log2(EP) <= 3L for L >= 2, and a row of one entry has no merge;
  * the final division (forward) or exp(t − lse) with lse = max + log s (backward: two roundings of lse, one of the difference,
    the exp) are in the constants 8 and 16.
  * δ is summed over the row as Σ_j p_j dP_j rather than taken as <dO, O>: its absolute evaluation is the first term of δ̄, and
    the second (d u Σ|dO||O|) is not needed; the bound is kept as stated.
The gradient bounds also carry the forward's underflow term (tiny per stored probability, see error_bounds): without it a
probability that underflows in float32 would have to be matched exactly.
bfloat16: every result is the float32 path's result on the same bfloat16-valued inputs rounded once, bit for bit (the kernels
walk a row with the same lanes in both types), hence within the float32 bound + 2^-8 |oracle|.
"""

import functools
import os
import re

import numpy as np
import pytest
import torch

import _attention_ref as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
TINY = {torch.float32: float(np.finfo(np.float32).tiny), torch.float64: float(np.finfo(np.float64).tiny)}
GEOMETRIES = [(1, 8), (3, 16), (2, 64), (1, 128), (8, 128)]
CASES = ["short", "ragged", "slices", "hub"]
SCALE = {8: 8 ** -0.5, 16: 0.25, 64: 0.125, 128: 128 ** -0.5}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _geometry(dtype, heads, d):
    from torchsparsegradutils_amd import _backend

    return _backend.attention_geometry(dtype, heads, d)


def _rows_mask(lengths, m, gen, first=None):
    """A mask with the given row lengths: random columns, `first` (a column) in every non-empty row when given."""
    mask = torch.zeros((len(lengths), m), dtype=torch.bool)
    for i, L in enumerate(lengths):
        cols = torch.randperm(m, generator=gen)[:L]
        mask[i, cols] = True
    if first is not None:
        mask[:, first] = True
    return mask


@functools.lru_cache(maxsize=None)
def _mask(case, ep, rpb, stage):
    gen = torch.Generator().manual_seed(11)
    if case == "short":
        n, m = 37, 23
        lengths = [0, 1, max(ep - 1, 0), ep, ep + 1] + torch.randint(0, 12, (n - 5,), generator=gen).tolist()
        mask = _rows_mask(lengths, m, gen)
        mask[:, 7] = False
        return mask
    if case == "ragged":
        return torch.rand((300, 41), generator=gen) < 0.2
    if case == "slices":
        m = 2 * stage + 16
        lengths = []
        for total in (stage - 1, stage, stage + 1):           # three workgroups by their number of entries
            lengths += [total - (rpb - 1)] + [1] * (rpb - 1)
        lengths += [stage - 1, stage, stage + 1, 2 * stage + 7]  # rows across slice boundaries, and one of three slices
        lengths += [3]                                          # (the row count is no multiple of RPB)
        return _rows_mask(lengths, m, gen)
    if case == "hub":
        n, m = 3 * stage + 1, 41
        mask = torch.rand((n, m), generator=gen) < 0.05
        mask[:, 0] = True
        mask[:, 5] = False
        return mask
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def _inputs(case, heads, d, dtype, spread=False):
    """(mask, B, Q, K, V, dO) ~ N(0, 1) rounded to `dtype` (as float64; the oracle gets exactly these).  spread: the bias takes
    values up to ±40, so that exp underflows inside a row."""
    ep, rpb, stage = _geometry(torch.float32 if dtype == torch.bfloat16 else dtype, heads, d)
    mask = _mask(case, ep, rpb, stage)
    n, m = mask.shape
    gen = torch.Generator().manual_seed(5)
    shapes = ((n, m), (n, heads, d), (m, heads, d), (m, heads, d), (n, heads, d))
    B, Q, K, V, dO = (torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes)
    if spread:
        B = B * 40 / 3
        B = B.clamp(-40, 40)
    return (mask,) + tuple(x.to(dtype).double() for x in (B, Q, K, V, dO))


@functools.lru_cache(maxsize=None)
def _reference(case, heads, d, dtype, spread=False):
    """(oracle results, bounds) in float64: computed once per case, shared by the layouts and index types, never changed."""
    mask, B, Q, K, V, dO = _inputs(case, heads, d, dtype, spread)
    O, dQ, dK, dV, dB, P = ar.dense_oracle(mask, B, Q, K, V, dO, SCALE[d])
    acc = torch.float32 if dtype == torch.bfloat16 else dtype
    bounds = ar.error_bounds(mask, B, Q, K, V, dO, SCALE[d], True, U[acc], TINY[acc], P, O)
    return (O, dQ, dK, dV, dB), bounds


def _run(case, heads, d, dtype, layout, index_dtype, spread=False):
    """(O, dQ, dK, dV, dA at the stored positions as a dense [n, m]) of the operator under test, on the GPU."""
    from torchsparsegradutils_amd import sparse_attention

    mask, B, Q, K, V, dO = _inputs(case, heads, d, dtype, spread)
    A = ar.sparse_from_dense(B, mask, layout, index_dtype, dtype).to(DEV).requires_grad_(True)
    q, k, v = (x.to(dtype).to(DEV).requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v, scale=SCALE[d])
    dA, dq, dk, dv = torch.autograd.grad(O, (A, q, k, v), dO.to(dtype).to(DEV))
    assert dA.layout == A.layout and dA.dtype == dtype
    for a, b in zip(ar.index_tensors(A), ar.index_tensors(dA)):
        assert a.data_ptr() == b.data_ptr() and a.dtype == index_dtype
    dense = torch.zeros(mask.shape, dtype=dtype)
    order = ar.stored_order(torch.arange(mask.numel()).view(mask.shape), A.detach().cpu())
    dense.view(-1)[order] = ar.values_of(dA).cpu()
    return O.detach().cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dense


def _assert_within(got, want, bound, extra, what):
    print(f"{what}: max |err| / bound = {float(((got.double() - want).abs() / (bound + extra).clamp(min=1e-300)).max()):.3g}")
    assert torch.equal(got.isnan(), want.isnan()), what
    assert bool(((got.double() - want).abs() <= bound + extra).all()), what


NAMES = ("O", "dQ", "dK", "dV", "dA")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("heads,d", GEOMETRIES, ids=[f"H{h}d{d}" for h, d in GEOMETRIES])
@pytest.mark.parametrize("case", CASES)
def test_structural_cases_within_the_bounds(case, heads, d, dtype):
    want, bounds = _reference(case, heads, d, dtype)
    assert bounds[5] < 2.0 ** -10, "the first-order bound needs max rho < 2^-10"
    mask = _inputs(case, heads, d, dtype)[0]
    for layout, index_dtype in (("csr", torch.int32), ("csc", torch.int32), ("csr", torch.int64), ("csc", torch.int64)):
        got = _run(case, heads, d, dtype, layout, index_dtype)
        for name, g, w, b in zip(NAMES, got, want, bounds):
            if name == "dA":
                g, w, b = g[mask], w[mask], b[mask]
            _assert_within(g, w, b, 0.0, f"{name} {case} H{heads} d{d} {layout} {index_dtype}")
    assert bool((got[0][~mask.any(1)] == 0).all()) and bool((got[1][~mask.any(1)] == 0).all())      # rows without entries
    assert bool((got[2][~mask.any(0)] == 0).all()) and bool((got[3][~mask.any(0)] == 0).all())      # columns without entries


@pytest.mark.parametrize("heads,d", GEOMETRIES, ids=[f"H{h}d{d}" for h, d in GEOMETRIES])
@pytest.mark.parametrize("case", CASES)
def test_bfloat16_is_the_float32_result_rounded_once(case, heads, d):
    """The same bfloat16-valued inputs through the float32 kernels and through the bfloat16 kernels: bit for bit the rounded
    float32 results, hence within the float32 bound + 2^-8 |oracle|."""
    from torchsparsegradutils_amd import sparse_attention

    mask, B, Q, K, V, dO = _inputs(case, heads, d, torch.bfloat16)
    want, bounds = _reference(case, heads, d, torch.bfloat16)
    assert bounds[5] < 2.0 ** -10
    for layout in ("csr", "csc"):
        low = _run(case, heads, d, torch.bfloat16, layout, torch.int32)
        A = ar.sparse_from_dense(B, mask, layout, torch.int32, torch.float32).to(DEV).requires_grad_(True)
        q, k, v = (x.float().to(DEV).requires_grad_(True) for x in (Q, K, V))
        O = sparse_attention(A, q, k, v, scale=SCALE[d])
        dA, dq, dk, dv = torch.autograd.grad(O, (A, q, k, v), dO.float().to(DEV))
        dense = torch.zeros(mask.shape)
        dense.view(-1)[ar.stored_order(torch.arange(mask.numel()).view(mask.shape), A.detach().cpu())] = ar.values_of(dA).cpu()
        full = (O.detach().cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dense)
        for name, lo, hi, w, b in zip(NAMES, low, full, want, bounds):
            if name == "dA":
                lo, hi, w, b = lo[mask], hi[mask], w[mask], b[mask]
            assert lo.dtype == torch.bfloat16 and torch.equal(lo, hi.to(torch.bfloat16)), f"{name} {case} {layout}"
            _assert_within(lo, w, b, 2.0 ** -8 * w.abs(), f"{name} {case} H{heads} d{d} {layout} bf16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_bias_spread_over_80_underflows_inside_rows(dtype):
    want, bounds = _reference("ragged", 3, 16, dtype, True)
    assert bounds[5] < 2.0 ** -10
    mask, B = _inputs("ragged", 3, 16, dtype, True)[:2]
    assert float(B[mask].max()) == 40 and float(B[mask].min()) == -40
    for layout in ("csr", "csc"):
        got = _run("ragged", 3, 16, dtype, layout, torch.int32, True)
        for name, g, w, b in zip(NAMES, got, want, bounds):
            if name == "dA":
                g, w, b = g[mask], w[mask], b[mask]
            _assert_within(g, w, b, 0.0, f"{name} spread {layout}")


def _batched_operands(dtype, layout):
    """b = 3 items with different values on one mask (torch's batched CSR / CSC), or different masks as well (COO)."""
    gen = torch.Generator().manual_seed(21)
    n, m, heads, d, b = 45, 19, 3, 16, 3
    masks = [torch.rand((n, m), generator=gen) < 0.3 for _ in range(b)]
    if layout != "coo":
        masks = [masks[0]] * b
    shapes = ((b, n, m), (b, n, heads, d), (b, m, heads, d), (b, m, heads, d), (b, n, heads, d))
    B, Q, K, V, dO = (torch.randn(s, generator=gen, dtype=torch.float64).to(dtype).double() for s in shapes)
    return masks, B, Q, K, V, dO


def _sparse_item(B, mask, layout, dtype):
    if layout == "coo":
        idx = mask.nonzero().t()
        return torch.sparse_coo_tensor(idx, B[mask].to(dtype), mask.shape, is_coalesced=True)
    return ar.sparse_from_dense(B, mask, layout, torch.int32, dtype)


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_batched_items_within_the_bounds_and_bitwise_those_of_the_item_alone(layout):
    from torchsparsegradutils_amd import sparse_attention

    dtype, scale = torch.float32, 0.25
    masks, B, Q, K, V, dO = _batched_operands(dtype, layout)
    if layout == "coo":
        idx = torch.cat([torch.cat([torch.full((1, int(mk.sum())), i), mk.nonzero().t()]) for i, mk in enumerate(masks)], 1)
        A = torch.sparse_coo_tensor(idx, torch.cat([B[i][mk] for i, mk in enumerate(masks)]).to(dtype), B.shape, is_coalesced=True)
    else:
        A = ar.sparse_from_dense(B, masks[0], layout, torch.int32, dtype)
    A = A.to(DEV).requires_grad_(True)
    q, k, v = (x.to(dtype).to(DEV).requires_grad_(True) for x in (Q, K, V))
    O = sparse_attention(A, q, k, v, scale=scale)
    dA, dq, dk, dv = torch.autograd.grad(O, (A, q, k, v), dO.to(dtype).to(DEV))
    assert dA.layout == A.layout and dA.shape == A.shape
    dAd = torch.zeros(B.shape, dtype=dtype)
    if layout == "coo":
        dAd[tuple(dA._indices().cpu())] = dA._values().cpu()
    else:
        order = ar.stored_order(torch.arange(B.numel()).view(B.shape), A.detach().cpu())
        dAd.view(-1)[order.reshape(-1)] = dA.values().cpu().reshape(-1)
    for i, mk in enumerate(masks):
        want = ar.dense_oracle(mk, B[i], Q[i], K[i], V[i], dO[i], scale)
        bounds = ar.error_bounds(mk, B[i], Q[i], K[i], V[i], dO[i], scale, True, U[dtype], TINY[dtype], want[5], want[0])
        assert bounds[5] < 2.0 ** -10
        Ai = _sparse_item(B[i], mk, layout, dtype).to(DEV).requires_grad_(True)
        qi, ki, vi = (x[i].to(dtype).to(DEV).requires_grad_(True) for x in (Q, K, V))
        Oi = sparse_attention(Ai, qi, ki, vi, scale=scale)
        dAi, dqi, dki, dvi = torch.autograd.grad(Oi, (Ai, qi, ki, vi), dO[i].to(dtype).to(DEV))
        got = (O[i].detach().cpu(), dq[i].cpu(), dk[i].cpu(), dv[i].cpu(), dAd[i])
        alone = (Oi.detach().cpu(), dqi.cpu(), dki.cpu(), dvi.cpu())
        for name, g, a in zip(NAMES, got, alone):
            assert torch.equal(g, a), f"{name} of item {i} differs from the item run alone"
        alone_dA = torch.zeros(mk.shape, dtype=dtype)
        if layout == "coo":
            alone_dA[tuple(dAi._indices().cpu())] = dAi._values().cpu()
        else:
            alone_dA.view(-1)[ar.stored_order(torch.arange(mk.numel()).view(mk.shape), Ai.detach().cpu())] = dAi.values().cpu()
        assert torch.equal(dAd[i], alone_dA)
        for name, g, w, b in zip(NAMES, got, want, bounds):
            if name == "dA":
                g, w, b = g[mk], w[mk], b[mk]
            _assert_within(g, w, b, 0.0, f"{name} item {i} {layout}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_two_runs_are_bitwise_equal(dtype):
    for case, heads, d in (("slices", 3, 16), ("hub", 8, 128)):
        first = _run(case, heads, d, dtype, "csr", torch.int32)
        second = _run(case, heads, d, dtype, "csr", torch.int32)
        for name, a, b in zip(NAMES, first, second):
            assert torch.equal(a, b), (name, case)


def test_against_the_parts():
    """O against sparse_mm(sparse_softmax(S), V) per head, S = csr_sddmm(Q, K)·scale + bias: within the sum of both bounds — the
    fused bound above, and for the chain (d + 2) u a_j on the logit, test_gpu_sparse_softmax.py's (L + |v − m| + 8) u on the
    probability and L u for the product's sum, against the same oracle."""
    import torchsparsegradutils_amd as t
    from torchsparsegradutils_amd import _backend

    heads, d, dtype = 3, 16, torch.float32
    mask, B, Q, K, V, dO = _inputs("ragged", heads, d, dtype)
    (O64, *_), bounds = _reference("ragged", heads, d, dtype)
    A = ar.sparse_from_dense(B, mask, "csr", torch.int32, dtype).to(DEV)
    q, k, v = (x.to(dtype).to(DEV) for x in (Q, K, V))
    O = t.sparse_attention(A, q, k, v, scale=SCALE[d]).cpu()
    n, m = mask.shape
    u = U[dtype]
    L = mask.sum(1).double().view(n, 1, 1)
    for h in range(heads):
        S = _backend.csr_sddmm(A.crow_indices(), A.col_indices(), q[:, h].contiguous(), k[:, h].contiguous(), n, m, alpha=SCALE[d])
        P = t.sparse_softmax(torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), S + A.values(), A.shape), -1)
        Oh = t.sparse_mm(P, v[:, h].contiguous()).cpu()
        # the chain's bound in the oracle's terms: the fused bound's ρ without the online terms is smaller than ρ itself, so the
        # fused bound + L u Σ p |v| covers the chain
        P64 = torch.softmax((torch.einsum("id,jd->ij", Q[:, h], K[:, h]) * SCALE[d] + B).masked_fill(~mask, float("-inf")), -1)
        P64 = torch.where(mask.any(1, keepdim=True), P64, torch.zeros_like(P64))
        chain = bounds[0][:, h] + (L[:, 0] * u) * (P64 @ V[:, h].abs())
        assert bool(((Oh.double() - O64[:, h]).abs() <= chain).all())
        assert bool(((O[:, h].double() - Oh.double()).abs() <= bounds[0][:, h] + chain).all()), h


def test_special_values_on_the_gpu():
    """The CPU test's cases (tests/test_sparse_attention_cpu.py::test_special_values): the same results from the kernels."""
    from torchsparsegradutils_amd import sparse_attention

    inf, nan = float("inf"), float("nan")
    rows = [[0.5, None, 1.0, -0.5], [None, None, None, None], [-inf, -inf, None, -inf], [-inf, 1.0, None, 2.0], [nan, 1.0, 0.0, None],
            [inf, 1.0, None, None]]
    mask = torch.tensor([[v is not None for v in r] for r in rows])
    B = torch.tensor([[0.0 if v is None else v for v in r] for r in rows], dtype=torch.float64)
    g = torch.Generator().manual_seed(6)
    Q, K, V, dO = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((6, 2, 8), (4, 2, 8), (4, 2, 8), (6, 2, 8)))
    for dtype in (torch.float64, torch.float32, torch.bfloat16):
        for layout in ("csr", "csc", "coo"):
            def run(dev):
                A = ar.sparse_from_dense(B, mask, layout, torch.int64, dtype).to(dev).requires_grad_(True)
                q, k, v = (x.to(dtype).to(dev).requires_grad_(True) for x in (Q, K, V))
                O = sparse_attention(A, q, k, v, scale=0.5)
                gA, gq, gk, gv = torch.autograd.grad(O, (A, q, k, v), dO.to(dtype).to(dev))
                return [x.detach().cpu() for x in (O, gq, gk, gv, gA.to_dense() if layout == "coo" else gA.values())]
            got, want = run(DEV), run("cpu")
            rel = {torch.float64: 1e-12, torch.float32: 1e-5, torch.bfloat16: 2.0 ** -6}[dtype]
            for name, a, b in zip(NAMES, got, want):
                assert torch.equal(a.isnan(), b.isnan()), (name, dtype, layout)
                assert torch.allclose(a.double(), b.double(), rtol=rel, atol=rel, equal_nan=True), (name, dtype, layout)
            O, gq = got[0], got[1]
            assert bool((O[1] == 0).all()) and bool((gq[1] == 0).all())
            assert O[2].isnan().all() and O[4].isnan().all() and O[5].isnan().all() and O[0].isfinite().all() and O[3].isfinite().all()


def test_refusal_of_unsupported_geometry_on_the_gpu():
    from torchsparsegradutils_amd import sparse_attention

    A = torch.eye(4, device=DEV).to_sparse_csr()
    for shape in ((4, 12), (4, 9, 128), (4, 256)):
        X = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError, match=re.escape("sparse_attention: the gfx950 kernels take d in {8, 16, 32, 64, 128}, V as wide as "
                                                       "Q and K, and H*d <= 1024, got d=")):
            sparse_attention(A, X, X, X)


def test_through_the_c_abi_directly():
    """The three entries called with ctypes on raw pointers, with row strides larger than heads·d: the stub printed in
    INTEGRATION.md, executed as written (only the library path is filled in)."""
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = next(b for b in re.findall(r"```python\n(.*?)```", text, re.S) if "attention stub" in b)
    code = code.replace('ctypes.CDLL("libtsgu_hip.so")', f'ctypes.CDLL("{_backend.LIB_PATH}")')
    ns = {}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)  # noqa: S102  (our own document)
    heads, d, dtype = 3, 16, torch.float32
    mask, B, Q, K, V, dO = _inputs("short", heads, d, dtype)
    want, bounds = _reference("short", heads, d, dtype)
    n, m = mask.shape
    A = ar.sparse_from_dense(B, mask, "csr", torch.int32, dtype).to(DEV)

    def padded(X):          # rows of heads·d elements inside rows of heads·d + 12 (a multiple of 16 bytes)
        buf = torch.full((X.size(0), heads * d + 12), float("nan"), dtype=dtype, device=DEV)
        buf[:, :heads * d] = X.reshape(X.size(0), -1).to(dtype)
        return buf[:, :heads * d]

    q, k, v, g = padded(Q), padded(K), padded(V), padded(dO)
    assert q.stride(0) == heads * d + 12
    O, lse = ns["attention_forward"](A, q, k, v, heads, d, SCALE[d])
    dQ, dK, dV, dA = ns["attention_backward"](A, ns["transposed_walk"](A), q, k, v, g, lse, heads, d, SCALE[d])
    torch.cuda.synchronize()
    dense = torch.zeros(mask.shape)
    dense[mask] = dA.cpu()
    got = (O.cpu().view(n, heads, d), dQ.cpu().view(n, heads, d), dK.cpu().view(m, heads, d), dV.cpu().view(m, heads, d), dense)
    for name, gt, w, b in zip(NAMES, got, want, bounds):
        if name == "dA":
            gt, w, b = gt[mask], w[mask], b[mask]
        _assert_within(gt, w, b, 0.0, f"{name} through the C ABI")
