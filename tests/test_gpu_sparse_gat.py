"""sparse_gat_attention / sparse_gatv2_attention on the GPU against the dense float64 oracle of tests/_gat_ref.py.

Inputs lie on a grid of 1/32 with magnitude below 4 (att below 1): exact in bfloat16, so one oracle run serves the three dtypes, and
z = s_dst + s_src (X_dst + X_src) is exact in every type — the LeakyReLU takes the same branch, the value 0 included, in the kernel
and in float64.  That is a condition of the test: with continuous operands a float32 z near 0 may take the other branch and the
gradient then differs by (1 − slope)·dS.  Several z are exactly 0 (`_inputs` plants them and asserts it).

Bounds: _gat_ref.error_bounds — the form and constants of _attention_ref.error_bounds (C = 8 forward, 16 gradients, tiny per
stored entry) with the logit error e_j = 3u(|s_dst| + |s_src| + |b_j|) for GAT, (d + 3)u(Σ_k |att_k||z_k| + |b_j|) for GATv2; a sum
of N terms in a fixed order adds N·u·Σ|terms| (N = L for row sums, L'_j for column sums — 2L'_j for dX_src, whose column sum has two
terms per entry — and nnz for datt); a coefficient that is itself rounded (att·slope, slope·z) adds one u; u = 2⁻²⁴ for float32 and
bfloat16, 2⁻⁵³ for float64; every bfloat16 output adds 2⁻⁸·|ref| for its one rounding.  No fitted constants.  bfloat16 results are
also held bit for bit against the float32 results rounded once where the walk is the same: the forward when a workgroup's entries
fit one slice (the slices of the GAT forward start at the workgroup's first entry, and float32 and bfloat16 workgroups own
different numbers of rows), the gradients always given the same lse.
"""

import functools

import numpy as np
import pytest
import torch

import _gat_ref as gr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24}
TINY = {torch.float32: float(np.finfo(np.float32).tiny), torch.float64: float(np.finfo(np.float64).tiny),
        torch.bfloat16: float(np.finfo(np.float32).tiny)}
WIDTHS = [(1, 8), (3, 16), (2, 128), (3, 128), (128, 8)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _geometry(kind, dtype, heads, d):
    from torchsparsegradutils_amd import _backend

    return _backend.gat_geometry(dtype, kind, heads, d)


def _fn(kind):
    import torchsparsegradutils_amd as pkg

    return pkg.sparse_gat_attention if kind == "gat" else pkg.sparse_gatv2_attention


def _rows_mask(lengths, m, gen):
    mask = torch.zeros((len(lengths), m), dtype=torch.bool)
    for i, L in enumerate(lengths):
        mask[i, torch.randperm(m, generator=gen)[:L]] = True
    return mask


@functools.lru_cache(maxsize=None)
def _inputs(kind, heads, d, mask_key, batch=None):
    """(mask, B, a, b, c, dO) in float64 on the grid, with z = 0 exactly at the last stored entry of a few rows."""
    mask = _MASKS[mask_key[0]](*mask_key[1:])
    n, m = mask.shape
    gen = torch.Generator().manual_seed(5)
    lead = () if batch is None else (batch,)
    if kind == "gat":
        shapes = (lead + (n, heads), lead + (m, heads), lead + (m, heads, d))
    else:
        shapes = (lead + (n, heads, d), lead + (m, heads, d), (heads, d))
    B, dO = gr.grid(lead + (n, m), gen), gr.grid(lead + (n, heads, d), gen)
    a, b = gr.grid(shapes[0], gen, 1), gr.grid(shapes[1], gen, 3)           # |z| < 4, and both signs are likely in a row
    c = gr.grid(shapes[2], gen, 4 if kind == "gat" else 1)
    rows = [i for i in range(n) if mask[i].any()][:6]
    for i in rows:
        j = int(mask[i].nonzero()[-1])
        if kind == "gat":
            b[..., j, :] = -a[..., i, :]
        else:
            b[..., j, :, ::2] = -a[..., i, :, ::2]
    # the condition of the test, on the oracle's inputs: exact zeros, and both signs in every row of some length
    a0, b0 = (a, b) if batch is None else (a[0], b[0])
    zeros = sum(int((a0[i] + b0[int(mask[i].nonzero()[-1])] == 0).sum()) for i in rows)
    assert zeros >= min(3, len(rows)), "several z must be exactly 0"
    for i in range(n):
        if int(mask[i].sum()) >= 32:
            z = a0[i].unsqueeze(0) + b0[mask[i]]
            assert bool((z > 0).any()) and bool((z < 0).any()), f"row {i}: both signs of z must occur"
    return mask, B, a, b, c, dO


@functools.lru_cache(maxsize=None)
def _reference(kind, heads, d, mask_key, slope, acc_dtype, grads):
    """(oracle results, bounds) in float64: computed once per case and arithmetic, shared, never changed."""
    mask, B, a, b, c, dO = _inputs(kind, heads, d, mask_key)
    ref = gr.dense_oracle(kind, mask, B, a, b, c, dO, slope)
    return ref, gr.error_bounds(kind, mask, B, a, b, c, dO, slope, True, U[acc_dtype], TINY[acc_dtype], ref, grads)


def _check(name, got, want, bound, dtype):
    """|got − want| <= bound (+ 2⁻⁸|want| for a bfloat16 output); the figure is printed before it is asserted."""
    got, allow = got.detach().double().cpu().reshape(want.shape), bound + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)
    err = (got - want).abs()
    worst = float((err / allow.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max error {float(err.max()) if err.numel() else 0.0:.3e}, {worst:.3f} of the allowance")
    assert bool((err <= allow).all()), f"{name}: {worst:.3f} of the allowance"


def _structural(kind, dtype, heads, d):
    R, S, _ = _geometry(kind, dtype, heads, d)
    lengths = [0, 1, S - 1, S, S + 1, 2 * S + 1]
    lengths += [2] * (-len(lengths) % R)                       # the run below starts a workgroup
    lengths += [S // R + 1] * R                                # R rows that together overflow one slice
    lengths += [3, 2, 5, 0, 0]
    return _rows_mask(lengths, 2 * S + 8, torch.Generator().manual_seed(11))


def _row_count(n):
    return _rows_mask(torch.randint(0, 12, (n,), generator=torch.Generator().manual_seed(n)).tolist(), 29, torch.Generator().manual_seed(7))


def _hub(S):
    """S + 8 rows and columns: a hub column and one row longer than a slice, short rows, empty rows and columns."""
    n = S + 8
    gen = torch.Generator().manual_seed(13)
    mask = _rows_mask(torch.randint(1, 6, (n,), generator=gen).tolist(), n, gen)
    mask[3, : S + 1] = True
    mask[:, 0] = True
    mask[[5, 77]] = False
    mask[:, 7] = False
    return mask


def _small():
    mask = torch.rand((37, 29), generator=torch.Generator().manual_seed(3)) < 0.25
    mask[4] = False
    mask[:, 6] = False
    mask[9, :] = True
    mask[9, 6] = False
    return mask


_MASKS = {"structural": _structural, "rows": _row_count, "hub": _hub, "small": _small}


def _csr_arrays(mask, B, index_dtype, dtype):
    crow = torch.zeros(mask.size(0) + 1, dtype=torch.int64)
    crow[1:] = mask.sum(1).cumsum(0)
    return crow.to(index_dtype).to(DEV), mask.nonzero()[:, 1].to(index_dtype).to(DEV), B[mask].to(dtype).to(DEV)


def _forward_entry(kind, dtype, heads, d, mask_key, index_dtype, slope):
    """O of the backend's forward entry on the case's CSR arrays."""
    from torchsparsegradutils_amd import _backend

    mask, B, a, b, c, _ = _inputs(kind, heads, d, mask_key)
    crow, col, val = _csr_arrays(mask, B, index_dtype, dtype)
    a, b, c = (x.to(dtype).to(DEV) for x in (a, b, c))
    n, m = mask.shape
    if kind == "gat":
        O, lse = _backend.csr_gat_forward(kind, (crow, col, None), val, a, b, None, c.view(m, -1), None, heads, d, slope)
    else:
        O, lse = _backend.csr_gat_forward(kind, (crow, col, None), val, None, None, a.view(n, -1), b.view(m, -1), c.reshape(-1), heads, d, slope)
    assert lse.shape == (n, heads) and lse.dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    return O.view(n, heads, d)


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("heads,d,index_dtype", [w + (torch.int32,) for w in WIDTHS] + [(3, 16, torch.int64)], ids=str)
def test_structural_matrix_forward(kind, dtype, heads, d, index_dtype):
    key = ("structural", kind, dtype, heads, d)
    O = _forward_entry(kind, dtype, heads, d, key, index_dtype, 0.2)
    ref, bounds = _reference(kind, heads, d, key, 0.2, dtype, False)
    _check("O", O, ref["O"], bounds["O"], dtype)


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("which", ["one", "R-1", "R", "R+1"])
def test_row_counts_around_a_workgroup(kind, which):
    heads, d = 2, 16
    res = {}
    for dtype in DTYPES:
        R = _geometry(kind, dtype, heads, d)[0]
        n = {"one": 1, "R-1": R - 1, "R": R, "R+1": R + 1}[which]
        if n < 1:
            continue
        key = ("rows", n)
        res[dtype, n] = O = _forward_entry(kind, dtype, heads, d, key, torch.int32, 0.25)
        ref, bounds = _reference(kind, heads, d, key, 0.25, dtype, False)
        _check(f"O {dtype} n={n}", O, ref["O"], bounds["O"], dtype)
    # every workgroup's entries fit one slice here: bfloat16 walks as float32 does, and rounds once
    for (dtype, n), O in res.items():
        if dtype == torch.bfloat16:
            O32 = res.get((torch.float32, n))
            if O32 is None:
                O32 = _forward_entry(kind, torch.float32, heads, d, ("rows", n), torch.int32, 0.25)
            assert gr.same_bits(O, O32.to(torch.bfloat16))


def _public(kind, dtype, heads, d, mask_key, layout, slope, batch=None, index_dtype=torch.int32, use_bias=True, B=None):
    """(O, da, db, dc, dA as the gradient's value array, A) through the public function."""
    mask, B0, a, b, c, dO = _inputs(kind, heads, d, mask_key, batch)
    A = gr.sparse_from_dense(B0 if B is None else B, mask, layout, index_dtype, dtype).to(DEV).requires_grad_(True)
    xa, xb, xc = (x.to(dtype).to(DEV).requires_grad_(True) for x in (a, b, c))
    O = _fn(kind)(A, xa, xb, xc, negative_slope=slope, values_as_bias=use_bias)
    gA, ga, gb, gc = torch.autograd.grad(O, (A, xa, xb, xc), dO.to(dtype).to(DEV), allow_unused=True)
    return O.detach(), ga, gb, gc, gA, A


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_gradients_on_a_hub_matrix(kind, dtype):
    heads, d = 1, 8
    S = max(_geometry(kind, t, heads, d)[1] for t in DTYPES)
    key = ("hub", S)
    O, da, db, dc, gA, A = _public(kind, dtype, heads, d, key, "csr", 0.2)
    ref, bounds = _reference(kind, heads, d, key, 0.2, torch.float64 if dtype == torch.float64 else torch.float32, True)
    for name, got in (("O", O), ("da", da), ("db", db), ("dc", dc)):
        _check(name, got, ref[name], bounds[name], dtype)
    assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and gA.col_indices().data_ptr() == A.col_indices().data_ptr()
    assert gA.col_indices().dtype == torch.int32
    _check("dA", gA.values(), gr.stored_order(ref["dB"], A.detach().cpu()), gr.stored_order(bounds["dB"], A.detach().cpu()), dtype)
    if dtype == torch.bfloat16:     # the backward's sums do not depend on the slices: bfloat16 is float32 rounded once, given the lse
        ref32 = _public(kind, torch.float32, heads, d, key, "csr", 0.2)
        if gr.same_bits(O, ref32[0].to(dtype)):
            for got, want in zip((da, db, dc, gA.values()), (*ref32[1:4], ref32[4].values())):
                assert gr.same_bits(got, want.to(dtype))


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("layout", ["csr", "csc", "coo", "coo_uncoalesced", "batched"])
def test_layouts(kind, dtype, layout):
    heads, d, key = 3, 16, ("small",)
    batch = 2 if layout == "batched" else None
    slope = 0.0 if layout == "coo" else 0.25
    O, da, db, dc, gA, A = _public(kind, dtype, heads, d, key, "csr" if batch else layout, slope, batch,
                                   torch.int64 if layout == "csc" else torch.int32)
    mask, B, a, b, c, dO = _inputs(kind, heads, d, key, batch)
    acc = torch.float64 if dtype == torch.float64 else torch.float32
    items = []
    for i in (range(batch) if batch else [None]):
        pick = (lambda x: x if i is None else x[i])
        args = (kind, mask, pick(B), pick(a), pick(b), c if kind == "gatv2" else pick(c), pick(dO), slope)
        ref = gr.dense_oracle(*args)
        items.append((ref, gr.error_bounds(*args, True, U[acc], TINY[acc], ref)))
    join = (lambda k, w: torch.stack([it[w][k] for it in items]) if batch else items[0][w][k])
    for name, got in (("O", O), ("da", da), ("db", db), ("dc", dc)):
        want, bound = join(name, 0), join(name, 1)
        if batch and kind == "gatv2" and name == "dc":
            want, bound = want.sum(0), bound.sum(0) + batch * U[acc] * want.abs().sum(0)
        _check(name, got, want, bound, dtype)
    Ac = A.detach().cpu()
    if layout == "coo_uncoalesced":
        Ac, gA = Ac.coalesce(), gA.coalesce()
    else:
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(gr.index_tensors(gA), gr.index_tensors(A)))
    _check("dA", gr.values_of(gA), gr.stored_order(join("dB", 0), Ac), gr.stored_order(join("dB", 1), Ac), dtype)


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("case", ["ninf_beside", "only_ninf", "pinf", "nan", "empty_row", "no_bias"])
def test_special_values(kind, case):
    heads, d, key, dtype = 2, 8, ("small",), torch.float32
    mask, B, a, b, c, dO = _inputs(kind, heads, d, key)
    base = _public(kind, dtype, heads, d, key, "csr", 0.2)
    row = 9                                                    # the full row of the mask
    cols = mask[row].nonzero().flatten()
    others = torch.arange(mask.size(0)) != row
    B2 = B.clone()
    if case == "empty_row":
        O, da = base[0], base[1]
        assert not O[4].any() and not da[4].any(), "a row without stored entries gives zeros and zero gradients"
        return
    if case == "no_bias":
        got = _public(kind, dtype, heads, d, key, "csr", 0.2, use_bias=False, B=B * float("nan"))
        zero = _public(kind, dtype, heads, d, key, "csr", 0.2, B=B * 0)
        assert got[4] is None, "A gets no gradient"
        for x, y in zip(got[:4], zero[:4]):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)
        return
    if case == "ninf_beside":
        B2[row, cols[1]] = float("-inf")
        got = _public(kind, dtype, heads, d, key, "csr", 0.2, B=B2)
        mask2 = mask.clone()
        mask2[row, cols[1]] = False                            # weight 0: the entry might as well be absent
        ref = gr.dense_oracle(kind, mask2, B, a, b, c, dO, 0.2)
        bounds = gr.error_bounds(kind, mask2, B, a, b, c, dO, 0.2, True, U[dtype], TINY[dtype], ref)
        for name, x in zip(("O", "da", "db", "dc"), got[:4]):
            _check(name, x, ref[name], bounds[name], dtype)
        dA = torch.zeros(mask.shape)
        dA[mask] = got[4].values().cpu()
        assert float(dA[row, cols[1]]) == 0.0, "gradient 0 at the -inf entry"
        return
    B2[row, cols if case == "only_ninf" else cols[2]] = {"only_ninf": float("-inf"), "pinf": float("inf"), "nan": float("nan")}[case]
    got = _public(kind, dtype, heads, d, key, "csr", 0.2, B=B2)
    assert bool(got[0][row].isnan().all()), "the row is NaN for every head"
    assert np.array_equal(got[0].cpu().numpy()[others], base[0].cpu().numpy()[others], equal_nan=True), "the other rows are untouched"
    assert np.array_equal(got[1].cpu().numpy()[others], base[1].cpu().numpy()[others], equal_nan=True)


def test_datt_is_reproducible():
    heads, d = 3, 16
    key = ("rows", 4 * _geometry("gatv2", torch.float32, heads, d)[0] + 1)       # several workgroups' shares
    first = _public("gatv2", torch.float32, heads, d, key, "csr", 0.2)[3]
    again = _public("gatv2", torch.float32, heads, d, key, "csr", 0.2)[3]
    assert gr.same_bits(first, again)
