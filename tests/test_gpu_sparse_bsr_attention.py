"""sparse_bsr_attention on the GPU against the dense float64 oracle on the CPU (tests/_attention_ref.py), given exactly the rounded
inputs.  Operands are built on the CPU; the block mask is expanded to an element mask for the oracle.

Structural cases, sized from the kernels' own constants (`_backend.bsr_attention_geometry`: T rows per workgroup, S keys per LDS
stage): blocks (16,16), (16,64), (64,16), (T,T), (2T,32) (pieces of a block row) and (32,S+16) (a block wider than a stage); per
block size block rows of 0, 1, c−1, c, c+1 and 2c+1 blocks with c = ⌈S/bw⌉; for bh < T a number of block rows of T/bh − 1, T/bh and
T/bh + 1 (the last workgroup is partial); block column 0 is a hub that every non-empty block row references (the column pass walks
it stage after stage), the last block column is referenced by none, and the block columns of a row are stored unsorted.

Bounds (derived, not measured): tests/_attention_ref.py::error_bounds with u = 2^-24 / 2^-53 and
ρ_j = e_j + Σ_l p_l e_l + (3L + |t_j − max t| + C) u, C = 8 (16 for the gradients).  How the kernels' order (csrc/bsr_attention_impl.h)
meets the 3L + C, L being the row's length (a multiple of the block width, so L >= 16):
  * the logit is an MFMA dot of d terms — for float32 / float64 bit for bit a k-ordered fma chain, d roundings — then one
    multiplication by scale and one addition of the bias: e_j = (d + 2) u a_j;
  * a probability costs one subtraction (t − m: rounds |t_j − max t| u in the exponent, as the rescaling exps telescope because
    the running maximum only rises) and one exp;
  * the row sum l: a stage's S terms are summed by 256/T lanes (S·T/256 − 1 additions along a lane, log2(256/T) butterfly steps),
    then one rescale and one addition per stage: at most S/4 + 3 + 2⌈L/S⌉ roundings, below L + 8 for L >= 16 and S <= 64;
  * O: the factor exp(m_old − m_new) is the SAME number for l and for the accumulator, so its own error cancels in O / l; what
    stays is one multiplication per stage (⌈L/S⌉ roundings) and the MFMA chain of P·V, L roundings: L + ⌈L/S⌉;
  * the final division, and in the backward exp(t − lse) with lse = m + log l, are in the constants 8 and 16.
  Together at most 2L + 3⌈L/S⌉ + S/4 + C' <= 3L + C for L >= 16.  The gradient sums run over a column's L'_j entries in MFMA chains
  (dK, dV: (L'_j + d) u and L'_j u) and over the row's (dQ: within ρ); δ = <dO, O> from the forward's unrounded O is the
  d·u·Σ|dO||O| term of δ̄; dA adds H terms: H u.
bfloat16: the float32 bound, plus 2^-8 |oracle| for the final store, plus the roundings of P and dS to bfloat16 (2^-9 relative each)
before P·V, Pᵀ·dO, dS·K and dSᵀ·Q:  O: 2^-9 Σ_j p_j |v_jc|,  dV: 2^-9 Σ_i p_ij |dO_ic|,  dQ: 2^-9 |scale| Σ_j dS̄_ij |k_jc|,
dK: 2^-9 |scale| Σ_i dS̄_ij |q_ic|, with dS̄ as in error_bounds.
"""

import functools
import re
import warnings

import numpy as np
import pytest
import torch

import _attention_ref as ar

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
TINY = {torch.float32: float(np.finfo(np.float32).tiny), torch.float64: float(np.finfo(np.float64).tiny)}
GEOMETRIES = [(1, 16), (3, 32), (2, 64), (2, 128)]
NAMES = ("O", "dQ", "dK", "dV", "dA")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _geometry(dtype, heads, d):
    from torchsparsegradutils_amd import _backend

    return _backend.bsr_attention_geometry(dtype, heads, d, 16, 16)


def _blocks(T, S):
    return [(16, 16), (16, 64), (64, 16), (T, T), (2 * T, 32), (32, S + 16)]


def _pattern(lens, ncb, seed, hub=True):
    """(crow, col) with the given block-row lengths: distinct random block columns below ncb − 1 (the last is referenced by none),
    block column 0 in every non-empty row when `hub`, stored in random (unsorted) order."""
    gen = torch.Generator().manual_seed(seed)
    crow, col = [0], []
    for L in lens:
        if L:
            if hub:
                rest = (torch.randperm(ncb - 2, generator=gen)[:L - 1] + 1).tolist()
                cols = [0] + rest
            else:
                cols = torch.randperm(ncb - 1, generator=gen)[:L].tolist()
            col += [cols[i] for i in torch.randperm(L, generator=gen).tolist()]
        crow.append(len(col))
    return torch.tensor(crow), torch.tensor(col, dtype=torch.int64)


def _block_rows(crow):
    return torch.repeat_interleave(torch.arange(crow.numel() - 1), crow[1:] - crow[:-1]).tolist()


def _to_dense(crow, col, blocks, ncb):
    """(mask, dense) of the stored blocks [nnzb, bh, bw] (no repeated (I, J))."""
    bh, bw = blocks.shape[1:]
    n, m = (crow.numel() - 1) * bh, ncb * bw
    mask, D = torch.zeros((n, m), dtype=torch.bool), torch.zeros((n, m), dtype=blocks.dtype)
    for e, (i, j) in enumerate(zip(_block_rows(crow), col.tolist())):
        assert not mask[i * bh, j * bw]
        mask[i * bh:(i + 1) * bh, j * bw:(j + 1) * bw] = True
        D[i * bh:(i + 1) * bh, j * bw:(j + 1) * bw] = blocks[e]
    return mask, D


def _to_blocks(crow, col, D, bh, bw):
    out = [D[i * bh:(i + 1) * bh, j * bw:(j + 1) * bw] for i, j in zip(_block_rows(crow), col.tolist())]
    return torch.stack(out) if out else torch.zeros((0, bh, bw), dtype=D.dtype)


def _randn(shape, seed, dtype):
    """N(0, 1) rounded to `dtype`, as float64: the oracle gets exactly what the kernels get."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).to(dtype).double()


def _run(crow, col, blocks, ncb, Q, K, V, dO, dtype, index_dtype, scale, use_bias=True):
    """(O, dQ, dK, dV, dA blocks) of the operator under test on the GPU; the inputs are float64 tensors on the CPU."""
    from torchsparsegradutils_amd import sparse_bsr_attention

    bh, bw = blocks.shape[-2:]
    shape = tuple(blocks.shape[:-3]) + ((crow.size(-1) - 1) * bh, ncb * bw)
    ci, cj = crow.to(index_dtype).to(DEV), col.to(index_dtype).to(DEV)
    A = torch.sparse_bsr_tensor(ci, cj, blocks.to(dtype).to(DEV), shape).requires_grad_(True)
    q, k, v = (x.to(dtype).to(DEV).requires_grad_(True) for x in (Q, K, V))
    O = sparse_bsr_attention(A, q, k, v, scale=scale, values_as_bias=use_bias)
    assert O.shape == q.shape and O.dtype == dtype
    if not use_bias:
        dq, dk, dv = torch.autograd.grad(O, (q, k, v), dO.to(dtype).to(DEV))
        (none,) = torch.autograd.grad(sparse_bsr_attention(A, q, k, v, scale=scale, values_as_bias=False).sum(), (A,), allow_unused=True)
        assert none is None
        return O.detach().cpu(), dq.cpu(), dk.cpu(), dv.cpu(), None
    dA, dq, dk, dv = torch.autograd.grad(O, (A, q, k, v), dO.to(dtype).to(DEV))
    assert dA.layout == torch.sparse_bsr and dA.dtype == dtype and dA.shape == A.shape
    assert dA.crow_indices().data_ptr() == A.crow_indices().data_ptr() and dA.col_indices().data_ptr() == A.col_indices().data_ptr()
    assert dA.col_indices().dtype == index_dtype
    return O.detach().cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dA.values().cpu()


def _assert_within(got, want, bound, extra, what):
    print(f"{what}: max |err| / bound = {float(((got.double() - want).abs() / (bound + extra).clamp(min=1e-300)).max()):.3g}")
    assert torch.equal(got.isnan(), want.isnan()), what
    assert bool(((got.double() - want).abs() <= bound + extra).all()), what


@functools.lru_cache(maxsize=None)
def _case(heads, d, dtype, block, lens, seed=3):
    """One structural case with its oracle results and bounds, computed once and shared by the index types; never changed."""
    bh, bw = block
    ncb = max(lens) + 2
    crow, col = _pattern(lens, ncb, seed)
    n, m = len(lens) * bh, ncb * bw
    blocks = _randn((col.numel(), bh, bw), 5, dtype)
    Q, K, V, dO = (_randn(s, 6 + i, dtype) for i, s in enumerate(((n, heads, d), (m, heads, d), (m, heads, d), (n, heads, d))))
    mask, B = _to_dense(crow, col, blocks, ncb)
    scale = d ** -0.5
    O, dQ, dK, dV, dB, P = ar.dense_oracle(mask, B, Q, K, V, dO, scale)
    acc = torch.float32 if dtype == torch.bfloat16 else dtype
    bounds = ar.error_bounds(mask, B, Q, K, V, dO, scale, True, U[acc], TINY[acc], P, O)
    extra = None
    if dtype == torch.bfloat16:
        Va, Ka, Qa, Ga = V.abs(), K.abs(), Q.abs(), dO.abs()
        dPb = torch.einsum("ihd,jhd->hij", Ga, Va)
        db = (P * dPb).sum(-1, keepdim=True) + d * U[acc] * (Ga * O.abs()).sum(-1).t().unsqueeze(-1)
        dSb = P * (dPb + db)
        h = 2.0 ** -9
        extra = (h * torch.einsum("hij,jhd->ihd", P, Va), h * abs(scale) * torch.einsum("hij,jhd->ihd", dSb, Ka),
                 h * abs(scale) * torch.einsum("hij,ihd->jhd", dSb, Qa), h * torch.einsum("hij,ihd->jhd", P, Ga), torch.zeros_like(B))
    want = (O, dQ, dK, dV, dB)
    return dict(crow=crow, col=col, ncb=ncb, blocks=blocks, Q=Q, K=K, V=V, dO=dO, mask=mask, scale=scale, want=want, bounds=bounds,
                extra=extra)


def _check_case(c, dtype, index_dtype, what):
    bh, bw = c["blocks"].shape[1:]
    got = list(_run(c["crow"], c["col"], c["blocks"], c["ncb"], c["Q"], c["K"], c["V"], c["dO"], dtype, index_dtype, c["scale"]))
    got[4] = _to_dense(c["crow"], c["col"], got[4], c["ncb"])[1]
    mask = c["mask"]
    for k, (name, g, w, b) in enumerate(zip(NAMES, got, c["want"], c["bounds"])):
        x = 0.0 if c["extra"] is None else c["extra"][k] + 2.0 ** -8 * w.abs()
        if name == "dA":
            g, w, b = g[mask], w[mask], b[mask]
            x = x if c["extra"] is None else x[mask]
        _assert_within(g, w, b, x, f"{name} {what}")
    assert bool((got[0][~mask.any(1)] == 0).all()) and bool((got[1][~mask.any(1)] == 0).all())      # block rows without blocks
    assert bool((got[2][~mask.any(0)] == 0).all()) and bool((got[3][~mask.any(0)] == 0).all())      # unreferenced block columns
    return got


def _lens(S, bw):
    c = -(-S // bw)
    return tuple(dict.fromkeys(x for x in (0, 1, c - 1, c, c + 1, 2 * c + 1) if x >= 0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("heads,d", GEOMETRIES, ids=[f"H{h}d{d}" for h, d in GEOMETRIES])
def test_structural_cases_within_the_bounds(heads, d, dtype):
    T, S = _geometry(dtype, heads, d)
    for block in _blocks(T, S):
        c = _case(heads, d, dtype, block, _lens(S, block[1]))
        assert c["bounds"][5] < 2.0 ** -10, "the first-order bound needs max rho < 2^-10"
        assert int(c["mask"].sum(1).max()) <= 1200
        for index_dtype in (torch.int32, torch.int64):
            _check_case(c, dtype, index_dtype, f"{block} H{heads} d{d} {dtype} {index_dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_partial_last_workgroup(dtype):
    """T/bh − 1, T/bh and T/bh + 1 block rows of blocks lower than a tile."""
    heads, d = 2, 32
    T, S = _geometry(dtype, heads, d)
    for block in ((16, 16), (16, 64)):
        per = T // block[0]
        for nbr in (per - 1, per, per + 1):
            lens = tuple(1 + i % 3 for i in range(nbr))
            c = _case(heads, d, dtype, block, lens, seed=20 + nbr)
            assert c["bounds"][5] < 2.0 ** -10
            _check_case(c, dtype, torch.int32, f"{block} x {nbr} block rows {dtype}")


@pytest.mark.parametrize("heads,d", GEOMETRIES, ids=[f"H{h}d{d}" for h, d in GEOMETRIES])
def test_bfloat16_within_the_float32_bound_and_its_operand_roundings(heads, d):
    T, S = _geometry(torch.bfloat16, heads, d)
    for block in _blocks(T, S):
        c = _case(heads, d, torch.bfloat16, block, _lens(S, block[1]))
        assert c["bounds"][5] < 2.0 ** -10
        _check_case(c, torch.bfloat16, torch.int32, f"{block} H{heads} d{d} bf16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_a_bias_spread_over_80_underflows_inside_rows(dtype):
    heads, d, bh, bw, ncb = 2, 32, 16, 64, 11
    lens = (10, 3, 0, 7)
    crow, col = _pattern(lens, ncb, 9)
    n, m = len(lens) * bh, ncb * bw
    blocks = (_randn((col.numel(), bh, bw), 5, torch.float64) * 40 / 3).clamp(-40, 40).to(dtype).double()
    Q, K, V, dO = (_randn(s, 6 + i, dtype) for i, s in enumerate(((n, heads, d), (m, heads, d), (m, heads, d), (n, heads, d))))
    mask, B = _to_dense(crow, col, blocks, ncb)
    assert int(mask.sum(1).max()) == 640 and float(blocks.max()) == 40 and float(blocks.min()) == -40
    scale = d ** -0.5
    O, dQ, dK, dV, dB, P = ar.dense_oracle(mask, B, Q, K, V, dO, scale)
    bounds = ar.error_bounds(mask, B, Q, K, V, dO, scale, True, U[dtype], TINY[dtype], P, O)
    assert bounds[5] < 2.0 ** -10
    c = dict(crow=crow, col=col, ncb=ncb, blocks=blocks, Q=Q, K=K, V=V, dO=dO, mask=mask, scale=scale, want=(O, dQ, dK, dV, dB),
             bounds=bounds, extra=None)
    _check_case(c, dtype, torch.int32, f"spread {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# semantics


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_block_causal_with_minus_inf_in_the_diagonal_blocks(dtype):
    """A -inf inside a stored block masks the element: the result is the oracle's on the mask without those elements."""
    heads, d, b, nb = 2, 32, 16, 5
    crow = torch.tensor([0, 1, 3, 6, 10, 15])
    col = torch.tensor([0, 1, 0, 0, 2, 1, 3, 0, 1, 2, 0, 1, 2, 3, 4])
    blocks = _randn((15, b, b), 5, dtype)
    upper = torch.triu(torch.ones(b, b, dtype=torch.bool), 1)
    for e, (i, j) in enumerate(zip(_block_rows(crow), col.tolist())):
        if i == j:
            blocks[e][upper] = float("-inf")
    Q, K, V, dO = (_randn((nb * b, heads, d), 6 + i, dtype) for i in range(4))
    mask, B = _to_dense(crow, col, blocks, nb)
    live = mask & B.isfinite()
    assert torch.equal(live, torch.tril(torch.ones(nb * b, nb * b, dtype=torch.bool)))
    Bf = B.masked_fill(~live, 0.0)
    scale = d ** -0.5
    O, dQ, dK, dV, dB, P = ar.dense_oracle(live, Bf, Q, K, V, dO, scale)
    bounds = ar.error_bounds(live, Bf, Q, K, V, dO, scale, True, U[dtype], TINY[dtype], P, O)
    got = list(_run(crow, col, blocks, nb, Q, K, V, dO, dtype, torch.int32, scale))
    got[4] = _to_dense(crow, col, got[4], nb)[1]
    assert bool((got[4][mask & ~live] == 0).all())                       # -inf beside finite logits: gradient 0
    for name, g, w, bd in zip(NAMES, got, (O, dQ, dK, dV, dB), bounds):
        if name == "dA":
            g, w, bd = g[live], w[live], bd[live]
        _assert_within(g, w, bd, 0.0, f"{name} causal {dtype}")


def test_a_row_of_only_minus_inf_is_nan_in_that_head_only():
    heads, d, b = 2, 32, 16
    crow, col = torch.tensor([0, 2, 3]), torch.tensor([1, 0, 1])
    for dtype in (torch.float32, torch.float64, torch.bfloat16):
        blocks = _randn((3, b, b), 5, dtype)
        Q, K, V, dO = (_randn((2 * b, heads, d), 6 + i, dtype) for i in range(4))
        clean = _run(crow, col, blocks, 2, Q, K, V, dO, dtype, torch.int32, 0.25)
        blocks[0][5] = float("-inf")
        blocks[1][5] = float("-inf")                                     # row 5: nothing but -inf, in every head (the bias is shared)
        K2 = K.clone()
        got = _run(crow, col, blocks, 2, Q, K2, V, dO, dtype, torch.int32, 0.25)
        assert got[0][5].isnan().all() and got[1][5].isnan().all()
        rest = [i for i in range(2 * b) if i != 5]
        assert torch.equal(got[0][rest], clean[0][rest]) and torch.equal(got[1][rest], clean[1][rest])
        # one head only: a +inf logit through Q·K in head 1 of row 20
        Qi = Q.clone()
        Qi[20, 1] = float("inf")
        one = _run(crow, col, _randn((3, b, b), 5, dtype), 2, Qi, K, V, dO, dtype, torch.int32, 0.25)
        assert one[0][20, 1].isnan().all() and one[0][20, 0].isfinite().all() and torch.equal(one[0][rest[:19]], clean[0][rest[:19]])


def test_values_as_bias_false_is_a_zero_bias_without_a_gradient():
    heads, d, block = 3, 32, (16, 64)
    for dtype in (torch.float32, torch.bfloat16):
        c = _case(heads, d, dtype, block, (2, 0, 3, 1))
        args = (c["crow"], c["col"])
        rest = (c["ncb"], c["Q"], c["K"], c["V"], c["dO"], dtype, torch.int32, c["scale"])
        off = _run(*args, c["blocks"], *rest, use_bias=False)
        zero = _run(*args, torch.zeros_like(c["blocks"]), *rest)
        assert off[4] is None
        for a, b in zip(off[:4], zero[:4]):
            assert torch.equal(a, b)


def test_a_repeated_block_is_two_sets_of_entries():
    """Block row 0 stores (0, 1) twice: the result is that of a matrix with one more block column whose K / V rows copy block column
    1; dK and dV of block column 1 are the sums of the two, and each stored block has its own dA."""
    heads, d, bh, bw, ncb = 2, 32, 16, 32, 4
    dtype = torch.float64
    crow, col = torch.tensor([0, 3, 5]), torch.tensor([1, 3, 1, 0, 2])
    ext = torch.tensor([1, 3, 4, 0, 2])
    blocks = _randn((5, bh, bw), 5, dtype)
    Q, dO = _randn((2 * bh, heads, d), 6, dtype), _randn((2 * bh, heads, d), 7, dtype)
    K, V = _randn((ncb * bw, heads, d), 8, dtype), _randn((ncb * bw, heads, d), 9, dtype)
    Ke, Ve = torch.cat([K, K[bw:2 * bw]]), torch.cat([V, V[bw:2 * bw]])
    mask, B = _to_dense(crow, ext, blocks, ncb + 1)
    scale = d ** -0.5
    O, dQ, dK, dV, dB, P = ar.dense_oracle(mask, B, Q, Ke, Ve, dO, scale)
    bO, bQ, bK, bV, bA, rho = ar.error_bounds(mask, B, Q, Ke, Ve, dO, scale, True, U[dtype], TINY[dtype], P, O)
    fold = lambda X: torch.cat([X[:bw], X[bw:2 * bw] + X[ncb * bw:], X[2 * bw:ncb * bw]])          # noqa: E731
    got = _run(crow, col, blocks, ncb, Q, K, V, dO, dtype, torch.int64, scale)
    _assert_within(got[0], O, bO, 0.0, "O repeated")
    _assert_within(got[1], dQ, bQ, 0.0, "dQ repeated")
    _assert_within(got[2], fold(dK), fold(bK), 0.0, "dK repeated")
    _assert_within(got[3], fold(dV), fold(bV), 0.0, "dV repeated")
    _assert_within(got[4], _to_blocks(crow, ext, dB, bh, bw), _to_blocks(crow, ext, bA, bh, bw), 0.0, "dA repeated")
    assert not torch.equal(got[4][0], got[4][2])


# ---------------------------------------------------------------------------------------------------------------------------
# consistency


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=["f32", "f64", "bf16"])
def test_run_to_run_and_index_type_bit_equality(dtype):
    heads, d = 2, 64
    T, S = _geometry(dtype, heads, d)
    c = _case(heads, d, dtype, (16, 16), _lens(S, 16))
    args = (c["crow"], c["col"], c["blocks"], c["ncb"], c["Q"], c["K"], c["V"], c["dO"], dtype)
    first = _run(*args, torch.int32, c["scale"])
    for other in (_run(*args, torch.int32, c["scale"]), _run(*args, torch.int64, c["scale"])):
        for name, a, b in zip(NAMES, first, other):
            assert torch.equal(a, b), name


def test_the_same_block_row_first_and_last_gives_the_same_bits():
    heads, d, bh, bw, ncb = 2, 32, 16, 32, 6
    for dtype in (torch.float32, torch.bfloat16):
        own = [3, 0, 4]
        crow = torch.tensor([0, 3, 4, 6, 8, 9, 12])
        col = torch.tensor(own + [1] + [2, 0] + [5, 1] + [0] + own)
        blocks = _randn((12, bh, bw), 5, dtype)
        blocks[9:12] = blocks[0:3]
        Q, dO = _randn((6 * bh, heads, d), 6, dtype), _randn((6 * bh, heads, d), 7, dtype)
        Q[5 * bh:], dO[5 * bh:] = Q[:bh], dO[:bh]
        K, V = _randn((ncb * bw, heads, d), 8, dtype), _randn((ncb * bw, heads, d), 9, dtype)
        got = _run(crow, col, blocks, ncb, Q, K, V, dO, dtype, torch.int32, d ** -0.5)
        assert torch.equal(got[0][:bh], got[0][5 * bh:]) and torch.equal(got[1][:bh], got[1][5 * bh:])
        assert torch.equal(got[4][0:3], got[4][9:12])


def test_a_batched_operand_equals_its_items_one_by_one():
    heads, d, bh, bw, ncb, b = 2, 32, 16, 32, 5, 3
    for dtype in (torch.float32, torch.bfloat16):
        items = [_pattern(L, ncb, 30 + i, hub=False) for i, L in enumerate(((2, 0, 3, 1), (0, 4, 1, 1), (3, 1, 1, 1)))]
        blocks = _randn((b, 6, bh, bw), 5, dtype)
        Q, dO = _randn((b, 4 * bh, heads, d), 6, dtype), _randn((b, 4 * bh, heads, d), 7, dtype)
        K, V = _randn((b, ncb * bw, heads, d), 8, dtype), _randn((b, ncb * bw, heads, d), 9, dtype)
        crow, col = torch.stack([c for c, _ in items]), torch.stack([c for _, c in items])
        whole = _run(crow, col, blocks, ncb, Q, K, V, dO, dtype, torch.int32, d ** -0.5)
        for i in range(b):
            one = _run(crow[i], col[i], blocks[i], ncb, Q[i], K[i], V[i], dO[i], dtype, torch.int32, d ** -0.5)
            for name, w, o in zip(NAMES, whole, one):
                assert torch.equal(w[i], o), (name, i)


def test_against_sparse_attention_on_the_csr_expansion():
    from torchsparsegradutils_amd import sparse_attention

    heads, d, dtype = 2, 64, torch.float32
    c = _case(heads, d, dtype, (16, 16), (2, 0, 3, 1))
    got = _check_case(c, dtype, torch.int32, "cross-check")
    mask = c["mask"]
    B = _to_dense(c["crow"], c["col"], c["blocks"], c["ncb"])[1]
    A = ar.sparse_from_dense(B, mask, "csr", torch.int32, dtype).to(DEV).requires_grad_(True)
    q, k, v = (x.to(dtype).to(DEV).requires_grad_(True) for x in (c["Q"], c["K"], c["V"]))
    O = sparse_attention(A, q, k, v, scale=c["scale"])
    dA, dq, dk, dv = torch.autograd.grad(O, (A, q, k, v), c["dO"].to(dtype).to(DEV))
    dense = torch.zeros(mask.shape, dtype=dtype)
    dense[mask] = dA.values().cpu()
    for name, a, b, bd in zip(NAMES, got, (O.detach().cpu(), dq.cpu(), dk.cpu(), dv.cpu(), dense), c["bounds"]):
        assert bool(((a.double() - b.double()).abs() <= 2 * bd).all()), name


def test_refusal_of_unsupported_geometry_on_the_gpu():
    from torchsparsegradutils_amd import sparse_bsr_attention

    def bsr(bh, bw):
        return torch.sparse_bsr_tensor(torch.tensor([0, 1]), torch.tensor([0]), torch.zeros(1, bh, bw), (bh, bw)).to(DEV)

    limits = "sparse_bsr_attention: the gfx950 kernels take block sides that are multiples of 16, d in {16, 32, 64, 128} and H >= 1, got "
    for bh, bw, d in ((8, 16, 32), (16, 24, 32), (16, 16, 8), (16, 16, 48), (16, 16, 256)):
        with pytest.raises(ValueError, match=re.escape(limits + f"blocks of {bh} x {bw}, d={d} and H=1")):
            sparse_bsr_attention(bsr(bh, bw), torch.zeros(bh, d, device=DEV), torch.zeros(bw, d, device=DEV), torch.zeros(bw, d, device=DEV))
