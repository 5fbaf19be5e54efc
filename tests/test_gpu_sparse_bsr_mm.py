"""sparse_bsr_mm on the GPU: the three kernels of include/tsgu_hip_bsr.h bit for bit on exact integer data at every size where their
walk changes path, position independence and run-to-run determinism, the rounding bounds through the public function, and the
pattern cache.  Operands are built on the CPU and every reference is numpy float64 on the CPU (tests/_bsr_ref.py); no torch BSR
conversion and no to_dense runs on the device."""

import warnings

import numpy as np
import pytest
import torch

import _bsr_ref as br
from torchsparsegradutils_amd import _backend as _be
from torchsparsegradutils_amd import _pattern, sparse_bsr_mm, sparse_mm

pytestmark = pytest.mark.gpu

warnings.filterwarnings("ignore", message="Sparse BSR tensor support is in beta state")

DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}


def _geometry():
    """(T, {dtype: S}, {dtype: W at a wide p}): the same tile height for every type (asserted), the stage per type."""
    geo = {dt: _be.bsr_mm_geometry(dt, 16, 16, 4096) for dt in DTYPES}
    assert len({g[0] for g in geo.values()}) == 1
    return geo[torch.float32][0], {dt: g[2] for dt, g in geo.items()}, {dt: g[1] for dt, g in geo.items()}


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _transposed_pattern(crow, col, ncb):
    """The pattern whose block (J, I) is stored for every block (I, J) of (crow, col): its block COLUMNS have the lengths of the
    given block rows."""
    rows = br.block_rows(crow)
    order = np.argsort(col, kind="stable")
    tcrow = np.concatenate(([0], np.cumsum(np.bincount(col, minlength=ncb)))).astype(np.int64)
    return tcrow, rows[order].astype(np.int64)


def _entries(crow, col, val, B, G, bh, bw, dtype, itype=torch.int64):
    """(C, dV, dB) of the three launchers for numpy operands, copied back to the CPU in `dtype`."""
    nrb, ncb = len(crow) - 1, B.shape[0] // bw
    crow_d, col_d = _dev(crow, itype), _dev(col, itype)
    val_d, B_d, G_d = _dev(val.reshape(-1, bh, bw), dtype), _dev(B, dtype), _dev(G, dtype)
    C = _be.bsr_spmm(crow_d, col_d, val_d, B_d, nrb, ncb)
    dV = _be.bsr_sddmm(crow_d, col_d, G_d, B_d, nrb, ncb, bh, bw)
    t = _pattern.RowGather(crow_d, col_d, nrb, ncb).transposed
    dB = _be.bsr_spmm_t(t.crow, t.col, t.perm, val_d, G_d, nrb, ncb)
    return C.cpu(), dV.cpu(), dB.cpu()


def _expect(x, dtype):
    """An exact integer result in `dtype`: itself, or rounded once for bfloat16."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype)


def _stage_lengths(stages, kb):
    """Block-row lengths around one and two LDS stages of every value type, for blocks of `kb` summed elements."""
    lens = {0, 1}
    for S in stages:
        q = -(-S // kb)
        lens |= {max(q - 1, 0), q, q + 1, 2 * q + 1}
    return sorted(lens)


def _structure_case(bh, bw, nrb, ncb, lens, p, seed, by_column):
    """Integer operands and their exact products.  `by_column`: the block COLUMNS get the lengths (the transposed product's walk)."""
    if by_column:
        tcrow, tcol = br.random_bsr(len(lens), nrb, lens, seed)            # rows of this pattern = block columns of A
        crow, col = _transposed_pattern(tcrow, tcol, nrb)
        ncb = len(lens)
    else:
        crow, col = br.random_bsr(nrb, ncb, lens, seed)
    val = br.small_ints((len(col), bh, bw), seed + 1)
    B = br.small_ints((ncb * bw, p), seed + 2, -2, 3)
    G = br.small_ints((nrb * bh, p), seed + 3)
    C, mag, _ = br.forward(crow, col, val, B, bh, bw)
    dV, _, dB, mag_b, _ = br.gradients(crow, col, val, B, G, bh, bw)
    assert max(mag.max(initial=0), mag_b.max(initial=0)) < 2 ** 24
    return crow, col, val, B, G, C, dV, dB


def _blocks():
    T, S, _ = _geometry()
    return [(16, 16), (32, 32), (16, 64), (64, 16), (8, 8), (3, 5), (1, 1), (T + 8, max(S.values()) + 8)]


@pytest.mark.parametrize("by_column", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("block", range(8), ids=["16x16", "32x32", "16x64", "64x16", "8x8", "3x5", "1x1", "beyond_tile"])
def test_structure_bit_for_bit(block, by_column):
    T, S, W = _geometry()
    bh, bw = _blocks()[block]
    oh, kb = (bw, bh) if by_column else (bh, bw)            # output rows / summed elements per block of the walked side
    lens_all = _stage_lengths(S.values(), kb)
    per_tile = max(T // oh, 1)
    counts = sorted({1, per_tile - 1, per_tile, per_tile + 1} - {0}) if oh <= T else [1, 2]
    ps = sorted({1, 3, 16, 17} | {w for w in W.values()} | {w + 1 for w in W.values()})
    other = 5
    empty_seen = False
    for ci, n_groups in enumerate(counts):
        # every length appears: the walked side is at least as long as the list, cycled through it from a moving start
        n_walk = max(n_groups, len(lens_all)) if ci == len(counts) - 1 else n_groups
        lens = [lens_all[(i + ci) % len(lens_all)] for i in range(n_walk)]
        for pi, p in enumerate(ps if ci == len(counts) - 1 else ps[ci::len(counts)] or ps[:1]):
            nrb, ncb = (other, n_walk) if by_column else (n_walk, other)
            crow, col, val, B, G, C, dV, dB = _structure_case(bh, bw, nrb, ncb, lens, p, 100 * block + 10 * ci + pi, by_column)
            empty_seen = empty_seen or 0 in lens
            for dtype in DTYPES:
                itype = torch.int32 if (pi + ci) % 2 else torch.int64
                got = _entries(crow, col, val, B, G, bh, bw, dtype, itype)
                for name, g, w in zip(("spmm", "sddmm", "spmm_t"), got, (C, dV.reshape(-1, bh, bw), dB)):
                    want = _expect(w, dtype)
                    assert g.shape == want.shape and torch.equal(g, want), (name, (bh, bw), n_walk, p, dtype, itype)
    assert empty_seen


def test_int64_and_int32_indices_agree():
    crow, col, val, B, G, C, dV, dB = _structure_case(16, 32, 5, 4, [3, 0, 9, 1, 4], 17, 7, False)
    for dtype in DTYPES:
        a = _entries(crow, col, val, B, G, 16, 32, dtype, torch.int32)
        b = _entries(crow, col, val, B, G, 16, 32, dtype, torch.int64)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(a[0], _expect(C, dtype)) and torch.equal(a[2], _expect(dB, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
def test_empty_rows_columns_and_matrices(dtype):
    bh, bw, p = 16, 32, 9
    # block rows 1 and 3 and block columns 0 and 2 hold nothing
    crow = np.array([0, 2, 2, 5, 5], dtype=np.int64)
    col = np.array([3, 1, 1, 4, 3], dtype=np.int64)
    val = br.small_ints((5, bh, bw), 1)
    B, G = br.small_ints((5 * bw, p), 2, -2, 3), br.small_ints((4 * bh, p), 3)
    C, dV, dB = _entries(crow, col, val, B, G, bh, bw, dtype)
    assert (C[bh:2 * bh] == 0).all() and (C[3 * bh:] == 0).all() and (C[:bh] != 0).any()
    assert (dB[:bw] == 0).all() and (dB[2 * bw:3 * bw] == 0).all() and (dB[bw:2 * bw] != 0).any()
    assert torch.equal(C, _expect(br.forward(crow, col, val, B, bh, bw)[0], dtype))
    # no blocks at all: zeros of the right shape, through the backend and through the public function
    none = np.zeros(0, dtype=np.int64)
    C, dV, dB = _entries(np.zeros(5, dtype=np.int64), none, np.zeros((0, bh, bw)), B, G, bh, bw, dtype)
    assert C.shape == (4 * bh, p) and (C == 0).all() and dV.shape == (0, bh, bw) and dB.shape == (5 * bw, p) and (dB == 0).all()
    A = torch.sparse_bsr_tensor(torch.zeros(5, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV),
                                torch.zeros(0, bh, bw, dtype=dtype, device=DEV), (4 * bh, 5 * bw)).requires_grad_(True)
    Bd = _dev(B, dtype).requires_grad_(True)
    out = sparse_bsr_mm(A, Bd)
    gA, gB = torch.autograd.grad(out, (A, Bd), torch.ones_like(out))
    assert out.shape == (4 * bh, p) and (out == 0).all() and gA.values().shape == (0, bh, bw) and (gB == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# position independence and determinism


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
def test_position_independence_and_determinism(dtype):
    """One block row's (block column's) content placed first, last and alone in a workgroup's tile: the same bits; and every
    launcher twice: the same bits."""
    T, S, _ = _geometry()
    bh = bw = 16
    per_tile, ncb, p = T // bh, 6, 33
    rng = np.random.default_rng(5)
    n_own = 2 * (-(-S[dtype] // bw)) + 1                                   # more than two stages
    own_col = rng.integers(0, ncb, n_own)
    own_val = rng.standard_normal((n_own, bh, bw))
    B = rng.standard_normal((ncb * bw, p))
    rows_out, cols_out, blocks_out = [], [], []
    for where in ("first", "last", "alone"):
        nrb = 1 if where == "alone" else per_tile
        at = nrb - 1 if where == "last" else 0
        lens = [n_own if i == at else 3 for i in range(nrb)]
        crow = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        col = rng.integers(0, ncb, crow[-1])
        val = rng.standard_normal((crow[-1], bh, bw))
        col[crow[at]:crow[at + 1]] = own_col
        val[crow[at]:crow[at + 1]] = own_val
        G = rng.standard_normal((nrb * bh, p))
        G[at * bh:(at + 1) * bh] = 0.5
        first = _entries(crow, col, val, B, G, bh, bw, dtype)
        again = _entries(crow, col, val, B, G, bh, bw, dtype)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        rows_out.append(first[0][at * bh:(at + 1) * bh])
        blocks_out.append(first[1][crow[at]:crow[at + 1]])
        # the same content as a block COLUMN: the transposed pattern, whose spmm_t output rows [at·bh, +bh) it owns
        tcrow, tcol = _transposed_pattern(crow, col, ncb)                 # (ncb x nrb blocks; its columns are the rows above)
        tval = np.ascontiguousarray(val[np.argsort(col, kind="stable")].transpose(0, 2, 1))
        cols_out.append(_entries(tcrow, tcol, tval, np.zeros((nrb * bh, p)), B, bw, bh, dtype)[2][at * bh:(at + 1) * bh])
    for outs in (rows_out, cols_out, blocks_out):
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert rows_out[0].abs().max() > 0 and cols_out[0].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# rounding, through the public function


def _bound(want, mag, dtype, chain):
    """The bounds of tests/test_gpu_indexed_mm.py::_check."""
    want, mag, chain = torch.as_tensor(want), torch.as_tensor(mag), torch.as_tensor(chain, dtype=torch.float64)
    if dtype == torch.bfloat16:
        # fp32 accumulation, one rounding: within one bf16 ulp of the exact value (plus the fp32 chain)
        ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (torch.floor(torch.log2(want.abs())) - 7))
        return ulp + chain * EPS[torch.float32] * mag * 2
    return chain * EPS[dtype] * mag + 1e-300


def _check(got, want, mag, dtype, chain):
    got, want = got.double().cpu(), torch.as_tensor(want)
    err = (got - want).abs()
    bound = _bound(want, mag, dtype, chain)
    assert got.shape == want.shape and bool((err <= bound).all()), float((err - bound).max())


def _random_case(bh, bw, lens, ncb, p, seed, dtype):
    crow, col = br.random_bsr(len(lens), ncb, lens, seed, duplicates=True)
    rng = np.random.default_rng(seed + 1)
    as_type = lambda x: torch.from_numpy(x).to(dtype)                       # noqa: E731  (the values the device sees)
    val, B, G = as_type(rng.standard_normal((len(col), bh, bw))), as_type(rng.standard_normal((ncb * bw, p))), as_type(
        rng.standard_normal((len(lens) * bh, p)))
    return crow, col, val, B, G


def _oracle(crow, col, val, B, G, bh, bw):
    C, mag, terms = br.forward(crow, col, val.double().numpy(), B.double().numpy(), bh, bw)
    dV, mag_v, dB, mag_b, terms_b = br.gradients(crow, col, val.double().numpy(), B.double().numpy(), G.double().numpy(), bh, bw)
    return (C, mag, terms[:, None]), (dV, mag_v, B.shape[1]), (dB, mag_b, terms_b[:, None])


LENS_R = [4, 0, 7, 1, 2, 9, 3]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("p", [8, 33])
@pytest.mark.parametrize("block", [(16, 16), (32, 64), (5, 3)], ids=["16x16", "32x64", "5x3"])
def test_rounding_2d(block, p, dtype):
    bh, bw = block
    ncb = 5
    crow, col, val, B, G = _random_case(bh, bw, LENS_R, ncb, p, 3, dtype)
    assert (np.diff(col) < 0).any() and len(col) != len({(i, j) for i, j in zip(br.block_rows(crow), col)})
    A = torch.sparse_bsr_tensor(_dev(crow, torch.int64), _dev(col, torch.int64), val.to(DEV), (len(LENS_R) * bh, ncb * bw)).requires_grad_(True)
    Bd = B.to(DEV).requires_grad_(True)
    C = sparse_bsr_mm(A, Bd)
    gA, gB = torch.autograd.grad(C, (A, Bd), G.to(DEV))
    oc, ov, ob = _oracle(crow, col, val, B, G, bh, bw)
    _check(C.detach(), *oc[:2], dtype, oc[2])
    assert gA.layout == torch.sparse_bsr and gA.crow_indices().data_ptr() == A.crow_indices().data_ptr()
    _check(gA.values(), *ov[:2], dtype, ov[2])
    _check(gB, *ob[:2], dtype, ob[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("block,p", [((16, 16), 33), ((32, 64), 8), ((5, 3), 33)], ids=["16x16", "32x64", "5x3"])
def test_rounding_batched(block, p, dtype):
    bh, bw = block
    ncb, b = 5, 3
    lens = ([4, 0, 7, 1], [0, 6, 3, 3], [2, 2, 4, 4])                       # equal nnzb per item, as torch's batched BSR requires
    items = [_random_case(bh, bw, L, ncb, p, 20 + i, dtype) for i, L in enumerate(lens)]
    stack = lambda k, dt=None: torch.stack([torch.as_tensor(it[k]) for it in items]).to(DEV)      # noqa: E731
    A = torch.sparse_bsr_tensor(stack(0).to(torch.int32), stack(1).to(torch.int32), stack(2), (b, 4 * bh, ncb * bw)).requires_grad_(True)
    Bd = stack(3).requires_grad_(True)
    C = sparse_bsr_mm(A, Bd)
    gA, gB = torch.autograd.grad(C, (A, Bd), stack(4))
    assert C.shape == (b, 4 * bh, p) and gA.values().shape == (b, 12, bh, bw) and gA.col_indices().dtype == torch.int32
    for i, it in enumerate(items):
        oc, ov, ob = _oracle(*it, bh, bw)
        _check(C[i].detach(), *oc[:2], dtype, oc[2])
        _check(gA.values()[i], *ov[:2], dtype, ov[2])
        _check(gB[i], *ob[:2], dtype, ob[2])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64", "bf16"])
def test_unit_blocks_agree_with_sparse_mm(dtype):
    n, m, p = 70, 40, 33
    lens = [(7 * i) % 23 for i in range(n)]
    crow, col = br.random_bsr(n, m, lens, 4, canonical=True)
    rng = np.random.default_rng(9)
    val, B = torch.from_numpy(rng.standard_normal(len(col))).to(dtype), torch.from_numpy(rng.standard_normal((m, p))).to(dtype)
    crow_d, col_d = _dev(crow, torch.int64), _dev(col, torch.int64)
    bsr = sparse_bsr_mm(torch.sparse_bsr_tensor(crow_d, col_d, val.to(DEV).reshape(-1, 1, 1), (n, m)), B.to(DEV))
    csr = sparse_mm(torch.sparse_csr_tensor(crow_d, col_d, val.to(DEV), (n, m)), B.to(DEV))
    C, mag, terms = br.forward(crow, col, val.double().numpy().reshape(-1, 1, 1), B.double().numpy(), 1, 1)
    _check(bsr, C, mag, dtype, terms[:, None])
    # with sparse_mm on the CSR form: within the sum of both bounds
    err = (bsr.double().cpu() - csr.double().cpu()).abs()
    assert bool((err <= 2 * _bound(C, mag, dtype, terms[:, None])).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_strided_b_and_one_sided_gradients(dtype):
    bh, bw, ncb, p = 16, 16, 5, 33
    crow, col, val, B, G = _random_case(bh, bw, LENS_R, ncb, p, 8, dtype)
    crow_d, col_d, val_d = _dev(crow, torch.int64), _dev(col, torch.int64), val.to(DEV)
    shape = (len(LENS_R) * bh, ncb * bw)
    A = torch.sparse_bsr_tensor(crow_d, col_d, val_d, shape)
    Bd, Gd = B.to(DEV), G.to(DEV)
    want = sparse_bsr_mm(A, Bd)
    assert not want.requires_grad
    wide = torch.zeros(ncb * bw, 2 * p + 1, dtype=dtype, device=DEV)
    wide[:, 1::2] = Bd
    wide[:, 0::2] = 7.0
    assert torch.equal(sparse_bsr_mm(A, wide[:, 1::2]), want)               # column stride 2: copied
    padded = torch.full((ncb * bw, p + 3), 7.0, dtype=dtype, device=DEV)
    padded[:, 1:p + 1] = Bd
    view = padded[:, 1:p + 1]
    assert not view.is_contiguous() and torch.equal(sparse_bsr_mm(A, view), want)     # row stride p + 3, unaligned start: in place
    assert torch.equal(sparse_bsr_mm(A, Bd.t().contiguous().t()), want)
    Ag, Bg = A.detach().clone().requires_grad_(True), Bd.clone().requires_grad_(True)
    gA, gB = torch.autograd.grad(sparse_bsr_mm(Ag, Bg), (Ag, Bg), Gd)
    (only_a,) = torch.autograd.grad(sparse_bsr_mm(Ag, Bd), (Ag,), Gd)
    (only_b,) = torch.autograd.grad(sparse_bsr_mm(A, Bg), (Bg,), Gd)
    assert torch.equal(only_a.values(), gA.values()) and torch.equal(only_b, gB)
    # a gradient that is a strided view
    gwide = torch.zeros(shape[0], 2 * p, dtype=dtype, device=DEV)
    gwide[:, ::2] = Gd
    (gB2,) = torch.autograd.grad(sparse_bsr_mm(A, Bg), (Bg,), gwide[:, ::2])
    assert torch.equal(gB2, gB)


# ---------------------------------------------------------------------------------------------------------------------------
# pattern cache


def test_the_pattern_cache_hits_on_the_index_tensors():
    bh, bw, ncb, p = 16, 16, 5, 8
    lens = [4, 0, 5, 1, 2, 3, 3]                                             # (torch's canonical form: what its own backward assumes)
    crow, col = br.random_bsr(len(lens), ncb, lens, 3, canonical=True)
    crow_d, col_d = _dev(crow, torch.int64), _dev(col, torch.int64)
    shape = (len(lens) * bh, ncb * bw)
    B = torch.randn(ncb * bw, p, device=DEV)
    A = torch.sparse_bsr_tensor(crow_d, col_d, torch.randn(len(col), bh, bw, device=DEV), shape).requires_grad_(True)
    torch.autograd.grad(sparse_bsr_mm(A, B).sum(), (A,))
    assert _pattern.cache_stats()[0] == 1
    core = next(iter(_pattern._CACHE.values()))
    torch.autograd.grad(sparse_bsr_mm(A, B).sum(), (A,))
    assert _pattern.cache_stats()[0] == 1 and next(iter(_pattern._CACHE.values())) is core
    # a values parameter rebuilt into a fresh BSR tensor each step
    values = torch.nn.Parameter(torch.randn(len(col), bh, bw, device=DEV))
    Bp = B.clone().requires_grad_(True)
    for _ in range(3):
        values.grad = None
        (sparse_bsr_mm(torch.sparse_bsr_tensor(crow_d, col_d, values, shape), Bp) ** 2).sum().backward()
        assert values.grad is not None and Bp.grad is not None
        assert _pattern.cache_stats()[0] == 1 and next(iter(_pattern._CACHE.values())) is core
    assert core.t is not None                                                # the transposed walk was built once, and kept
