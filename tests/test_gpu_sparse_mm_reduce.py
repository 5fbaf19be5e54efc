"""sparse_mm_reduce on the GPU against the numpy oracle of tests/_mm_reduce_ref.py (pinned to torch.sparse.mm(A, B, reduce) on the
CPU by tests/test_sparse_mm_reduce_cpu.py).

Forward and arg, at backend level: bit for bit, for float32, float64 and bfloat16.  Derived, not measured: a candidate is ONE IEEE
multiplication in the accumulator type (the build has -ffp-contract=off) and the rest is selection; bfloat16 is the float32
result rounded once.  The structural matrix is built from the geometry query — rows per workgroup R, staging capacity S, columns
per slice W — and its operands are bfloat16-exact, so one float64 run of the oracle serves the three value types (the product of
two bfloat16 numbers is exact in float32, and comparisons of exact numbers do not depend on the type).  Operands that do round
in the multiplication are in the gradient cases, whose forward is compared bit for bit as well.

Gradients, through the public function, against the oracle in float64 (u = 2^-24 for float32 / bfloat16, 2^-53 for float64):
  gradA   |gradA[e] - ref| <= (p + 2) u sum |G·B| over e's winning columns        (p terms, some of them zeros, summed in fp;
  gradB   |gradB[j,k] - ref| <= (L_j + 2) u sum |val·G| over the winners in column j    one rounding per product, one to store)
  bfloat16: one rounding to bfloat16 (2^-8 relative) of the float32 result on top.
Entries and elements without a winner are exactly 0; two runs are bit-identical.
"""

import functools

import numpy as np
import pytest
import torch

import _mm_reduce_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("float32", "float64", "bfloat16")
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53, "bfloat16": 2.0 ** -24}
U_BF16 = 2.0 ** -8          # unit roundoff of the bfloat16 storage format (tests/test_gpu_sparse_softmax.py)
S = 2048                    # staging capacity (asserted against the geometry query below)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _geometry(dtype, p):
    from torchsparsegradutils_amd import _backend

    return _backend.spmm_reduce_geometry(mr.TORCH_DTYPE[dtype], p)


def _bf16_exact(x):
    return torch.from_numpy(np.asarray(x)).to(torch.bfloat16).to(torch.float64).numpy()


def _dev(x, dtype, index=False):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(DEV) if index else t.to(mr.TORCH_DTYPE[dtype]).to(DEV)


def _backend_forward(crow, col, val, B, dtype, reduce, index_dtype=np.int32):
    from torchsparsegradutils_amd import _backend

    n, m = len(crow) - 1, B.shape[0]
    C, arg = _backend.csr_spmm_reduce(_dev(crow.astype(index_dtype), dtype, True), _dev(col.astype(index_dtype), dtype, True),
                                      _dev(val, dtype), _dev(B, dtype), n, m, reduce)
    torch.cuda.synchronize()
    return C.cpu(), arg.cpu()


def _expect(C64, dtype):
    """The oracle's exact float64 result as the value type stores it (one rounding for bfloat16, none otherwise)."""
    return torch.from_numpy(C64).to(mr.TORCH_DTYPE[dtype])


# ---------------------------------------------------------------------------------------------------------------------------
# structure: row lengths around the staging capacity, empty rows, a workgroup that overflows the stage with short rows

M_WIDE = 2 * S + 8


def _structural_lens():
    # 32 rows is the most a workgroup owns (p <= 32 columns) and 4 the fewest: a run of 32 rows of S/4 + 8 entries starting at
    # a multiple of 32 overflows the stage of every geometry (4 rows: 2080 > S) while no row does alone
    head = [0, 1, S - 1, S, S + 1, 0, 2 * S + 1, 1, 1]
    head += [2] * (32 - len(head))
    return head + [S // 4 + 8] * 32 + [1, 3, 0, 1, 0]


@functools.lru_cache(maxsize=None)
def _structural(p, reduce):
    lens = _structural_lens()
    crow, col = mr.random_csr(len(lens), M_WIDE, lens, seed=1)
    rng = np.random.default_rng(2)
    val, B = _bf16_exact(rng.standard_normal(len(col))), _bf16_exact(rng.standard_normal((M_WIDE, p)))
    C, arg = mr.forward(crow, col, val, B, reduce)
    return crow, col, val, B, C, arg


def _widths(dtype):
    W = _geometry(dtype, 4096)[2]
    return sorted({1, 3, 32, 33, W, W + 1, 130})


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_and_arg_bit_for_bit_on_the_structural_matrix(dtype):
    lens = _structural_lens()
    for p in _widths(dtype):
        R, stage, W = _geometry(dtype, p)
        assert stage == S and R in (4, 8, 16, 32) and 32 % R == 0 and lens[32:64] == [S // 4 + 8] * 32 and R * (S // 4 + 8) > S
        for reduce in (("amax", "amin") if p in (3, 32, 130) else ("amax",)):
            crow, col, val, B, C64, arg64 = _structural(p, reduce)
            C, arg = _backend_forward(crow, col, val, B, dtype, reduce, np.int64 if p == 33 else np.int32)
            assert mr.same_bits(C, _expect(C64, dtype)), (p, reduce)
            assert torch.equal(arg, torch.from_numpy(arg64)), (p, reduce)
            empty = np.nonzero(np.diff(crow) == 0)[0]
            assert len(empty) == 4 and (arg[empty] == -1).all() and (C[empty] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_counts_around_a_workgroup(dtype):
    for p in (1, 32, 33, 130):
        R = _geometry(dtype, p)[0]
        for n in sorted({1, R - 1, R, R + 1}):
            lens = list(np.random.default_rng(n).integers(0, 6, size=n))
            crow, col = mr.random_csr(n, 40, lens, seed=n)
            rng = np.random.default_rng(3)
            val, B = _bf16_exact(rng.standard_normal(len(col))), _bf16_exact(rng.standard_normal((40, p)))
            for reduce in ("amax", "amin"):
                C64, arg64 = mr.forward(crow, col, val, B, reduce)
                C, arg = _backend_forward(crow, col, val, B, dtype, reduce)
                assert mr.same_bits(C, _expect(C64, dtype)) and torch.equal(arg, torch.from_numpy(arg64)), (p, n, reduce)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_matrix_without_entries(dtype):
    crow, col = np.zeros(38, dtype=np.int64), np.zeros(0, dtype=np.int64)
    for p in (3, 32):
        C, arg = _backend_forward(crow, col, np.zeros(0), np.ones((5, p)), dtype, "amax")
        assert C.shape == (37, p) and (C == 0).all() and (arg == -1).all()


@functools.lru_cache(maxsize=None)
def _special(p, reduce):
    """Row 0: 2S + 2 entries whose first and last candidates tie for the maximum, and second and last but one for the minimum —
    the pairs fall into different entry lanes and different staging passes.  Row 1: all candidates negative (positive for amin).
    Row 2: a NaN value.  Row 3 gathers a NaN of B.  Row 4: +0.0 against -0.0 on rows of B of its own, column 1 with the opposite
    signs.  Row 5: empty.  Row 6: every candidate is the reduction's identity (-inf for amax, +inf for amin): the first is the
    winner.  Row 7: two such candidates, then numbers."""
    L = 2 * S + 2
    lens = [L, 10, 9, 9, 8, 0, 5, 6]
    crow, col = mr.random_csr(len(lens), M_WIDE, lens, seed=5)
    rng = np.random.default_rng(6)
    B = _bf16_exact(rng.uniform(0.5, 1.5, size=(M_WIDE + 9, p)))
    val = _bf16_exact(rng.uniform(-1.0, 1.0, size=len(col)))
    nan_row = M_WIDE                                    # a row of B only row 3 gathers (its last entry)
    col[crow[4] - 1] = nan_row
    B[nan_row, p // 2] = np.nan
    col[crow[4]:crow[5]] = M_WIDE + 1 + np.arange(8)
    if p > 1:
        B[M_WIDE + 1:, 1] *= -1.0
    for a, b, v in ((0, L - 1, 64.0), (1, L - 2, -64.0)):
        val[[a, b]] = v
        B[col[b]] = B[col[a]]
    r1 = slice(crow[1], crow[2])
    val[r1] = _bf16_exact(-np.abs(val[r1]) - 0.25 if reduce == "amax" else np.abs(val[r1]) + 0.25)
    val[crow[2] + 4] = np.nan
    val[crow[4]:crow[5]] = [0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 0.0]
    val[crow[6]:crow[7] + 2] = -np.inf if reduce == "amax" else np.inf
    C, arg = mr.forward(crow, col, val, B, reduce)
    return crow, col, val, B, C, arg


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_signed_zeros_and_nans(dtype, reduce):
    for p in (1, 3, 32):
        crow, col, val, B, C64, arg64 = _special(p, reduce)
        L = 2 * S + 2
        want = 0 if reduce == "amax" else 1
        assert (arg64[0] == want).all() and abs(C64[0]).min() >= 32.0              # the first of the tying pair, not the last
        assert np.isnan(C64[2]).all() and (arg64[2] == crow[2] + 4).all()
        assert np.isnan(C64[3, p // 2]) and arg64[3, p // 2] == crow[4] - 1 and np.isnan(C64[3]).sum() == 1
        assert (arg64[4] == crow[4]).all() and (C64[4] == 0).all()                  # equal zeros: the first stays, with its sign
        assert not np.signbit(C64[4, 0]) and (p == 1 or np.signbit(C64[4, 1]))
        assert ((C64[1] < 0) if reduce == "amax" else (C64[1] > 0)).all()          # absent entries are not zeros
        assert np.isinf(C64[6]).all() and (arg64[6] == crow[6]).all() and np.isfinite(C64[7]).all() and (arg64[7] >= crow[7] + 2).all()
        C, arg = _backend_forward(crow, col, val, B, dtype, reduce)
        assert mr.same_bits(C, _expect(C64, dtype)), p
        assert torch.equal(arg, torch.from_numpy(arg64)), p
        assert L % 8 == 2 and (L - 1) % 8 != 0 and (L - 1) // S == 2


# ---------------------------------------------------------------------------------------------------------------------------
# gradients through the public function


def _grad_case(dtype, p, ints):
    n, m = 70, 50
    rng = np.random.default_rng(11 + p)
    lens = list(rng.integers(0, 21, size=n))
    lens[0], lens[n // 2], lens[-1] = 0, 0, 0
    crow, col = mr.random_csr(n, m, lens, seed=12)
    draw = (lambda shape, s: mr.small_ints(shape, s)) if ints else (lambda shape, s: np.random.default_rng(s).standard_normal(shape))
    t = mr.TORCH_DTYPE[dtype]
    val, B, G = (torch.from_numpy(draw(shape, s)).to(t) for shape, s in ((len(col), 13), ((m, p), 14), ((n, p), 15)))
    return crow, col, val, B, G


def _public(A, B, G, reduce, need_a=True, need_b=True):
    from torchsparsegradutils_amd import sparse_mm_reduce

    A = A.detach().clone().requires_grad_(need_a)
    Bg = B.detach().clone().requires_grad_(need_b)
    C = sparse_mm_reduce(A, Bg, reduce)
    wanted = [t for t, need in ((A, need_a), (Bg, need_b)) if need]
    grads = list(torch.autograd.grad(C, wanted, G))
    torch.cuda.synchronize()
    gA = grads.pop(0) if need_a else None
    gB = grads.pop(0) if need_b else None
    return C.detach(), gA, gB


def _values_of(g):
    return g.values() if g.layout == torch.sparse_csr else g._values()


@pytest.mark.parametrize("ints", [False, True], ids=["normal", "ties"])
@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gradients_against_the_oracle(dtype, reduce, ints):
    u = U[dtype]
    for p in (1, 3, 32, 130, 264):
        crow, col, val, B, G = _grad_case(dtype, p, ints)
        n, m = len(crow) - 1, B.shape[0]
        C_o, arg = mr.forward(crow, col, mr.to_acc(val), mr.to_acc(B), reduce)
        dval, abs_a, dB, abs_b = mr.gradients(crow, col, mr.to_acc(val), mr.to_acc(B), mr.to_acc(G), arg)
        A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(torch.int32), torch.from_numpy(col).to(torch.int32), val, (n, m)).to(DEV)
        C, gA, gB = _public(A, B.to(DEV), G.to(DEV), reduce)
        assert mr.same_bits(C.cpu(), torch.from_numpy(C_o).to(mr.TORCH_DTYPE[dtype])), p           # (operands that round in the product)
        assert gA.layout == torch.sparse_csr and gA.col_indices().dtype == torch.int32
        assert torch.equal(gA.crow_indices(), A.crow_indices()) and torch.equal(gA.col_indices(), A.col_indices())
        ga, gb = gA.values().cpu().double().numpy(), gB.cpu().double().numpy()
        bound_a = (p + 2) * u * abs_a
        L = np.bincount(col, minlength=m).astype(np.float64)[:, None]
        bound_b = (L + 2) * u * abs_b
        if dtype == "bfloat16":
            bound_a = bound_a + U_BF16 * (np.abs(dval) + bound_a)
            bound_b = bound_b + U_BF16 * (np.abs(dB) + bound_b)
        ea, eb = np.abs(ga - dval), np.abs(gb - dB)
        print(f"{dtype} {reduce} p={p} ints={ints}: gradA err/bound {np.max(ea / np.maximum(bound_a, 1e-300)):.3f}, "
              f"gradB err/bound {np.max(eb / np.maximum(bound_b, 1e-300)):.3f}")
        assert (ea <= bound_a).all() and (eb <= bound_b).all(), p
        # without a winner: exactly 0
        won_a = np.zeros(len(col), dtype=bool)
        won_a[arg[arg >= 0]] = True
        assert ((~won_a).any() and (abs_b == 0).any()) or p > 32
        assert (ga[~won_a] == 0).all() and (gb[abs_b == 0] == 0).all()
        # two runs are bit-identical; one operand alone gives the same gradient
        C2, gA2, gB2 = _public(A, B.to(DEV), G.to(DEV), reduce)
        assert mr.same_bits(C2, C) and mr.same_bits(gA2.values(), gA.values()) and mr.same_bits(gB2, gB)
        if p in (3, 130):
            _, gA3, none = _public(A, B.to(DEV), G.to(DEV), reduce, need_b=False)
            _, none2, gB3 = _public(A, B.to(DEV), G.to(DEV), reduce, need_a=False)
            assert none is None and none2 is None and mr.same_bits(gA3.values(), gA.values()) and mr.same_bits(gB3, gB)


# ---------------------------------------------------------------------------------------------------------------------------
# layouts: the same bits as the CSR run


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts_give_the_csr_result(dtype, reduce):
    p = 32 if dtype != "float64" else 6
    crow, col, val, B, G = _grad_case(dtype, p, ints=False)
    n, m = len(crow) - 1, B.shape[0]
    B, G = B.to(DEV), G.to(DEV)
    crow_t, col_t = torch.from_numpy(crow), torch.from_numpy(col)
    A32 = torch.sparse_csr_tensor(crow_t.to(torch.int32), col_t.to(torch.int32), val, (n, m)).to(DEV)
    C, gA, gB = _public(A32, B, G, reduce)
    # int64 indices
    A64 = torch.sparse_csr_tensor(crow_t, col_t, val, (n, m)).to(DEV)
    C2, gA2, gB2 = _public(A64, B, G, reduce)
    assert gA2.col_indices().dtype == torch.int64
    assert mr.same_bits(C2, C) and mr.same_bits(gA2.values(), gA.values()) and mr.same_bits(gB2, gB)
    # coalesced COO
    rows = torch.repeat_interleave(torch.arange(n), crow_t[1:] - crow_t[:-1])
    idx = torch.stack((rows, col_t))
    Acoo = torch.sparse_coo_tensor(idx, val, (n, m)).coalesce().to(DEV)
    C3, gA3, gB3 = _public(Acoo, B, G, reduce)
    assert gA3.layout == torch.sparse_coo and torch.equal(gA3._indices(), Acoo._indices())
    assert mr.same_bits(C3, C) and mr.same_bits(gA3._values(), gA.values()) and mr.same_bits(gB3, gB)
    # un-coalesced COO: every entry as two exact halves, shuffled — one matrix entry, whose gradient coalesce's backward hands on
    perm = torch.randperm(2 * val.numel())
    Au = torch.sparse_coo_tensor(torch.cat((idx, idx), 1)[:, perm], torch.cat((val * 0.5, val * 0.5))[perm], (n, m)).to(DEV)
    assert not Au.is_coalesced()
    C4, gA4, gB4 = _public(Au, B, G, reduce)
    assert mr.same_bits(C4, C) and mr.same_bits(gB4, gB)
    gA4 = gA4.coalesce()
    assert torch.equal(gA4._indices(), Acoo._indices()) and mr.same_bits(gA4._values(), gA.values())
    # a transposed view of B
    Bt = B.t().contiguous().t()
    assert not Bt.is_contiguous()
    C5, gA5, gB5 = _public(A32, Bt, G, reduce)
    assert mr.same_bits(C5, C) and mr.same_bits(gA5.values(), gA.values()) and mr.same_bits(gB5, gB)


@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_operands_give_the_items_results(dtype):
    t, p, n, m = mr.TORCH_DTYPE[dtype], 32, 9, 12
    lens = ([3, 0, 2, 4, 1, 0, 7, 2, 1], [0, 0, 5, 1, 1, 12, 0, 0, 1], [2, 2, 2, 2, 2, 2, 2, 2, 4])
    assert sum(lens[0]) == sum(lens[1]) == sum(lens[2]) == 20
    items = []
    for b, L in enumerate(lens):
        crow, col = mr.random_csr(n, m, L, seed=30 + b)
        val = torch.from_numpy(np.random.default_rng(40 + b).standard_normal(len(col))).to(t)
        items.append((torch.from_numpy(crow).to(torch.int32), torch.from_numpy(col).to(torch.int32), val))
    B = torch.from_numpy(np.random.default_rng(50).standard_normal((3, m, p))).to(t).to(DEV)
    G = torch.from_numpy(np.random.default_rng(51).standard_normal((3, n, p))).to(t).to(DEV)
    alone = [_public(torch.sparse_csr_tensor(c, j, v, (n, m)).to(DEV), B[b], G[b], "amax") for b, (c, j, v) in enumerate(items)]
    # batched CSR
    Acsr = torch.sparse_csr_tensor(torch.stack([c for c, _, _ in items]), torch.stack([j for _, j, _ in items]),
                                   torch.stack([v for _, _, v in items]), (3, n, m)).to(DEV)
    C, gA, gB = _public(Acsr, B, G, "amax")
    assert C.shape == (3, n, p) and gA.layout == torch.sparse_csr and gA.col_indices().dtype == torch.int32
    for b in range(3):
        assert mr.same_bits(C[b], alone[b][0]) and mr.same_bits(gB[b], alone[b][2]) and mr.same_bits(gA.values()[b], alone[b][1].values())
    # batched COO, items of unequal nnz: the third item loses its last row
    keep = [20, 20, 16]
    coo = [torch.sparse_coo_tensor(torch.stack((torch.repeat_interleave(torch.arange(n), (c[1:] - c[:-1]).long())[:k], j[:k].long())),
                                   v[:k], (n, m)) for (c, j, v), k in zip(items, keep)]
    Acoo = torch.stack(coo).coalesce().to(DEV)
    C, gA, gB = _public(Acoo, B, G, "amax")
    c, j, v = items[2]
    c = c.clone()
    c[-1] = 16
    last = _public(torch.sparse_csr_tensor(c, j[:16], v[:16], (n, m)).to(DEV), B[2], G[2], "amax")
    want = [alone[0], alone[1], last]
    assert gA.layout == torch.sparse_coo and torch.equal(gA._indices(), Acoo._indices())
    for b in range(3):
        assert mr.same_bits(C[b], want[b][0]) and mr.same_bits(gB[b], want[b][2])
    assert mr.same_bits(gA._values(), torch.cat([w[1].values() for w in want]))


# ---------------------------------------------------------------------------------------------------------------------------
# mean: sparse_mm and one row scaling


@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_is_sparse_mm_divided_by_the_stored_count(dtype):
    from torchsparsegradutils_amd import sparse_mm

    crow, col, val, B, G = _grad_case(dtype, 32, ints=False)
    n, m = len(crow) - 1, B.shape[0]
    B, G = B.to(DEV), G.to(DEV)
    A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(torch.int32), torch.from_numpy(col).to(torch.int32), val, (n, m)).to(DEV)
    lens = np.diff(crow)
    count = torch.from_numpy(np.maximum(lens, 1)).to(mr.TORCH_DTYPE[dtype]).to(DEV)[:, None]        # (<= 20: exact in bfloat16)
    C, gA, gB = _public(A, B, G, "mean")
    Am, Bm = A.detach().clone().requires_grad_(True), B.clone().requires_grad_(True)
    Cm = sparse_mm(Am, Bm)
    gAm, gBm = torch.autograd.grad(Cm, (Am, Bm), G / count)
    assert mr.same_bits(C, Cm.detach() / count)
    assert mr.same_bits(gA.values(), gAm.values()) and mr.same_bits(gB, gBm)
    assert (lens == 0).sum() >= 3 and (C[torch.from_numpy(lens == 0).to(DEV)] == 0).all()
    assert gA.col_indices().dtype == torch.int32
