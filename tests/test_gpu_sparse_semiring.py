"""sparse_semiring_mm on the GPU against the float64 numpy oracle of tests/_semiring_ref.py (pinned to a dense restatement by
tests/test_sparse_semiring_cpu.py).  u = 2^-24 for float32 / bfloat16, 2^-53 for float64.

Tropical forward: C and arg bit for bit (one IEEE addition and a selection).  log forward, per element, L the row's length and w the
float64 weights:  |C - ref| <= (3L + 32 + 8 ln(1 + L)) u + u (Σ w|t| + 2|ref|)  (+ 2^-8 |ref| for a bfloat16 C) — the rounded
addition, L steps of at most three roundings plus the merges, the rounded arguments of the exp calls, the log and the final add.
Structural operands lie on a grid of 1/32 below 4: exact in bfloat16, sums exact in float32, one oracle run serves the three types.

Gradients (public function): log, with rho the forward bound plus u (2|t| + |C|) (the kernels read their own stored C):
  |dval[e] - ref| <= Σ_c |G| W (rho + (p + 4) u)        |dB[j,c] - ref| <= Σ_e |G| W (rho + (L_j + 4) u)
tropical: (p + 2) u Σ|G| and (L_j + 2) u Σ|G| over the winners, exactly 0 without one; bfloat16: one rounding (2^-8) on top.
"""

import functools

import numpy as np
import pytest
import torch

import _semiring_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("float32", "float64", "bfloat16")
U = {"float32": 2.0 ** -24, "float64": 2.0 ** -53, "bfloat16": 2.0 ** -24}
U_BF16 = 2.0 ** -8
S = 2048                    # staging capacity (asserted against the geometry query below)
M_WIDE = 2 * S + 8
both = lambda f: pytest.mark.parametrize("dtype", DTYPES)(pytest.mark.parametrize("semiring", sr.SEMIRINGS)(f))  # noqa: E731


def _be():
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    return _backend


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(sr.TORCH_DTYPE[dtype])).to(DEV)


def _grid(x):
    return np.clip(np.round(np.asarray(x) * 32), -127, 127) / 32


def _as64(x, dtype):
    """Operands as the value type holds them, converted exactly to float64."""
    return torch.from_numpy(np.asarray(x)).to(sr.TORCH_DTYPE[dtype]).to(torch.float64).numpy()


def _check_forward(case, dtype, semiring, index_dtype=np.int32, tag=None):
    crow, col, val, B, (C64, arg64, wt) = case
    C, C_acc, arg = _be().csr_semiring_mm(_t(crow.astype(index_dtype)), _t(col.astype(index_dtype)), _t(val, dtype), _t(B, dtype),
                                          len(crow) - 1, B.shape[0], semiring, want_acc=True)
    if semiring != "log":
        assert C_acc is None and sr.same_bits(C, torch.from_numpy(C64).to(C.dtype)) and torch.equal(arg.cpu(), torch.from_numpy(arg64)), tag
        return
    assert arg is None and C_acc.dtype == (torch.float64 if dtype == "float64" else torch.float32)
    assert sr.same_bits(C, C_acc.to(C.dtype)), "a bfloat16 C is the float32 one rounded once"
    fin = np.isfinite(C64)
    bound = sr.forward_bound(crow, C64, wt, U[dtype])
    for got, extra in ((C_acc, 0.0), (C, U_BF16 if dtype == "bfloat16" else 0.0)):
        got = got.double().cpu().numpy()
        with np.errstate(invalid="ignore"):
            excess = np.abs(got - C64)[fin] - (bound + extra * np.abs(C64))[fin]
        assert np.array_equal(got[~fin], C64[~fin], equal_nan=True), tag
        assert excess.size == 0 or excess.max() <= 0, (tag, float(excess.max()))


@functools.lru_cache(maxsize=None)
def _structural(p, semiring):
    # a run of 32 rows of S/4 + 8 entries starting at a multiple of 32 overflows the stage of every geometry (4 rows: 2080 > S)
    lens = [0, 1, S - 1, S, S + 1, 0, 2 * S + 1, 1, 1] + [2] * 23 + [S // 4 + 8] * 32 + [1, 3, 0, 1, 0]
    crow, col = sr.random_csr(len(lens), M_WIDE, lens, seed=1)
    rng = np.random.default_rng(2)
    val, B = _grid(rng.standard_normal(len(col))), _grid(rng.standard_normal((M_WIDE, p)))
    return crow, col, val, B, sr.forward(crow, col, val, B, semiring)


@both
def test_forward_on_the_structural_matrix(dtype, semiring):
    W = _be().semiring_geometry(sr.TORCH_DTYPE[dtype], 4096)[2]
    for p in sorted({1, 3, 32, 33, W, W + 1, 130}):
        R, stage, _ = _be().semiring_geometry(sr.TORCH_DTYPE[dtype], p)
        assert stage == S and R in (4, 8, 16, 32) and R * (S // 4 + 8) > S
        case = _structural(p, semiring)
        _check_forward(case, dtype, semiring, np.int64 if p == 33 else np.int32, p)
        empty = np.diff(case[0]) == 0
        assert empty.sum() == 4 and np.isinf(case[4][0][empty]).all() and (semiring == "log" or (case[4][1][empty] == -1).all())


@both
def test_row_counts_around_a_workgroup(dtype, semiring):
    for p in (1, 32, 33, 130):
        R = _be().semiring_geometry(sr.TORCH_DTYPE[dtype], p)[0]
        for n in sorted({1, R - 1, R, R + 1}):
            crow, col = sr.random_csr(n, 40, list(np.random.default_rng(n).integers(0, 6, size=n)), seed=n)
            rng = np.random.default_rng(3)
            val, B = _grid(rng.standard_normal(len(col))), _grid(rng.standard_normal((40, p)))
            _check_forward((crow, col, val, B, sr.forward(crow, col, val, B, semiring)), dtype, semiring, tag=(p, n))


@both
def test_special_values(dtype, semiring):
    inf, nan = np.inf, np.nan
    if semiring == "log":
        # rows: a lone -inf | -inf among numbers | gathers a -inf of B | nothing but -inf | +-80 | +-1e4 (exact in bfloat16) | +inf | NaN
        rows = [[-inf], [-inf, 1.0, 2.0], [0.5, 1.5], [-inf] * 3, [80.0, -80.0, 79.0], [9984.0, -9984.0, 9920.0], [1.0, inf, 2.0], [1.0, nan, 2.0]]
    else:
        # rows: a dozen ties from small integers (twice) | +0 against -0 | NaN first | NaN after a number
        rows = [list(sr.small_ints(12, 1)), list(sr.small_ints(12, 2)), [0.0, -0.0, 0.0, -0.0], [nan, 1.0, 2.0, nan], [1.0, 5.0, nan, 7.0, nan]]
    lens = [len(r) for r in rows]
    crow, col = sr.random_csr(len(rows), 20, lens, seed=8)
    val = np.array([x for r in rows for x in r])
    for p in (3, 32):
        B = sr.small_ints((20, p), 9) if semiring != "log" else _grid(np.random.default_rng(9).standard_normal((20, p)))
        if semiring == "log":
            B[col[crow[2]], 0] = -inf
        else:
            B[col[crow[2]:crow[3]]] = 0.0
        ref = sr.forward(crow, col, val, B, semiring)
        _check_forward((crow, col, val, B, ref), dtype, semiring, tag=p)
        if semiring != "log":
            assert (ref[1][2] == crow[2]).all() and (ref[1][3] == crow[3]).all() and (ref[1][4] == crow[4] + 2).all()
            continue
        assert (ref[0][[0, 3]] == -inf).all() and (ref[0][6] == inf).all() and np.isnan(ref[0][7]).all() and np.isfinite(ref[0][[1, 2, 4, 5]]).all()
        from torchsparsegradutils_amd import sparse_semiring_mm

        k = crow[6]                                   # the gradient of the six rows of numbers and absent entries
        A = torch.sparse_csr_tensor(_t(crow[:7]), _t(col[:k]), _t(val[:k], dtype), (6, 20)).requires_grad_(True)
        Bd = _t(B, dtype).requires_grad_(True)
        gA, gB = torch.autograd.grad(sparse_semiring_mm(A, Bd, "log").sum(), (A, Bd))
        dead = np.r_[crow[0]:crow[1], crow[1], crow[3]:crow[4]]
        assert (gA.values()[dead] == 0).all() and torch.isfinite(gA.values()).all() and torch.isfinite(gB).all()
        assert gB[col[crow[2]], 0] == 0 and abs(float(gA.values()[crow[4]:crow[5]].sum()) - p) < 2e-2 * p


def _grad_case(kind, p):
    rng = np.random.default_rng(11 + p)
    if kind == "random":
        n, m = 70, 50
        lens = list(rng.integers(0, 41, size=n))
        lens[0] = lens[-1] = 0
        shift = 300.0 if p == 33 else 0.0            # |C| ~ 300: a bfloat16 C in the exponent would be off by 2^-8·300
    else:                                            # column 0 is referenced by more rows than one staging pass holds
        n, m, shift = S + 70, 9, 0.0
        lens = [2] * n
    crow, col = sr.random_csr(n, m, lens, seed=p)
    if kind != "random":
        col[crow[:-1]] = 0
    return crow, col, rng.standard_normal(len(col)), rng.standard_normal((m, p)) + shift, rng.standard_normal((n, p))


@both
@pytest.mark.parametrize("kind,p", [("random", 3), ("random", 33), ("random", 130), ("hub", 3)])
def test_gradients_against_the_oracle_and_run_to_run(dtype, semiring, kind, p):
    from torchsparsegradutils_amd import sparse_semiring_mm

    crow, col, val, B, G = _grad_case(kind, p)
    val, B, G = (_as64(x, dtype) for x in (val, B, G))
    acc = np.float64 if semiring == "log" else sr.ACC[dtype]          # (the winners depend on the rounded addition)
    C64, arg64, wt = sr.forward(crow, col, val, B, semiring, acc)
    fb = sr.forward_bound(crow, C64, wt, U[dtype]) if semiring == "log" else None
    dval, bnd_a, dB, bnd_b = sr.gradients(crow, col, val, B, G, semiring, C64, arg64, fb, U[dtype], acc)
    runs = []
    for _ in range(2):
        A = torch.sparse_csr_tensor(_t(crow.astype(np.int32)), _t(col.astype(np.int32)), _t(val, dtype), (len(crow) - 1, B.shape[0])).requires_grad_(True)
        Bd = _t(B, dtype).requires_grad_(True)
        gA, gB = torch.autograd.grad(sparse_semiring_mm(A, Bd, semiring), (A, Bd), _t(G, dtype))
        runs.append((gA.values(), gB))
    assert sr.same_bits(runs[0][0], runs[1][0]) and sr.same_bits(runs[0][1], runs[1][1]), "two runs give the same bits"
    extra = U_BF16 if dtype == "bfloat16" else 0.0
    for got, want, bnd in ((runs[0][0], dval, bnd_a), (runs[0][1], dB, bnd_b)):
        excess = np.abs(got.double().cpu().numpy() - want) - (bnd + extra * (np.abs(want) + bnd))
        assert excess.max() <= 0, float(excess.max())


@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_layouts_and_batches(semiring):
    from torchsparsegradutils_amd import sparse_semiring_mm

    crow, col, val, B, G = _grad_case("random", 33)
    n, m = len(crow) - 1, B.shape[0]
    rows = np.repeat(np.arange(n), np.diff(crow))
    Bd, Gd = _t(B, "float32").requires_grad_(True), _t(G, "float32")

    def run(A, Bx=Bd, Gx=Gd):
        A = A.requires_grad_(True)
        C = sparse_semiring_mm(A, Bx, semiring)
        return (C,) + torch.autograd.grad(C, (A, Bx), Gx)

    csr = torch.sparse_csr_tensor(_t(crow), _t(col), _t(val, "float32"), (n, m))
    C0, gA0, gB0 = run(csr)
    assert gA0.layout == torch.sparse_csr and gA0.col_indices().data_ptr() == csr.col_indices().data_ptr()
    for idt in (torch.int32, torch.int64):
        coo = torch.sparse_coo_tensor(torch.stack([_t(rows), _t(col)]).to(idt), _t(val, "float32"), (n, m), is_coalesced=True)
        C, gA, gB = run(coo)
        assert sr.same_bits(C, C0) and sr.same_bits(gB, gB0) and sr.same_bits(gA._values(), gA0.values()) and gA.layout == torch.sparse_coo
        assert gA._indices().data_ptr() == coo._indices().data_ptr()
    half = _t(val, "float32") * 0.5                   # every entry stored twice, as halves: exact, so the coalesced sum is val
    dup = torch.sparse_coo_tensor(torch.stack([_t(rows), _t(col)]).repeat(1, 2), torch.cat([half, half]), (n, m))
    C, gA, gB = run(dup)
    assert sr.same_bits(C, C0) and sr.same_bits(gB, gB0) and gA.layout == torch.sparse_coo
    batched = torch.stack([csr.to_sparse_coo(), dup.coalesce()]).coalesce()
    Cb, gAb, gBb = run(batched, torch.stack([Bd, Bd]).detach().requires_grad_(True), torch.stack([Gd, Gd]))
    assert sr.same_bits(Cb[0], C0) and sr.same_bits(Cb[1], C0) and sr.same_bits(gBb[1], gB0) and gAb.shape == (2, n, m)


@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_graph_capture_replays_forward_and_backward_on_new_values(semiring):
    from torchsparsegradutils_amd import sparse_semiring_mm

    crow, col, val, B, G = _grad_case("random", 33)
    n, m = len(crow) - 1, B.shape[0]
    ci, cj, vals, Bd, Gd = _t(crow), _t(col), _t(val, "float32"), _t(B, "float32").requires_grad_(True), _t(G, "float32")

    def step():
        A = torch.sparse_csr_tensor(ci, cj, vals, (n, m)).requires_grad_(True)
        C = sparse_semiring_mm(A, Bd, semiring)
        gA, gB = torch.autograd.grad(C, (A, Bd), Gd)
        return C.detach(), gA.values().detach(), gB

    step()                                            # the pattern's caches are built outside the capture
    torch.cuda.synchronize()
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        outs = step()
    torch.cuda.current_stream().wait_stream(s)
    for k in range(3):
        vals.copy_(_t(np.random.default_rng(k).standard_normal(len(col)), "float32"))
        eager = [t.clone() for t in step()]
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(sr.same_bits(a, b) for a, b in zip(eager, outs)), k
