"""The 2:4 semi-structured kernels on the GPU (csrc/semi_impl.h) against the numpy restatement (tests/_semi_ref.py).

Exact cases hold small integers, so every product and sum is exact in float32, float64 and bfloat16's float32 accumulator and the
results must be EQUAL to the restatement's (a bfloat16 result is the exact value rounded once).  Random cases are held to the
counted-roundings bound of tests/test_gpu_sparse_bsr_mm.py (`_bound`, restated here): the terms really added are k / 2 for the
forward, m for Aᵀ·G and p for the SDDMM; stored zeros add no error."""

import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _semi_ref as sr
from torchsparsegradutils_amd import (SemiStructured, _backend, sparse_semi_structured_linear, sparse_semi_structured_mm,
                                      sparse_semi_structured_prune)
from torchsparsegradutils_amd import sparse_semi_structured as mod

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_semi.h")
F64 = torch.float64
BF16 = torch.bfloat16
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
NAN, INF = float("nan"), float("inf")
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
# (value type, bfloat16 on the sparse instruction?)
VARIANTS = [(torch.float32, True), (F64, True), (BF16, True), (BF16, False)]
VARIANT_IDS = ["f32", "f64", "bf16-smfmac", "bf16-expand"]

M_SIZES, P_SIZES, K_SIZES = (1, 15, 16, 17, 33), (1, 15, 17, 65), (4, 8, 28, 32, 36, 124, 128, 132, 260)
# the cross of the extremes, then a sample in which every size occurs
SHAPES = [(m, k, p) for m in (1, 33) for k in (4, 260) for p in (1, 65)] + [
    (15, 8, 15), (16, 28, 17), (17, 32, 1), (33, 36, 15), (1, 124, 17), (15, 128, 65), (16, 132, 1), (17, 260, 15), (16, 128, 17), (33, 132, 65)]
assert {s[0] for s in SHAPES} == set(M_SIZES) and {s[1] for s in SHAPES} == set(K_SIZES) and {s[2] for s in SHAPES} == set(P_SIZES)


def _bound(want, mag, dtype, chain):
    """tests/test_gpu_sparse_bsr_mm.py::_bound."""
    want, mag, chain = torch.as_tensor(want), torch.as_tensor(mag), torch.as_tensor(chain, dtype=torch.float64)
    if dtype == torch.bfloat16:
        # fp32 accumulation, one rounding: within one bf16 ulp of the exact value (plus the fp32 chain)
        ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (torch.floor(torch.log2(want.abs())) - 7))
        return ulp + chain * EPS[torch.float32] * mag * 2
    return chain * EPS[dtype] * mag + 1e-300


def _check(got, want, mag, dtype, chain, what=""):
    got, want = got.double().cpu(), torch.as_tensor(want)
    err = (got - want).abs()
    bound = _bound(want, mag, dtype, chain)
    worst = float((err - bound).max()) if err.numel() else 0.0
    print(f"{what}: max error {float(err.max()) if err.numel() else 0.0:.3e}, max (error - bound) {worst:.3e}")
    assert got.shape == want.shape and bool((err <= bound).all()), (what, worst)


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(DEV)


def _rounded(x, dtype):
    """The exact float64 result rounded once to the value type, as float64."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).double().numpy()


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


@pytest.fixture
def path(monkeypatch):
    def select(smfmac):
        monkeypatch.setattr(mod, "USE_SMFMAC", bool(smfmac))
    return select


def _run(S, values, dense, cot, linear, bias=None):
    """(forward, gradient of the values, gradient of the dense operand, gradient of the bias) through the public functions.  `dense`
    is B (k, p) and `cot` (m, p); with `linear` they are handed over as X = Bᵀ and Gᵀ and the results transposed back."""
    v = values.clone().requires_grad_(True)
    d = (dense.t().contiguous() if linear else dense).clone().requires_grad_(True)
    b = None if bias is None else bias.clone().requires_grad_(True)
    out = sparse_semi_structured_linear(d, S.with_values(v), b) if linear else sparse_semi_structured_mm(S.with_values(v), d)
    grads = torch.autograd.grad(out, (v, d) + (() if b is None else (b,)), cot.t().contiguous() if linear else cot)
    if linear:
        return out.detach().t(), grads[0], grads[1].t(), (grads[2] if b is not None else None)
    return out.detach(), grads[0], grads[1], None


# ---- the sparse instruction's positions -------------------------------------------------------------------------------------------

def _position_case():
    """Rows (pair t, group g, variant, row r of a 16-row tile), k = 128: group g keeps PAIRS[t] with the values (1, 0) or (0, 1), so
    a row's result names ONE kept position of one group; every other group holds stored zeros at a pair that differs from PAIRS[t].
    The dense operand holds distinct integers in [-64, 63]: a position taken from another lane, byte or bit pair changes the row."""
    k = 128
    rows = [(t, g, var, r) for t in range(6) for g in range(32) for var in range(2) for r in range(16)]
    m = len(rows)
    pattern, values = np.zeros((m, k)), np.zeros((m, k // 2))
    for i, (t, g, var, r) in enumerate(rows):
        for other in range(32):
            pair = PAIRS[t] if other == g else PAIRS[(t + 1 + abs(other - g) % 5) % 6]
            pattern[i, 4 * other + pair[0]] = pattern[i, 4 * other + pair[1]] = 1.0
        values[i, 2 * g + var] = 1.0
    c = np.arange(k)
    B = np.stack([c - 64, (c * 5) % 128 - 64], axis=1).astype(np.float64)
    return rows, pattern, values, B


@pytest.mark.parametrize("smfmac", [True, False], ids=["smfmac", "expand"])
def test_positions_bf16(path, smfmac):
    path(smfmac)
    rows, pattern, values, B = _position_case()
    S = SemiStructured.from_dense(_dev(pattern, BF16))
    _, cols = sr.prune(pattern)
    assert np.array_equal(S.indices().cpu().numpy(), cols)
    for i, (t, g, var, r) in enumerate(rows[::97]):
        assert tuple(cols[97 * i, 2 * g:2 * g + 2] - 4 * g) == PAIRS[t] and 97 * i % 16 == r
    want = sr.mm(values, cols, 128, B)[0]
    assert np.array_equal(want[:, 0], np.array([4 * g + PAIRS[t][var] - 64 for t, g, var, r in rows], dtype=np.float64))
    out = sparse_semi_structured_mm(S.with_values(_dev(values, BF16)), _dev(B, BF16))
    assert np.array_equal(out.double().cpu().numpy(), want)
    lin = sparse_semi_structured_linear(_dev(B.T, BF16), S.with_values(_dev(values, BF16)))
    assert np.array_equal(lin.double().cpu().numpy(), want.T)


def test_positions_differ_in_the_lane_quarters_of_one_instruction(path):
    """All eight groups of each 32-column instruction hold different pairs in its four lane quarters, every kept value is live."""
    rng = np.random.default_rng(5)
    m, k, p = 48, 256, 16
    pattern = np.zeros((m, k))
    for i in range(m):
        for g in range(k // 4):
            pair = PAIRS[(i + i // 16 + g + (g % 8) // 6) % 6]
            pattern[i, 4 * g + pair[0]] = pattern[i, 4 * g + pair[1]] = 1.0
    values, B = _ints(rng, (m, k // 2), 1, 2), _ints(rng, (k, p), -1, 1) + np.arange(k)[:, None] % 3
    _, cols = sr.prune(pattern)
    quarters = (cols.reshape(m, k // 32, 4, 4) % 4)[..., [0, 1]]                    # (row, instruction, quarter, first group's pair)
    assert all(len({tuple(x) for x in quarters[i, s]}) == 4 for i in range(m) for s in range(k // 32))
    want = _rounded(sr.mm(values, cols, k, B)[0], BF16)
    outs = []
    for smfmac in (True, False):
        path(smfmac)
        S = SemiStructured.from_dense(_dev(pattern, BF16)).with_values(_dev(values, BF16))
        outs.append(sparse_semi_structured_mm(S, _dev(B, BF16)))
        assert np.array_equal(outs[-1].double().cpu().numpy(), want)
    assert torch.equal(outs[0], outs[1])


# ---- tails and boundaries: integers, equality ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("linear", [False, True], ids=["mm", "linear"])
@pytest.mark.parametrize("dtype,smfmac", VARIANTS, ids=VARIANT_IDS)
def test_shapes_exact(path, dtype, smfmac, linear):
    path(smfmac)
    rng = np.random.default_rng(7)
    for m, k, p in SHAPES:
        W, B, G = _ints(rng, (m, k)), _ints(rng, (k, p)), _ints(rng, (m, p))
        S = sparse_semi_structured_prune(_dev(W, dtype))
        values, cols = sr.prune(W)
        assert np.array_equal(S.indices().cpu().numpy(), cols) and np.array_equal(S.values.double().cpu().numpy(), values)
        out, dv, dd, _ = _run(S, S.values, _dev(B, dtype), _dev(G, dtype), linear)
        what = f"(m, k, p) = {(m, k, p)}"
        assert np.array_equal(out.double().cpu().numpy(), _rounded(sr.mm(values, cols, k, B)[0], dtype)), what
        assert np.array_equal(dv.double().cpu().numpy(), _rounded(sr.sddmm(cols, G, B)[0], dtype)), what
        assert np.array_equal(dd.double().cpu().numpy(), _rounded(sr.mm_t(values, cols, k, G)[0], dtype)), what


@pytest.mark.parametrize("linear", [False, True], ids=["mm", "linear"])
def test_the_two_bf16_paths_agree_bit_for_bit(path, linear):
    rng = np.random.default_rng(8)
    for m, k, p in SHAPES:
        W, B, G = _ints(rng, (m, k)), _ints(rng, (k, p)), _ints(rng, (m, p))
        S = sparse_semi_structured_prune(_dev(W, BF16))
        outs = []
        for smfmac in (True, False):
            path(smfmac)
            outs.append(_run(S, S.values, _dev(B, BF16), _dev(G, BF16), linear)[0])
        assert torch.equal(outs[0], outs[1]), (m, k, p)


# ---- random data: the counted-roundings bound ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("linear", [False, True], ids=["mm", "linear"])
@pytest.mark.parametrize("dtype,smfmac", VARIANTS, ids=VARIANT_IDS)
def test_random_forward_and_gradients(path, dtype, smfmac, linear):
    path(smfmac)
    for seed, (m, k, p) in enumerate([(33, 260, 65), (70, 132, 15), (17, 516, 130)]):
        rng = np.random.default_rng(100 + seed)
        as_type = lambda x: torch.from_numpy(x).to(dtype)                  # noqa: E731  (the values the device sees)
        W, B, G, bias = (as_type(rng.standard_normal(s)) for s in ((m, k), (k, p), (m, p), (m,)))
        S = sparse_semi_structured_prune(W.to(DEV))
        values, cols = sr.prune(W.double().numpy())
        assert np.array_equal(S.indices().cpu().numpy(), cols)
        out, dv, dd, db = _run(S, S.values, B.to(DEV), G.to(DEV), linear, bias.to(DEV) if linear else None)
        Bn, Gn = B.double().numpy(), G.double().numpy()
        want, mag, chain = sr.mm(values, cols, k, Bn)
        if linear:                                                         # the bias is one more term of the same sum
            want, mag, chain = want + bias.double().numpy()[:, None], mag + bias.double().abs().numpy()[:, None], chain + 1
            _check(db, Gn.sum(1), np.abs(Gn).sum(1), dtype, p, "grad bias")
        what = f"{'linear' if linear else 'mm'} {dtype} smfmac={smfmac} (m, k, p) = {(m, k, p)}"
        _check(out, want, mag, dtype, chain, what + " forward")
        _check(dv, *sr.sddmm(cols, Gn, Bn)[:2], dtype, p, what + " grad values")
        _check(dd, *sr.mm_t(values, cols, k, Gn)[:2], dtype, m, what + " grad dense")


# ---- prune and expand -----------------------------------------------------------------------------------------------------------------

def _special_rows(dtype):
    groups = [[0, 0, 0, 0], [0, 0, 0, 5], [0, 3, 0, 0], [1, 2, 3, 0], [4, 3, 2, 1], [1, 1, 1, 1], [-1, 1, -1, 1], [2, -2, 1, 2], [1, 2, 2, 2],
              [-0.0, 0.0, -0.0, 0.0], [0.0, -0.0, 1, -0.0], [-0.0, -0.0, -0.0, -1], [NAN, 1, 2, 3], [1, INF, NAN, 2], [INF, -INF, NAN, NAN],
              [NAN, NAN, NAN, NAN], [-INF, 1, INF, 7], [INF, INF, -INF, INF], [1, NAN, INF, -INF], [0, NAN, 0, 0], [0.5, -0.25, 0.25, -0.5]]
    rows = [sum((groups[(i + j) % len(groups)] for j in range(len(groups))), []) for i in range(5)]
    return torch.tensor(rows, dtype=F64).to(dtype)


def _bits(t):
    return t.cpu().view({BF16: torch.int16, torch.float32: torch.int32, F64: torch.int64}[t.dtype])


@pytest.mark.parametrize("dtype", [torch.float32, F64, BF16], ids=["f32", "f64", "bf16"])
def test_prune_equals_the_cpu_path_and_expand_is_the_masked_matrix(dtype):
    rng = np.random.default_rng(11)
    cases = [_special_rows(dtype)] + [torch.from_numpy(_ints(rng, (m, k), -2, 2)).to(dtype) for m, k in ((1, 4), (33, 260), (17, 124))] + [
        torch.from_numpy(rng.standard_normal((70, 132))).to(dtype)]
    wide = torch.from_numpy(rng.standard_normal((19, 140))).to(dtype)
    for W, Wd in [(W, W.to(DEV)) for W in cases] + [(wide[:, 3:139], wide.to(DEV)[:, 3:139])]:      # the last one: rows off 16-byte alignment
        cpu, gpu = sparse_semi_structured_prune(W), sparse_semi_structured_prune(Wd)
        assert gpu.device.type == "cuda" and torch.equal(gpu.indices().cpu(), cpu.indices())
        assert torch.equal(_bits(gpu.values), _bits(cpu.values)), "the kept values are copies, NaN payloads and zero signs included"
        assert torch.equal(gpu.meta.cpu(), cpu.meta), "one packed layout on both devices"
        mask = torch.zeros(W.shape, dtype=torch.bool).scatter_(1, cpu.indices(), True)
        assert torch.equal(_bits(gpu.to_dense()), _bits(torch.where(mask, W, torch.zeros_like(W))))
        # prune's gradient is the expansion of the cotangent
        Wg = Wd.clone().requires_grad_(True)
        Gv = torch.from_numpy(_ints(rng, (W.size(0), W.size(1) // 2), 1, 3)).to(dtype).to(DEV)
        (gW,) = torch.autograd.grad(sparse_semi_structured_prune(Wg).values, Wg, Gv)
        assert torch.equal(gW.cpu(), torch.zeros(W.shape, dtype=dtype).scatter_(1, cpu.indices(), Gv.cpu()))


# ---- bias, views, graphs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,smfmac", VARIANTS, ids=VARIANT_IDS)
def test_linear_with_bias_and_leading_dimensions(path, dtype, smfmac):
    path(smfmac)
    rng = np.random.default_rng(12)
    out_f, k = 37, 132
    W, X, bias = _ints(rng, (out_f, k)), _ints(rng, (2, 3, 5, k)), _ints(rng, (out_f,), -9, 9)
    S = sparse_semi_structured_prune(_dev(W, dtype))
    values, cols = sr.prune(W)
    Xd, bd = _dev(X, dtype).requires_grad_(True), _dev(bias, dtype).requires_grad_(True)
    out = sparse_semi_structured_linear(Xd, S, bd)
    want = sr.mm(values, cols, k, X.reshape(-1, k).T)[0].T + bias[None, :]
    assert out.shape == (2, 3, 5, out_f) and np.array_equal(out.detach().double().cpu().numpy().reshape(-1, out_f), _rounded(want, dtype))
    G = _ints(rng, (2, 3, 5, out_f), -1, 1)
    gX, gb = torch.autograd.grad(out, (Xd, bd), _dev(G, dtype))
    assert gX.shape == Xd.shape and np.array_equal(gb.double().cpu().numpy(), G.reshape(-1, out_f).sum(0))
    assert np.array_equal(gX.double().cpu().numpy().reshape(-1, k), _rounded(sr.mm_t(values, cols, k, G.reshape(-1, out_f).T)[0].T, dtype))


@pytest.mark.parametrize("linear", [False, True], ids=["mm", "linear"])
@pytest.mark.parametrize("dtype,smfmac", VARIANTS, ids=VARIANT_IDS)
def test_unaligned_views(path, dtype, smfmac, linear):
    """`values`, the dense operand and the cotangent as column slices of wider tensors: their rows start off 16-byte alignment, so
    the staging takes its scalar path."""
    path(smfmac)
    rng = np.random.default_rng(13)
    m, k, p = 35, 140, 21
    W, B, G = _ints(rng, (m, k)), _ints(rng, (k, p)), _ints(rng, (m, p))
    S = sparse_semi_structured_prune(_dev(W, dtype))
    values, cols = sr.prune(W)
    wide_v = torch.zeros((m, k // 2 + 5), dtype=dtype, device=DEV)
    wide_v[:, 3:3 + k // 2] = S.values
    v_view = wide_v[:, 3:3 + k // 2]
    dense, cot = (B.T, G.T) if linear else (B, G)
    wide_d = torch.full((dense.shape[0], dense.shape[1] + 4), 7.0, dtype=dtype, device=DEV)
    wide_d[:, 1:1 + dense.shape[1]] = _dev(dense, dtype)
    wide_g = torch.full((cot.shape[0], cot.shape[1] + 4), 7.0, dtype=dtype, device=DEV)
    wide_g[:, 3:3 + cot.shape[1]] = _dev(cot, dtype)
    d_view, g_view = wide_d[:, 1:1 + dense.shape[1]], wide_g[:, 3:3 + cot.shape[1]]
    assert not v_view.is_contiguous() and v_view.data_ptr() % 16 and d_view.data_ptr() % 16 and g_view.data_ptr() % 16
    v = v_view.detach().requires_grad_(True)
    d = d_view.detach().requires_grad_(True)
    out = sparse_semi_structured_linear(d, S.with_values(v)) if linear else sparse_semi_structured_mm(S.with_values(v), d)
    dv, dd = torch.autograd.grad(out, (v, d), g_view)
    fix = (lambda x: x.T) if linear else (lambda x: x)
    assert np.array_equal(out.detach().double().cpu().numpy(), _rounded(fix(sr.mm(values, cols, k, B)[0]), dtype))
    assert np.array_equal(dv.double().cpu().numpy(), _rounded(sr.sddmm(cols, G, B)[0], dtype))
    assert np.array_equal(dd.double().cpu().numpy(), _rounded(fix(sr.mm_t(values, cols, k, G)[0]), dtype))


def test_forward_and_backward_are_captured_in_a_graph():
    rng = np.random.default_rng(14)
    out_f, k, tokens = 40, 132, 50
    S = sparse_semi_structured_prune(_dev(rng.standard_normal((out_f, k)), BF16))
    v = S.values.clone().requires_grad_(True)
    X = _dev(rng.standard_normal((tokens, k)), BF16).requires_grad_(True)
    bias = _dev(rng.standard_normal(out_f), BF16).requires_grad_(True)
    G = _dev(rng.standard_normal((tokens, out_f)), BF16)

    def step():
        out = sparse_semi_structured_linear(X, S.with_values(v), bias)
        return (out,) + torch.autograd.grad(out, (v, X, bias), G)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.detach().clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    for t in held:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(held, eager):
        assert torch.equal(got.detach(), want), "the replay is bit-identical to the eager result"
    assert float(eager[0].abs().max()) > 0 and float(eager[1].abs().max()) > 0


# ---- the C ABI on the device ------------------------------------------------------------------------------------------------------------

def test_refusals_through_the_c_abi_launch_nothing():
    lib = _backend.load_library()
    m, k, p = 20, 136, 9
    W = torch.randn((m, k), dtype=torch.float32, device=DEV)
    S = sparse_semi_structured_prune(W)
    val, meta = S.values, S.meta
    Y = torch.randn((p, k), dtype=torch.float32, device=DEV)
    G = torch.randn((m, p), dtype=torch.float32, device=DEV)
    Yk = torch.randn((k, p), dtype=torch.float32, device=DEV)
    SENT = 12345.0
    outs = {n: torch.full(s, SENT, dtype=torch.float32, device=DEV) for n, s in
            (("C", (m, p)), ("D", (k, p)), ("dv", (m, k // 2)), ("dense", (m, k)), ("val2", (m, k // 2)))}
    meta2 = torch.full_like(meta, 77)
    stream = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()                                               # noqa: E731
    calls = {
        "tsgu_semi_prune": dict(vtype=0, W=P(W), ldw=k, m=m, k=k, val=P(outs["val2"]), ldv=k // 2, meta=P(meta2), ldm=8),
        "tsgu_semi_expand": dict(vtype=0, val=P(val), ldv=k // 2, meta=P(meta), ldm=8, m=m, k=k, out=P(outs["dense"]), ldo=k),
        "tsgu_semi_mm": dict(vtype=0, val=P(val), ldv=k // 2, meta=P(meta), ldm=8, Y=P(Y), ldy=k, bias=None, C=P(outs["C"]), ldc=p, m=m, k=k,
                             p=p, flags=0, path=0),
        "tsgu_semi_mm_t": dict(vtype=0, val=P(val), ldv=k // 2, meta=P(meta), ldm=8, G=P(G), ldg=p, D=P(outs["D"]), ldd=p, m=m, k=k, p=p,
                               flags=0),
        "tsgu_semi_sddmm": dict(vtype=0, G=P(G), ldg=p, Y=P(Yk), ldy=p, meta=P(meta), ldm=8, out=P(outs["dv"]), ldo=k // 2, m=m, k=k, p=p,
                                flags=0),
    }
    header = dict(A.prototypes(HEADER))
    for name, base in calls.items():
        fn = getattr(lib, name)

        def call(**ch):
            a = dict(base)
            a.update(ch)
            return fn(*a.values(), 0, stream)

        assert [q[0] for q in header[name][:-2]] == list(base), "the call names the header's parameters"
        for pn, pt in header[name][:-2]:
            if pt.endswith("*") and pn != "bias":
                assert call(**{pn: None}) == A.BAD_ARG, (name, pn)
        assert call(k=k + 2) == A.BAD_ARG and call(k=-4) == A.BAD_ARG and call(m=-1) == A.BAD_ARG, name
        assert call(vtype=3) == A.BAD_DTYPE and call(vtype=-1) == A.BAD_DTYPE, name
        assert call(ldm=4) == A.BAD_ARG and call(meta=base["meta"] + 4) == A.BAD_ARG, name
        if "p" in base:
            assert call(p=-1) == A.BAD_ARG and call(flags=8) == A.BAD_ARG, name
        if name == "tsgu_semi_mm":
            assert call(path=1) == A.BAD_ARG, "the sparse instruction is bfloat16's"
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in outs.values()) and bool((meta2 == 77).all()), "nothing was launched"
    for name, base in calls.items():
        assert getattr(lib, name)(*base.values(), 0, stream) == A.OK, name
    torch.cuda.synchronize()
    assert all(not bool((t == SENT).any()) for t in outs.values()) and torch.equal(meta2, meta) and torch.equal(outs["val2"], val)
    assert torch.equal(outs["dense"], S.to_dense())
    values, cols = sr.prune(W.double().cpu().numpy())
    _check(outs["C"], *sr.mm(values, cols, k, Y.double().cpu().numpy().T)[:2], torch.float32, k // 2, "C ABI forward")
    _check(outs["D"], *sr.mm_t(values, cols, k, G.double().cpu().numpy())[:2], torch.float32, m, "C ABI transposed")
    _check(outs["dv"], *sr.sddmm(cols, G.double().cpu().numpy(), Yk.double().cpu().numpy())[:2], torch.float32, p, "C ABI sddmm")
