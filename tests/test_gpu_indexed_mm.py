"""gather_mm / segment_mm on the MI355X: golden parity, the MFMA lane maps bit for bit, accuracy against float64 for every
value and index dtype, edge shapes of the tile and chunk schedule, gradcheck, out-of-range indices, determinism, the plan
cache and a graph capture."""
import json
import os

import numpy as np
import pytest
import torch

import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend as _be
from torchsparsegradutils_amd import indexed_matmul as imm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "indexed_mm.npz"))
CASES = sorted({k.split(".")[0] for k in GOLDEN.files})
BM = imm.TILE_ROWS
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24}   # (bf16: fp32 accumulation)


def _golden(name):
    meta = json.loads(str(GOLDEN[f"{name}.meta"]))
    a = torch.from_numpy(GOLDEN[f"{name}.a"]).to(DEV).requires_grad_(True)
    b = torch.from_numpy(GOLDEN[f"{name}.b"]).to(DEV).requires_grad_(True)
    idx = torch.from_numpy(GOLDEN[f"{name}.idx"]).to(DEV)
    return meta, a, b, idx


@pytest.mark.parametrize("seglen_on_host", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_golden_parity(name, seglen_on_host):
    meta, a, b, idx = _golden(name)
    if meta["fn"] == "segment":
        out = tsgu.segment_mm(a, b, idx.cpu() if seglen_on_host else idx)
    else:
        out = tsgu.gather_mm(a, b, idx)
    w = torch.from_numpy(GOLDEN[f"{name}.w"]).to(DEV)
    ga, gb = torch.autograd.grad((out * w).sum(), (a, b))
    for got, key in ((out, "out"), (ga, "ga"), (gb, "gb")):
        torch.testing.assert_close(got.cpu(), torch.from_numpy(GOLDEN[f"{name}.{key}"]), atol=1e-6, rtol=1e-4, msg=key)


def _model(a, b, groups, g=None):
    """float64 model: out (and with g: grad_a, grad_b) plus the Σ|terms| of each element."""
    a64, b64 = a.double().cpu(), b.double().cpu()
    bg = b64[groups.clamp(0, b.size(0) - 1)] * ((groups >= 0) & (groups < b.size(0))).double()[:, None, None]
    out = torch.einsum("nk,nkj->nj", a64, bg)
    mag = torch.einsum("nk,nkj->nj", a64.abs(), bg.abs())
    if g is None:
        return out, mag
    g64 = g.double().cpu()
    ga = torch.einsum("nj,nkj->nk", g64, bg)
    ga_mag = torch.einsum("nj,nkj->nk", g64.abs(), bg.abs())
    onehot = torch.zeros(a.size(0), b.size(0), dtype=torch.float64)
    ok = (groups >= 0) & (groups < b.size(0))
    onehot[ok.nonzero()[:, 0], groups[ok]] = 1
    gb = torch.einsum("nr,nk,nj->rkj", onehot, a64, g64)
    gb_mag = torch.einsum("nr,nk,nj->rkj", onehot, a64.abs(), g64.abs())
    return out, mag, ga, ga_mag, gb, gb_mag


def _seg_groups(seglen, n):
    bounds = [0] + [min(int(x), n) for x in torch.cumsum(seglen[:-1], 0)] + [n]
    groups = torch.empty(n, dtype=torch.int64)
    for r in range(len(seglen)):
        groups[bounds[r]:bounds[r + 1]] = r
    return groups


def _check(got, want, mag, dtype, chain):
    got = got.double().cpu()
    if dtype == torch.bfloat16:
        # fp32 accumulation, one rounding: within one bf16 ulp of the exact value (plus the fp32 chain)
        ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (torch.floor(torch.log2(want.abs())) - 7))
        bound = ulp + chain * EPS[torch.float32] * mag * 2
    else:
        bound = chain * EPS[dtype] * mag + 1e-300
    err = (got - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())


def _chunk_chain(n, r, d1, d2, dtype, lens):
    chunk, _, _ = _be.segment_mm_grad_b_workspace(dtype, n, r, d1, d2)
    return chunk + max(1, -(-max(lens) // chunk))


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
@pytest.mark.parametrize("fn", ["gather", "segment"])
def test_against_float64(fn, dtype, itype):
    g = torch.Generator().manual_seed(11)
    n, r, d1, d2 = 3000, 9, 70, 45
    a = torch.randn(n, d1, generator=g).to(dtype)
    b = torch.randn(r, d1, d2, generator=g).to(dtype)
    w = torch.randn(n, d2, generator=g).to(dtype)
    if fn == "gather":
        groups = torch.randint(0, r, (n,), generator=g)
        idx = groups.to(itype)
    else:
        idx = torch.tensor([500, 0, 731, 129, 128, 127, 1, 1000, 9999], dtype=itype)
        groups = _seg_groups(idx, n)
    lens = torch.bincount(groups, minlength=r).tolist()
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = (tsgu.gather_mm if fn == "gather" else tsgu.segment_mm)(ad, bd, idx.to(DEV))
    assert out.dtype == dtype
    ga, gb = torch.autograd.grad(out, (ad, bd), w.to(DEV))
    want, mag, wa, wa_mag, wb, wb_mag = _model(a, b, groups, w)
    _check(out, want, mag, dtype, d1)
    _check(ga, wa, wa_mag, dtype, d2)
    _check(gb, wb, wb_mag, dtype, _chunk_chain(n, r, d1, d2, dtype, lens))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_lane_maps_bit_exact(dtype):
    """Small integers and an asymmetric b: every product and sum is exact, so a misplaced MFMA lane shows as a wrong value."""
    g = torch.Generator().manual_seed(12)
    n, r, d1, d2 = 700, 5, 37, 41
    a = torch.randint(-4, 5, (n, d1), generator=g).to(dtype)
    b = (torch.arange(d1)[:, None] * 3 - torch.arange(d2)[None, :] * 2 + torch.arange(r)[:, None, None] * 5).to(dtype)
    gw = torch.randint(-3, 4, (n, d2), generator=g).to(dtype)
    groups = torch.randint(0, r, (n,), generator=g)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = tsgu.gather_mm(ad, bd, groups.to(DEV))
    ga, gb = torch.autograd.grad(out, (ad, bd), gw.to(DEV))
    want, _, wa, _, wb, _ = _model(a, b, groups, gw)
    assert torch.equal(out.double().cpu(), want)
    assert torch.equal(ga.double().cpu(), wa)
    assert torch.equal(gb.double().cpu(), wb)


def test_bf16_fp32_accumulation_one_rounding():
    """Operands exact in bf16 whose sums are exact in fp32 but not in bf16: the result is the exact sum rounded once."""
    n, r, d1, d2 = 300, 3, 64, 24
    g = torch.Generator().manual_seed(13)
    a = (torch.randint(1, 128, (n, d1), generator=g).float())           # 7-bit integers: exact in bf16
    b = (torch.randint(1, 128, (r, d1, d2), generator=g).float())
    groups = torch.randint(0, r, (n,), generator=g)
    exact = torch.einsum("nk,nkj->nj", a.double(), b.double()[groups])   # < 2^24: exact in fp32, not in bf16
    out = tsgu.gather_mm(a.bfloat16().to(DEV), b.bfloat16().to(DEV), groups.to(DEV))
    assert torch.equal(out.cpu(), exact.float().bfloat16())


@pytest.mark.parametrize("d1,d2", [(1, 1), (7, 15), (16, 17), (17, 16), (129, 7), (15, 129), (64, 64), (128, 128), (256, 200)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_tails_and_segment_lengths(d1, d2, dtype):
    g = torch.Generator().manual_seed(d1 * 1000 + d2)
    lens = [0, 1, BM - 1, BM, BM + 1, 0, 2 * BM + 3, 0]
    n, r = sum(lens), len(lens)
    a = torch.randn(n, d1, generator=g).to(dtype)
    b = torch.randn(r, d1, d2, generator=g).to(dtype)
    w = torch.randn(n, d2, generator=g).to(dtype)
    seglen = torch.tensor(lens)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = tsgu.segment_mm(ad, bd, seglen.to(DEV))
    ga, gb = torch.autograd.grad(out, (ad, bd), w.to(DEV))
    groups = _seg_groups(seglen, n)
    want, mag, wa, wa_mag, wb, wb_mag = _model(a, b, groups, w)
    _check(out, want, mag, dtype, d1)
    _check(ga, wa, wa_mag, dtype, d2)
    _check(gb, wb, wb_mag, dtype, _chunk_chain(n, r, d1, d2, dtype, lens))
    assert torch.equal(gb[0].cpu(), torch.zeros(d1, d2, dtype=dtype))


def test_many_relations_few_rows():
    g = torch.Generator().manual_seed(14)
    n, r, d1, d2 = 9000, 4096, 24, 40
    a, b = torch.randn(n, d1, generator=g), torch.randn(r, d1, d2, generator=g)
    w = torch.randn(n, d2, generator=g)
    groups = torch.randint(0, r, (n,), generator=g)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = tsgu.gather_mm(ad, bd, groups.to(DEV))
    ga, gb = torch.autograd.grad(out, (ad, bd), w.to(DEV))
    want, mag, wa, wa_mag, wb, wb_mag = _model(a, b, groups, w)
    _check(out, want, mag, torch.float32, d1)
    _check(ga, wa, wa_mag, torch.float32, d2)
    _check(gb, wb, wb_mag, torch.float32, _chunk_chain(n, r, d1, d2, torch.float32, torch.bincount(groups).tolist()))


def test_one_long_segment_splits_grad_b():
    n, d1, d2 = 1 << 20, 32, 48
    g = torch.Generator().manual_seed(15)
    a, b = torch.randn(n, d1, generator=g), torch.randn(1, d1, d2, generator=g)
    w = torch.randn(n, d2, generator=g)
    chunk, _, _ = _be.segment_mm_grad_b_workspace(torch.float32, n, 1, d1, d2)
    assert chunk < n          # the split path
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = tsgu.segment_mm(ad, bd, torch.tensor([n]))
    ga, gb = torch.autograd.grad(out, (ad, bd), w.to(DEV))
    torch.testing.assert_close(out.cpu(), a @ b[0], atol=1e-4, rtol=1e-5)
    torch.testing.assert_close(ga.cpu(), w @ b[0].t(), atol=1e-4, rtol=1e-5)
    a64, w64 = a.double(), w.double()
    want = (a64.t() @ w64)[None]
    mag = (a64.abs().t() @ w64.abs())[None]
    _check(gb, want, mag, torch.float32, chunk + -(-n // chunk))


def test_noncontiguous_operands_and_stride0_gradient():
    g = torch.Generator().manual_seed(16)
    n, r, d1, d2 = 500, 4, 33, 20
    a = torch.randn(d1 * 2, n, generator=g).t()[:, ::2]                  # neither row- nor column-major
    b = torch.randn(r, d2, d1, generator=g).transpose(1, 2)              # k contiguous
    groups = torch.randint(0, r, (n,), generator=g)
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    out = tsgu.gather_mm(ad, bd, groups.to(DEV))
    ga, gb = torch.autograd.grad(out.sum(), (ad, bd))                    # a stride-0 output gradient
    want, mag, wa, wa_mag, wb, wb_mag = _model(a, b, groups, torch.ones(n, d2))
    _check(out, want, mag, torch.float32, d1)
    _check(ga, wa, wa_mag, torch.float32, d2)
    _check(gb, wb, wb_mag, torch.float32, _chunk_chain(n, r, d1, d2, torch.float32, torch.bincount(groups).tolist()))


def test_gradcheck_fp64():
    g = torch.Generator().manual_seed(17)
    a = torch.randn(21, 5, dtype=torch.float64, generator=g).to(DEV).requires_grad_(True)
    b = torch.randn(4, 5, 3, dtype=torch.float64, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, 4, (21,), generator=g).to(DEV)
    assert torch.autograd.gradcheck(lambda x, y: tsgu.gather_mm(x, y, idx), (a, b))
    seglen = torch.tensor([6, 0, 10, 5], device=DEV)
    assert torch.autograd.gradcheck(lambda x, y: tsgu.segment_mm(x, y, seglen), (a, b))


def test_out_of_range_indices(monkeypatch):
    a = torch.randn(300, 8, device=DEV, requires_grad=True)
    b = torch.randn(3, 8, 5, device=DEV, requires_grad=True)
    idx = torch.randint(0, 3, (300,), device=DEV)
    idx[::7] = -2
    idx[3::11] = 3
    ok = (idx >= 0) & (idx < 3)
    with pytest.raises(RuntimeError, match="outside"):
        tsgu.gather_mm(a, b, idx)
    monkeypatch.setattr(_be, "_SYNC_CHECK", False)
    out = tsgu.gather_mm(a, b, idx)
    with pytest.raises(RuntimeError, match="outside"):
        tsgu.poll_errors(block=True)
    assert torch.equal(out[~ok], torch.zeros_like(out[~ok]))
    torch.testing.assert_close(out[ok], torch.einsum("nk,nkj->nj", a[ok], b[idx[ok]]))
    ga, gb = torch.autograd.grad(out.sum(), (a, b))
    assert torch.equal(ga[~ok], torch.zeros_like(ga[~ok]))
    want_gb = torch.stack([a[ok & (idx == r)].sum(0)[:, None].expand(8, 5) for r in range(3)])
    torch.testing.assert_close(gb, want_gb.detach(), atol=1e-5, rtol=1e-5)
    seglen = torch.tensor([100, -5, 205], device=DEV)
    tsgu.segment_mm(a, b, seglen)
    with pytest.raises(RuntimeError, match="negative"):
        tsgu.poll_errors(block=True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_repeat_calls_are_bit_identical(dtype):
    g = torch.Generator().manual_seed(18)
    n, r, d1, d2 = 200000, 3, 64, 64
    a = torch.randn(n, d1, generator=g).to(dtype).to(DEV).requires_grad_(True)
    b = torch.randn(r, d1, d2, generator=g).to(dtype).to(DEV).requires_grad_(True)
    idx = torch.randint(0, r, (n,), generator=g).to(DEV)
    w = torch.randn(n, d2, generator=g).to(dtype).to(DEV)
    first = None
    for _ in range(3):
        out = tsgu.gather_mm(a, b, idx)
        res = (out,) + torch.autograd.grad(out, (a, b), w)
        if first is None:
            first = res
        for x, y in zip(first, res):
            assert torch.equal(x, y)


def test_plan_cache_reuse_and_inplace_rebuild():
    a, b = torch.randn(1000, 16, device=DEV), torch.randn(5, 16, 8, device=DEV)
    idx = torch.randint(0, 5, (1000,), device=DEV)
    imm.clear_plans()
    before = imm.STATS["built"]
    tsgu.gather_mm(a, b, idx)
    tsgu.gather_mm(a, b, idx)
    assert imm.STATS["built"] == before + 1
    idx[:10] = (idx[:10] + 1) % 5
    out = tsgu.gather_mm(a, b, idx)
    assert imm.STATS["built"] == before + 2
    torch.testing.assert_close(out, torch.einsum("nk,nkj->nj", a, b[idx]))


def test_graph_capture_replays_eager():
    g = torch.Generator().manual_seed(19)
    n, r, d1, d2 = 5000, 6, 48, 40
    a = torch.randn(n, d1, generator=g).to(DEV).requires_grad_(True)
    b = torch.randn(r, d1, d2, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, r, (n,), generator=g).to(DEV)
    seglen = torch.tensor([900, 0, 1100, 1000, 1500, 500])
    w = torch.randn(n, d2, generator=g).to(DEV)

    def step():
        out = tsgu.gather_mm(a, b, idx) + tsgu.segment_mm(a, b, seglen)
        return (out,) + torch.autograd.grad(out, (a, b), w)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, captured):
        assert torch.equal(x, y)


def test_reference_test_shapes_drop_in():
    """The reference test file's own calls and tolerances (test_indexed_matmul.py), on the GPU."""
    for _ in range(2):
        n, r, d1, d2 = 100, 32, 7, 10
        a, b = torch.randn((n, d1), device=DEV), torch.randn((r, d1, d2), device=DEV)
        seglen = torch.randint(low=1, high=int(n / r), size=(r,), device=DEV)
        seglen[-1] = n - seglen[:-1].sum()
        ab = tsgu.segment_mm(a, b, seglen)
        k = 0
        for i in range(r):
            for _j in range(seglen[i]):
                assert torch.allclose(ab[k], a[k] @ b[i], atol=1e-6, rtol=1e-4)
                k += 1
        idx = torch.randint(low=0, high=r, size=(n,), device=DEV)
        ab = tsgu.gather_mm(a, b, idx)
        for i in range(n):
            assert torch.allclose(ab[i], a[i] @ b[idx[i]], atol=1e-6, rtol=1e-4)
