"""neighbor_mm on the MI355X: every lane, offset and stage exact on integer data for every value and index type around the tile,
stage and chunk edges; accuracy against float64 on random data within the bound of the summation lengths; the error word, strided
operands, determinism, the empty result and the voxel tables."""
import pytest
import torch

import _conv_ref as cr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend as _be

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53, torch.bfloat16: 2.0 ** -24}   # (bf16: fp32 accumulation)
N_IN = 200
# whole offsets packed per stage; a stage tail; the unaligned scalar path; D1 > KC in fp32 / fp64; D1 > KC in bf16
SHAPES = [(1, 1, 1), (27, 16, 16), (5, 20, 17), (3, 3, 65), (2, 65, 64), (9, 130, 33)]
_DATA = {}


def _integer_case(n_out, K, d1, d2):
    """(x, w, g, bias, nbr, reference) of one shape, computed once and shared by the value and index types."""
    key = (n_out, K, d1, d2)
    if key not in _DATA:
        gen = torch.Generator().manual_seed(1000 * n_out + K)
        x, w, g, bias = cr.integers(N_IN, n_out, K, d1, d2, gen)
        nbr = cr.table(N_IN, n_out, K, gen)
        _DATA[key] = (x, w, g, bias, nbr, cr.reference(x, w, nbr, bias, g))
    return _DATA[key]


def _run(x, w, nbr, bias, g, dtype, itype):
    xs, ws, bs = (t.to(DEV, dtype).requires_grad_(True) for t in (x, w, bias))
    out = tsgu.neighbor_mm(xs, ws, nbr.to(DEV, itype), bs)
    assert out.dtype == dtype and out.shape == g.shape
    gx, gw, gb = torch.autograd.grad(out, (xs, ws, bs), g.to(DEV, dtype))
    return {"out": out.detach(), "grad_x": gx, "grad_w": gw, "grad_bias": gb}


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,d1,d2", SHAPES)
@pytest.mark.parametrize("n_out", [1, 127, 129, 257])
def test_exact_on_integers(n_out, K, d1, d2, dtype, itype):
    x, w, g, bias, nbr, ref = _integer_case(n_out, K, d1, d2)
    got = _run(x, w, nbr, bias, g, dtype, itype)
    for name, val in got.items():
        want = ref[name].to(dtype).double()            # every sum is an integer below 2^24: exact, for bf16 rounded once
        bad = (val.double().cpu() != want).nonzero()
        assert bad.numel() == 0, (name, bad[:4].tolist(), val.double().cpu()[tuple(bad[0])].item(), want[tuple(bad[0])].item())


def _check(got, want, mag, dtype, chain):
    got = got.double().cpu()
    if dtype == torch.bfloat16:    # fp32 accumulation, one rounding: within one bf16 ulp of the exact value (plus the fp32 chain)
        ulp = torch.where(want == 0, torch.zeros_like(want), 2.0 ** (torch.floor(torch.log2(want.abs())) - 7))
        bound = ulp + chain * EPS[torch.float32] * mag * 2
    else:
        bound = chain * EPS[dtype] * mag + 1e-300
    err = (got - want).abs()
    print(f"max error / bound: {float((err / bound.clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_data_against_float64(dtype):
    n, K, d1, d2 = 700, 27, 70, 45
    gen = torch.Generator().manual_seed(7)
    x, w, g, bias = (torch.randn(s, generator=gen).to(dtype) for s in ((n, d1), (K, d1, d2), (n, d2), (d2,)))
    nbr = cr.table(n, n, K, gen)
    ref = cr.reference(x, w, nbr, bias, g)
    got = _run(x, w, nbr, bias, g, dtype, torch.int32)
    _, chunk_rows, chunks, _ = _be.neighbor_mm_geometry(dtype, n, K, d1, d2)
    for name, chain in (("out", K * d1), ("grad_x", K * d2), ("grad_w", chunk_rows + chunks), ("grad_bias", n)):
        _check(got[name], ref[name], ref[name + "_mag"], dtype, chain)


def test_the_error_word():
    x, w = torch.zeros(6, 4, device=DEV), torch.zeros(3, 4, 5, device=DEV)
    for rows in ([[0, 1, 6]], [[2, -1, -1], [2, -1, -1]]):
        with pytest.raises(RuntimeError, match=r"neighbor_mm \(nbr holds entries >= n_in, or a column that names one input twice\)"):
            tsgu.neighbor_mm(x, w, torch.tensor(rows, device=DEV))


@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_views_and_determinism(dtype):
    n_out, K, d1, d2 = 257, 5, 20, 17
    x, w, g, bias, nbr, _ = _integer_case(n_out, K, d1, d2)
    base = _run(x, w, nbr, bias, g, dtype, torch.int64)
    again = _run(x, w, nbr, bias, g, dtype, torch.int64)
    assert torch.equal(base["grad_w"], again["grad_w"])
    nb, gd = nbr.to(DEV), g.to(DEV, dtype)
    xv = torch.zeros(2 * N_IN, d1 + 3, device=DEV, dtype=dtype)[::2, 1:1 + d1].copy_(x)           # row stride, unaligned rows
    wv = torch.zeros(K, 2 * d1, d2 + 1, device=DEV, dtype=dtype)[:, ::2, :d2].copy_(w)
    wt = w.to(DEV, dtype).transpose(1, 2).contiguous().transpose(1, 2)                             # (K, d1, d2) with d1 contiguous
    for xs, ws in ((xv, wv), (x.to(DEV, dtype), wt)):
        xs, ws = xs.requires_grad_(True), ws.requires_grad_(True)
        out = tsgu.neighbor_mm(xs, ws, nb, bias.to(DEV, dtype))
        gx, gw = torch.autograd.grad(out, (xs, ws), gd)
        for name, val in (("out", out.detach()), ("grad_x", gx), ("grad_w", gw)):
            assert torch.equal(val, base[name]), name


def test_empty_results_and_voxel_tables():
    x, w = torch.ones(6, 4, device=DEV, requires_grad=True), torch.ones(3, 4, 5, device=DEV, requires_grad=True)
    out = tsgu.neighbor_mm(x, w, torch.empty((0, 3), dtype=torch.int32, device=DEV))
    assert out.shape == (0, 5)
    gx, gw = torch.autograd.grad(out.sum(), (x, w))
    assert not gx.any() and not gw.any()
    gen = torch.Generator().manual_seed(3)
    coords = torch.unique(torch.cat([torch.randint(0, 2, (300, 1), generator=gen), torch.randint(-4, 5, (300, 3), generator=gen)], 1), dim=0)
    offsets = tsgu.kernel_offsets(3)
    assert torch.equal(tsgu.voxel_neighbors(coords.to(DEV), offsets).cpu(), tsgu.voxel_neighbors(coords, offsets))
