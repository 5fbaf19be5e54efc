"""gather_mm / segment_mm on CPU operands: the reference's exported names, golden parity with the reference's own outputs and
gradients, its validation errors, this package's own semantics (N = 0, fp64, bf16, out-of-range indices, integer index dtypes),
and the plans' offsets and tile prefix against a numpy model."""
import json
import os

import numpy as np
import pytest
import torch

import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend as _be
from torchsparsegradutils_amd import indexed_matmul as imm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = np.load(os.path.join(HERE, "golden", "indexed_mm.npz"))
CASES = sorted({k.split(".")[0] for k in GOLDEN.files})
with open(os.path.join(HERE, "golden", "indexed_mm_errors.json")) as f:
    ERRORS = json.load(f)
REFERENCE_ALL = ["sparse_mm", "gather_mm", "segment_mm", "sparse_triangular_solve", "sparse_generic_solve",
                 "sparse_generic_lstsq", "sparse_logsumexp", "sparse_bidir_logsumexp"]


def test_every_reference_name_is_exported():
    for name in REFERENCE_ALL:
        assert name in tsgu.__all__ and callable(getattr(tsgu, name)), name


def _call(name, device="cpu"):
    meta = json.loads(str(GOLDEN[f"{name}.meta"]))
    a = torch.from_numpy(GOLDEN[f"{name}.a"]).to(device).requires_grad_(True)
    b = torch.from_numpy(GOLDEN[f"{name}.b"]).to(device).requires_grad_(True)
    idx = torch.from_numpy(GOLDEN[f"{name}.idx"]).to(device)
    fn = tsgu.segment_mm if meta["fn"] == "segment" else tsgu.gather_mm
    out = fn(a, b, idx)
    w = torch.from_numpy(GOLDEN[f"{name}.w"]).to(device)
    ga, gb = torch.autograd.grad((out * w).sum(), (a, b))
    return out, ga, gb


@pytest.mark.parametrize("name", CASES)
def test_golden_outputs_and_gradients(name):
    out, ga, gb = _call(name)
    assert out.dtype == torch.float32
    for got, key in ((out, "out"), (ga, "ga"), (gb, "gb")):
        want = torch.from_numpy(GOLDEN[f"{name}.{key}"])
        assert got.shape == want.shape, key
        torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-4, msg=key)


def _error_args(name):
    a, b = torch.randn(10, 4), torch.randn(2, 4, 3)
    seg = {
        "segment_old_torch": (a, b, torch.tensor([5, 5])),
        "segment_a_1d": (a[0], b, torch.tensor([5, 5])),
        "segment_b_2d": (a, b[0], torch.tensor([5, 5])),
        "segment_seglen_2d": (a, b, torch.tensor([[5, 5]])),
        "segment_d1_mismatch": (torch.randn(10, 5), b, torch.tensor([5, 5])),
        "segment_r_mismatch": (a, b, torch.tensor([5, 3, 2])),
    }
    a, b = torch.randn(3, 4), torch.randn(2, 4, 5)
    gat = {
        "gather_old_torch": (a, b, torch.tensor([0, 1, 0])),
        "gather_not_tensor_a": (a.tolist(), b, torch.tensor([0, 1, 0])),
        "gather_not_tensor_idx": (a, b, [0, 1, 0]),
        "gather_a_1d": (a[0], b, torch.tensor([0, 1, 0])),
        "gather_b_2d": (a, b[0], torch.tensor([0, 1, 0])),
        "gather_idx_2d": (a, b, torch.tensor([[0, 1, 0]])),
        "gather_n_mismatch": (a, b, torch.tensor([0, 1])),
        "gather_d1_mismatch": (torch.randn(3, 5), b, torch.tensor([0, 1, 0])),
    }
    return {**seg, **gat}[name]


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_validation_errors_match_the_reference(name, monkeypatch):
    e = ERRORS[name]
    if name.endswith("old_torch"):
        monkeypatch.setattr(torch, "__version__", "2.3.0")
    with pytest.raises(Exception) as info:
        getattr(imm, e["fn"])(*_error_args(name))
    assert type(info.value).__name__ == e["type"]
    assert str(info.value) == e["msg"]


def test_own_checks():
    a, b = torch.randn(6, 3), torch.randn(2, 3, 4)
    with pytest.raises(TypeError):
        tsgu.gather_mm(a, b.double(), torch.zeros(6, dtype=torch.long))
    with pytest.raises(TypeError):
        tsgu.gather_mm(a.half(), b.half(), torch.zeros(6, dtype=torch.long))
    with pytest.raises(TypeError):
        tsgu.gather_mm(a, b, torch.zeros(6))
    with pytest.raises(TypeError):
        tsgu.segment_mm(a, b, torch.tensor([3.0, 3.0]))
    with pytest.raises(ValueError, match="negative"):
        tsgu.segment_mm(a, b, torch.tensor([7, -1]))
    # other integer dtypes are converted
    idx = torch.tensor([1, 0, 1, 1, 0, 0], dtype=torch.int16)
    torch.testing.assert_close(tsgu.gather_mm(a, b, idx), tsgu.gather_mm(a, b, idx.long()))
    torch.testing.assert_close(tsgu.segment_mm(a, b, torch.tensor([2, 4], dtype=torch.uint8)),
                               torch.cat([a[:2] @ b[0], a[2:] @ b[1]]))


def test_empty_rows():
    b = torch.randn(3, 4, 5, requires_grad=True)
    a = torch.randn(0, 4, requires_grad=True)
    for out in (tsgu.gather_mm(a, b, torch.zeros(0, dtype=torch.long)), tsgu.segment_mm(a, b, torch.tensor([0, 0, 0]))):
        assert out.shape == (0, 5) and out.dtype == torch.float32
        ga, gb = torch.autograd.grad(out.sum(), (a, b))
        assert ga.shape == (0, 4) and torch.equal(gb, torch.zeros_like(b))


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16])
def test_fp64_and_bf16_compute_in_their_own_dtype(dtype):
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(20, 6, generator=g).to(dtype), torch.randn(4, 6, 3, generator=g).to(dtype)
    idx = torch.randint(0, 4, (20,), generator=g)
    out = tsgu.gather_mm(a, b, idx)
    assert out.dtype == dtype
    want = torch.einsum("nk,nkj->nj", a.double(), b.double()[idx])
    tol = 1e-12 if dtype == torch.float64 else 2e-2
    torch.testing.assert_close(out.double(), want, atol=tol, rtol=tol)
    out = tsgu.segment_mm(a, b, torch.tensor([5, 0, 9, 6]))
    assert out.dtype == dtype


def test_out_of_range_rows_are_zero_and_reported(monkeypatch):
    a = torch.randn(6, 3, requires_grad=True)
    b = torch.randn(2, 3, 4, requires_grad=True)
    idx = torch.tensor([1, -1, 0, 2, 1, 5])
    with pytest.raises(RuntimeError, match="outside"):
        tsgu.gather_mm(a, b, idx)
    monkeypatch.setattr(_be, "_SYNC_CHECK", False)
    out = tsgu.gather_mm(a, b, idx)
    with pytest.raises(RuntimeError, match="outside"):
        tsgu.poll_errors(block=True)
    ok = torch.tensor([True, False, True, False, True, False])
    assert torch.equal(out[~ok], torch.zeros(3, 4))
    torch.testing.assert_close(out[ok], torch.einsum("nk,nkj->nj", a[ok], b[idx[ok]]))
    ga, gb = torch.autograd.grad(out.sum(), (a, b))
    assert torch.equal(ga[~ok], torch.zeros(3, 3))
    want_gb = torch.stack([a[ok & (idx == r)].sum(0)[:, None].expand(3, 4) for r in range(2)])
    torch.testing.assert_close(gb, want_gb.detach())
    # the plan is cached: the check ran once for this index tensor
    tsgu.gather_mm(a, b, idx)
    tsgu.poll_errors(block=True)


def _np_plan(groups_of_rows, n, r, bm):
    """numpy model: extended offsets [0, s_0 .. s_R, n] and the tile prefix of the R + 2 extended segments."""
    ext = np.concatenate([[0], groups_of_rows, [n]]).astype(np.int64)
    tiles = (np.diff(ext) + bm - 1) // bm
    return ext, np.concatenate([[0], np.cumsum(tiles)])


@pytest.mark.parametrize("seed", range(4))
def test_plans_against_a_numpy_model(seed):
    rng = np.random.default_rng(seed)
    bm = imm.TILE_ROWS
    n, r = int(rng.integers(0, 1000)), int(rng.integers(1, 12))
    idx = rng.integers(-2, r + 2, n)
    p = imm.gather_plan(torch.from_numpy(idx), r)
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(p.perm.numpy(), order)
    bounds = np.searchsorted(idx[order], np.arange(r + 1), side="left")
    ext, tp = _np_plan(bounds, n, r, bm)
    assert np.array_equal(p.offsets.numpy(), ext) and np.array_equal(p.tile_ptr.numpy(), tp)
    assert int(p.bad) == int(((idx < 0) | (idx >= r)).sum())
    assert tp[-1] <= p.max_tiles == -(-n // bm) + min(r, n) + 2

    lens = rng.integers(0, 2 * max(n, 1) // r + 2, r)
    p = imm.segment_plan(torch.from_numpy(lens), n, torch.device("cpu"))
    bounds = np.concatenate([[0], np.minimum(np.cumsum(lens[:-1]), n), [n]])
    ext, tp = _np_plan(bounds, n, r, bm)
    assert p.perm is None and int(p.bad) == 0
    assert np.array_equal(p.offsets.numpy(), ext) and np.array_equal(p.tile_ptr.numpy(), tp)
    assert tp[-1] <= p.max_tiles
    for chunk in (1, 3, 256):
        cp, pp = p.chunks(chunk)
        nch = (np.diff(bounds) + chunk - 1) // chunk
        assert np.array_equal(cp.numpy(), np.concatenate([[0], np.cumsum(nch)]))
        assert np.array_equal(pp.numpy(), np.concatenate([[0], np.cumsum(np.where(nch > 1, nch, 0))]))
        assert pp.numpy()[-1] <= 2 * -(-n // chunk)


def test_plan_cache_reuse_and_inplace_rebuild():
    a, b = torch.randn(10, 3), torch.randn(3, 3, 2)
    idx = torch.randint(0, 3, (10,))
    imm.clear_plans()
    before = imm.STATS["built"]
    tsgu.gather_mm(a, b, idx)
    tsgu.gather_mm(a, b, idx)
    assert imm.STATS["built"] == before + 1
    idx[0] = (idx[0] + 1) % 3
    out = tsgu.gather_mm(a, b, idx)
    assert imm.STATS["built"] == before + 2
    torch.testing.assert_close(out, torch.einsum("nk,nkj->nj", a, b[idx]))


def test_noncontiguous_and_stride0_gradients():
    g = torch.Generator().manual_seed(5)
    a = torch.randn(9, 14, generator=g)[:, ::2].requires_grad_(True)
    b = torch.randn(3, 5, 7, generator=g).transpose(1, 2).requires_grad_(True)
    seglen = torch.tensor([2, 3, 4])
    out = tsgu.segment_mm(a, b, seglen)
    ga, gb = torch.autograd.grad(out.sum(), (a, b))
    a2, b2 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    ref = torch.cat([a2[:2] @ b2[0], a2[2:5] @ b2[1], a2[5:] @ b2[2]])
    ra, rb = torch.autograd.grad(ref.sum(), (a2, b2))
    torch.testing.assert_close(out, ref)
    torch.testing.assert_close(ga, ra)
    torch.testing.assert_close(gb, rb)


def test_gradcheck_fp64():
    g = torch.Generator().manual_seed(6)
    a = torch.randn(7, 3, dtype=torch.float64, generator=g, requires_grad=True)
    b = torch.randn(3, 3, 2, dtype=torch.float64, generator=g, requires_grad=True)
    idx = torch.tensor([2, 0, 2, 1, 0, 2, 2])
    assert torch.autograd.gradcheck(lambda x, y: tsgu.gather_mm(x, y, idx), (a, b))
    assert torch.autograd.gradcheck(lambda x, y: tsgu.segment_mm(x, y, torch.tensor([3, 0, 4])), (a, b))
