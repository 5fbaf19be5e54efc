"""neighbor_mm / voxel_neighbors / kernel_offsets without a GPU: the torch-op path of _cpu.py against the float64 reference
(tests/_conv_ref.py), the tables against a dictionary lookup, the refusals, and the geometry query of include/tsgu_hip_conv.h."""

import pytest
import torch

import _abi_cases as A
import _conv_ref as cr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_in,n_out,K,d1,d2", [(200, 257, 5, 20, 17), (200, 127, 27, 4, 6), (40, 40, 1, 1, 1), (0, 9, 3, 4, 5)])
def test_the_torch_op_path_against_the_reference(dtype, n_in, n_out, K, d1, d2):
    gen = torch.Generator().manual_seed(5)
    x, w, g, bias = cr.integers(n_in, n_out, K, d1, d2, gen)
    nbr = cr.table(n_in, n_out, K, gen, torch.int32) if n_in else torch.full((n_out, K), -1, dtype=torch.int32)
    ref = cr.reference(x, w, nbr, bias, g)
    xs, ws, bs = (t.to(dtype).requires_grad_(True) for t in (x, w, bias))
    out = tsgu.neighbor_mm(xs, ws, nbr, bs)
    assert out.dtype == dtype and out.shape == (n_out, d2)
    grads = torch.autograd.grad(out, (xs, ws, bs), g.to(dtype))
    for name, got in zip(("out", "grad_x", "grad_w", "grad_bias"), (out.detach(),) + grads):
        assert torch.equal(got.double(), ref[name].to(dtype).double()), name      # integers: exact, bf16 rounded once
    assert torch.equal(tsgu.neighbor_mm(xs, ws, nbr).detach().double(), (ref["out"] - bias).to(dtype).double())
    assert torch.equal(out[n_out // 2].detach().double(), bias.to(dtype).double())   # a row without neighbours gives the bias


def _lookup(coords, offsets, out_coords):
    where = {tuple(c): j for j, c in enumerate(coords.tolist())}
    return torch.tensor([[where.get(tuple(a + b for a, b in zip(o, off)), -1) for off in offsets.tolist()] for o in out_coords.tolist()])


def test_voxel_tables_against_a_dictionary():
    gen = torch.Generator().manual_seed(2)
    grid = torch.cartesian_prod(torch.arange(2), torch.arange(-2, 3), torch.arange(4), torch.arange(3))
    coords = grid[torch.randperm(grid.size(0), generator=gen)[:48]]
    offsets = tsgu.kernel_offsets(3)
    assert offsets.shape == (27, 4) and offsets[0].tolist() == [0, -1, -1, -1] and offsets[1].tolist() == [0, -1, -1, 0]
    assert tsgu.kernel_offsets((2, 3), dilation=2, batch=False).tolist() == [[0, -2], [0, 0], [0, 2], [2, -2], [2, 0], [2, 2]]
    nbr = tsgu.voxel_neighbors(coords, offsets)
    assert nbr.dtype == torch.int64 and torch.equal(nbr, _lookup(coords, offsets, coords))
    assert torch.equal(nbr[:, 13], torch.arange(48))
    # a strided layer: outputs at the even voxels, in the input's coordinate system; and int32 coordinates give an int32 table
    out_coords = torch.unique(coords // torch.tensor([1, 2, 2, 2]) * torch.tensor([1, 2, 2, 2]), dim=0)
    got = tsgu.voxel_neighbors(coords.int(), tsgu.kernel_offsets(2), out_coords.int())
    assert got.dtype == torch.int32 and torch.equal(got.long(), _lookup(coords, tsgu.kernel_offsets(2), out_coords))
    with pytest.raises(RuntimeError, match=r"voxel_neighbors \(coords holds duplicate rows\)"):
        tsgu.voxel_neighbors(torch.cat([coords, coords[5:6]]), offsets)
    # the tables feed neighbor_mm: the inverse exists, so the gradient of x is the transposed convolution
    x = torch.randn(48, 3, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = torch.randn(27, 3, 2, dtype=torch.float64, generator=gen)
    gx, = torch.autograd.grad(tsgu.neighbor_mm(x, w, nbr).sum(), x)
    torch.testing.assert_close(gx, cr.reference(x.detach(), w, nbr, None, torch.ones(48, 2))["grad_x"], rtol=1e-12, atol=1e-12)


def test_refusals():
    x, w, nbr = torch.zeros(6, 4), torch.zeros(3, 4, 5), torch.full((7, 3), -1)
    with pytest.raises(ValueError, match="Input tensors have unexpected dimensions"):
        tsgu.neighbor_mm(x, w[0], nbr)
    with pytest.raises(ValueError, match="Incompatible size for inputs"):
        tsgu.neighbor_mm(x, w, nbr[:, :2])
    with pytest.raises(ValueError, match="Incompatible size for inputs"):
        tsgu.neighbor_mm(x, w, nbr, torch.zeros(4))
    with pytest.raises(TypeError, match="x and w must have the same dtype, got torch.float32 and torch.float64"):
        tsgu.neighbor_mm(x, w.double(), nbr)
    with pytest.raises(TypeError, match="unsupported value dtype torch.float16"):
        tsgu.neighbor_mm(x.half(), w.half(), nbr)
    with pytest.raises(TypeError, match="nbr must be an integer tensor, got torch.float32"):
        tsgu.neighbor_mm(x, w, nbr.float())
    with pytest.raises(RuntimeError, match=r"neighbor_mm \(nbr holds entries >= n_in, or a column that names one input twice\)"):
        tsgu.neighbor_mm(x, w, torch.tensor([[0, 1, 6]] * 1))
    with pytest.raises(RuntimeError, match=r"neighbor_mm \(nbr holds entries >= n_in"):
        tsgu.neighbor_mm(x, w, torch.tensor([[2, -1, -1], [2, -1, -1]]))
    with pytest.raises(ValueError, match="Incompatible size for inputs"):
        tsgu.voxel_neighbors(torch.zeros(3, 5, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64))


def test_geometry():
    lib = _backend.load_library()
    # the geometry the GPU tests take their summation lengths from: 256-row chunks until the launch has 2048 workgroups
    assert _backend.neighbor_mm_geometry(torch.float32, 700, 27, 70, 45) == (128, 256, 3, 3 * 27 * 70 * 45 * 4)
    assert _backend.neighbor_mm_geometry(torch.float64, 256, 9, 130, 33) == (128, 256, 1, 16)
    assert _backend.neighbor_mm_geometry(torch.bfloat16, 1 << 18, 27, 64, 64) == (128, 4096, 64, 64 * 27 * 64 * 64 * 4)
    assert lib.tsgu_neighbor_mm_geometry(9, 1, 1, 1, 1, None, None, None, None) == A.BAD_ARG
