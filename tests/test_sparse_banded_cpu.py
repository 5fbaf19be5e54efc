"""sparse_banded_triangular_solve without a GPU: the validation of sparse_triangular_solve, CPU operands, the widths band_plan reports
and the geometry queries of include/tsgu_hip_band.h."""

import numpy as np
import pytest
import torch

import _trsm_ref as R
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern

def csr(ptr, idx, val):
    n = len(ptr) - 1
    return torch.sparse_csr_tensor(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(val), (n, n))


def test_geometry():
    lib = _backend.load_library()
    assert _backend.band_geometry(torch.float32, 1 << 20, 8, 3) == (64, 32, 256)
    assert lib.tsgu_csr_band_sptrsm_work_bytes(_backend.TSGU_F32, 1 << 20, 8, 9, 0, 0) == 0          # wider than the cap


BAD = [
    (lambda: ("A", torch.ones(3, 2))),
    (lambda: (torch.ones(3), torch.ones(3))),
    (lambda: (torch.eye(3).to_sparse_csr(), torch.ones(1, 3, 2))),
    (lambda: (torch.eye(3), torch.ones(3, 2))),
    (lambda: (torch.eye(3).to_sparse_csr(), torch.ones(3, 2).to_sparse())),
    (lambda: (torch.ones(3, 4).to_sparse_csr(), torch.ones(3, 2))),
    (lambda: (torch.eye(3).to_sparse_csr(), torch.ones(4, 2))),
    (lambda: (torch.stack([torch.eye(3)] * 2).to_sparse_coo(), torch.ones(3, 3, 2))),
]


@pytest.mark.parametrize("make", BAD)
def test_validation_messages_are_those_of_sparse_triangular_solve(make):
    a, b = make()
    with pytest.raises(ValueError) as want:
        tsgu.sparse_triangular_solve(a, b)
    with pytest.raises(ValueError) as got:
        tsgu.sparse_banded_triangular_solve(a, b)
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("mode", R.MODES)
def test_cpu_operands_return_what_sparse_triangular_solve_returns(mode):
    c = R.Case("chain", 33, "f64", mode, 3)
    kw = dict(upper=c.upper, unitriangular=c.unit, transpose=c.transpose)
    out = []
    for fn in (tsgu.sparse_triangular_solve, tsgu.sparse_banded_triangular_solve):
        M, B = csr(*c.api).requires_grad_(True), torch.from_numpy(c.B).requires_grad_(True)
        X = fn(M, B, **kw)
        gA, gB = torch.autograd.grad(X, (M, B), torch.from_numpy(c.G))
        out.append((X.detach(), gA.values(), gB))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert R.rel_err(out[1][0].numpy(), c.forward()[0]) < 1e-12


def test_band_plan_reports_the_width_of_each_side():
    widths = lambda M: tuple(_pattern.band_plan(_pattern.from_csr(M), lower=side).width for side in (True, False))
    assert widths(csr(*R.chain(40))) == (1, 0)
    assert widths(csr(*R.diag_only(5))) == (0, 0)
    for w in (2, 3, 8, 9):
        assert widths(csr(*R.pattern(64, R.SEED, band=w))) == (w, 0)
        assert widths(csr(*R.to_upper(*R.pattern(64, R.SEED, band=w)))) == (0, w)
    both = R.dense(*R.pattern(64, R.SEED, band=3)) + np.triu(R.dense(*R.to_upper(*R.pattern(64, R.SEED, band=5))), 1)          # an L \ U array
    assert widths(torch.from_numpy(both).to_sparse_csr()) == (3, 5)
    unsorted = torch.sparse_csr_tensor(torch.tensor([0, 1, 3]), torch.tensor([0, 1, 0]), torch.ones(3), (2, 2))
    with pytest.raises(ValueError, match="strictly ascending"):
        _pattern.band_plan(_pattern.from_csr(unsorted), lower=True)
