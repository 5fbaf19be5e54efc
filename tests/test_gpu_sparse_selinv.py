"""sparse_selected_inverse on the MI355X (csrc/selinv_impl.h): the cases and bounds of tests/_selinv_ref.py, error words, repeats."""

import pytest
import torch

import _selinv_ref as R
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("dtype,itype,layout", R.KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_the_kernel_against_the_dense_inverse(name, dtype, itype, layout, ldlt):
    R.check(name, _backend.selinv_geometry(dtype)[0], dtype, itype, layout, ldlt, DEV)


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_columns_on_both_sides_of_the_staged_capacity(dtype, ldlt):
    """A dense lower block two longer than the capacity: its first columns work in the Σ array itself, the others in LDS (the arrow
    cases straddle the capacity in n only: their columns hold five entries).  The bits do not depend on the grid."""
    cap = _backend.selinv_geometry(dtype)[0]
    Z1, d1 = R.check("dense", cap, dtype, torch.int32, torch.sparse_csr, ldlt, DEV, workgroups_per_cu=1)
    Z8, d8 = R.check("dense", cap, dtype, torch.int32, torch.sparse_csr, ldlt, DEV, workgroups_per_cu=8)
    assert torch.equal(Z1.values(), Z8.values()) and (d1 is None or torch.equal(d1, d8))


@pytest.mark.parametrize("name", ["band", "blocks", "random"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_two_calls_and_two_grids_give_the_same_bits(name, dtype):
    F, mask, _, _ = R.case(name)
    for ldlt in (False, True):
        L, D = R.operands(F, mask, dtype, torch.int64, torch.sparse_csr, ldlt, DEV)
        runs = [tsgu.sparse_selected_inverse(L, D, workgroups_per_cu=w) for w in (1, 1, 8)]
        vals = [torch.cat((r[0].values(), r[1])) if ldlt else r.values() for r in runs]
        assert torch.equal(vals[0], vals[1]) and torch.equal(vals[0], vals[2])


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_pattern_that_is_not_closed(dtype, ldlt):
    L = R.open_stencil(dtype, DEV)
    D = None
    if ldlt:
        L, D = torch.tril(L.to_dense(), -1).to_sparse_coo(), torch.full((42,), 2.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError, match=r"column 0 needs an entry .* closed under elimination"):
        tsgu.sparse_selected_inverse(L, D)
    res = tsgu.sparse_selected_inverse(L, D, check=False)
    assert (res[0] if ldlt else res).selinv_info.tolist() == [0, 1]


def test_a_zero_pivot_is_reported_and_the_call_returns():
    R.check_zero_pivot(DEV)


def test_the_grad_guard():
    F, mask, _, _ = R.case("blocks")
    L, _ = R.operands(F, mask, torch.float64, torch.int64, torch.sparse_coo, False, DEV)
    with pytest.raises(NotImplementedError, match="not differentiable: the adjoint recurrence is not implemented"):
        tsgu.sparse_selected_inverse(L.requires_grad_(True))


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("layout", [torch.sparse_coo, torch.sparse_csr])
def test_marginal_variance(layout, ldlt):
    R.check_marginal_variance(layout, ldlt, DEV)


def test_ic0_of_the_cholesky_pattern_is_an_exact_factor_the_kernel_accepts():
    """The route from a precision matrix: cholesky_pattern → sparse_ic0 → sparse_selected_inverse, against the dense inverse."""
    A = R._laplacian(6, 7, 0.5)
    L = tsgu.sparse_ic0(tsgu.cholesky_pattern(A.to(DEV))).L
    Z = tsgu.sparse_selected_inverse(L)
    want = torch.linalg.inv(A.to_dense())
    got = Z.to_dense().cpu()
    assert float((got - torch.where(got != 0, want, got)).norm() / want.norm()) < 1e-10
