"""sparse_selected_inverse / cholesky_pattern / marginal_variance without a GPU: _cpu.selected_inverse against the dense float64
inverse (tests/_selinv_ref.py), the error behaviour and the refusals."""

import pytest
import torch

import _selinv_ref as R
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend

CPU = torch.device("cpu")


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("dtype,itype,layout", R.KINDS)
@pytest.mark.parametrize("name", R.CASES)
def test_the_column_loop_against_the_dense_inverse(name, dtype, itype, layout, ldlt):
    R.check(name, _backend.selinv_geometry(dtype)[0], dtype, itype, layout, ldlt, CPU)


@pytest.mark.parametrize("ldlt", [False, True])
def test_a_pattern_that_is_not_closed(ldlt):
    L = R.open_stencil(torch.float64, CPU)
    D = None
    if ldlt:
        L, D = torch.tril(L.to_dense(), -1).to_sparse_coo(), torch.full((42,), 2.0, dtype=torch.float64)
    with pytest.raises(ValueError, match=r"column 0 needs an entry .* closed under elimination"):
        tsgu.sparse_selected_inverse(L, D)
    res = tsgu.sparse_selected_inverse(L, D, check=False)
    assert (res[0] if ldlt else res).selinv_info.tolist() == [0, 1]


def test_a_zero_pivot_is_reported_and_the_call_returns():
    R.check_zero_pivot(CPU)


def test_refusals_and_the_grad_guard():
    F, mask, _, _ = R.case("blocks")
    L, D = R.operands(F, mask, torch.float64, torch.int64, torch.sparse_csr, True, CPU)
    with pytest.raises(NotImplementedError, match="not differentiable: the adjoint recurrence is not implemented"):
        tsgu.sparse_selected_inverse(L.requires_grad_(True), D)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        tsgu.sparse_selected_inverse(L.detach(), D.clone().requires_grad_(True))
    with torch.no_grad():
        tsgu.sparse_selected_inverse(L, D)
    L = L.detach()
    with pytest.raises(ValueError, match="column 0 does not store its diagonal"):
        tsgu.sparse_selected_inverse(L)
    with pytest.raises(ValueError, match="on or above the diagonal: L must be strictly lower"):
        tsgu.sparse_selected_inverse(R.operands(F, mask, torch.float64, torch.int64, torch.sparse_csr, False, CPU)[0], D)
    with pytest.raises(ValueError, match="column 1 stores an entry above the diagonal"):
        tsgu.sparse_selected_inverse(torch.tensor([[1.0, 2.0], [0.0, 1.0]]).to_sparse_csr())
    with pytest.raises(TypeError, match="float32 and float64 operands only, got torch.bfloat16"):
        tsgu.sparse_selected_inverse(torch.eye(3, dtype=torch.bfloat16).to_sparse_coo())
    with pytest.raises(ValueError, match="batched operands are not supported"):
        tsgu.sparse_selected_inverse(torch.eye(3).expand(2, 3, 3).to_sparse_coo())
    with pytest.raises(ValueError, match="either COO or CSR sparse format"):
        tsgu.sparse_selected_inverse(torch.eye(3).to_sparse_csc())
    with pytest.raises(ValueError, match=r"diagonal must have shape \(63,\)"):
        tsgu.sparse_selected_inverse(L, D[:5])
    assert {"sparse_selected_inverse", "cholesky_pattern", "SparseSelectedInverse"} <= set(tsgu.__all__)


@pytest.mark.parametrize("ldlt", [False, True])
@pytest.mark.parametrize("layout", [torch.sparse_coo, torch.sparse_csr])
def test_marginal_variance(layout, ldlt):
    R.check_marginal_variance(layout, ldlt, CPU)
