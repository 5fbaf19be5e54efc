"""sparse_spgemm without a GPU: the numpy restatement of the GPU tests pinned to torch.sparse.mm(A, B) and its autograd on the
CPU, the CPU path of sparse_spgemm for COO and CSR operands, every refusal, and the fifth C-ABI header with its host-side
refusals."""

import numpy as np
import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import _spgemm_ref as sr
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_spgemm

DTYPES = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}


def test_exports():
    assert {"sparse_spgemm", "SparseSpGEMM"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_spgemm) and issubclass(tsgu.SparseSpGEMM, torch.autograd.Function)
    from torchsparsegradutils_amd.sparse_spgemm import __all__ as mod_all

    assert mod_all == ["sparse_spgemm", "SparseSpGEMM"]


# ---- the restatement against torch's own op ----------------------------------------------------------------------------------------
def test_the_restatement_agrees_with_torch_sparse_mm_and_its_autograd():
    a, A, b, B, G, ref = sr.case("random_small")
    At = sr.to_torch(a, A, "coo", torch.float64).requires_grad_(True)
    Bt = sr.to_torch(b, B, "coo", torch.float64).requires_grad_(True)
    C = torch.sparse.mm(At, Bt)
    sr.assert_on_pattern(C.coalesce(), ref["crow"], ref["col"], ref["C"], ref["C_terms"], "float64", "torch C")
    rows = np.repeat(np.arange(a.shape[0]), np.diff(ref["crow"]))
    Gs = torch.sparse_coo_tensor(torch.from_numpy(np.stack((rows, ref["col"]))), torch.tensor(G[rows, ref["col"]]), C.shape)
    gA, gB = torch.autograd.grad(C, (At, Bt), Gs)
    # both gradients on the operands' own patterns, nothing outside, nothing dropped
    sr.assert_on_pattern(gA.coalesce(), *sr.csr_of(a), ref["gA"], ref["gA_terms"], "float64", "torch gradA")
    sr.assert_on_pattern(gB.coalesce(), *sr.csr_of(b), ref["gB"], ref["gB_terms"], "float64", "torch gradB")


def test_a_cancelling_entry_stays_stored_in_torch_and_in_the_restatement():
    a, b = np.ones((1, 2), dtype=bool), np.ones((2, 1), dtype=bool)
    A, B = np.array([[1.0, 1.0]]), np.array([[1.0], [-1.0]])
    S, crow, col = sr.pattern(a, b)
    assert S.tolist() == [[True]] and crow.tolist() == [0, 1] and col.tolist() == [0]
    C = torch.sparse.mm(sr.to_torch(a, A, "coo", torch.float64), sr.to_torch(b, B, "coo", torch.float64)).coalesce()
    assert C._nnz() == 1 and C._indices().tolist() == [[0], [0]] and C._values().tolist() == [0.0]
    for layout in ("coo", "csr"):
        ours = sparse_spgemm(sr.to_torch(a, A, layout, torch.float32), sr.to_torch(b, B, layout, torch.float32))
        sr.assert_on_pattern(ours, crow, col, np.zeros((1, 1)), np.full((1, 1), 2.0), "float32", "cancellation")


def test_the_cases_of_the_gpu_tests_are_what_they_claim():
    limits = _backend.SPGEMM_BIN_LIMITS
    a, _, b, _, _, ref = sr.case("random_small")
    lens = np.diff(ref["crow"])
    assert a.shape == (37, 29) and b.shape == (29, 41) and 0.1 < a.mean() < 0.2 and 0.1 < b.mean() < 0.2
    assert not a[3].any() and not a[20].any() and lens[3] == lens[20] == 0            # empty rows of A
    assert a[5].any() and a[11].any() and lens[5] == lens[11] == 0                    # rows that meet only empty rows of B
    assert lens[9] == 1 and lens.max() > 8
    a, _, b, _, _, ref = sr.case("all_empty")
    assert a.any() and b.any() and ref["crow"][-1] == 0
    for L in limits:
        for name in ("bound_one_long_row", "bound_overlapping_rows"):
            a, _, b, _, _, ref = sr.case(name, L)
            ub = a.astype(np.int64) @ b.sum(1)
            assert ub.tolist() == [L - 1, L, L + 1], (name, L)
            if name == "bound_overlapping_rows":
                assert (np.diff(ref["crow"]) * 4 < ub).all()                              # upper bound ≫ distinct count
    _, _, _, _, _, ref = sr.case("long_row")
    assert np.diff(ref["crow"]).max() > limits[-1]
    a, _, _, _, _, ref = sr.case("stencil27")
    assert a.shape == (512, 512) and (a.sum(1) == 27).all() and (np.diff(ref["crow"]) == 125).all()


# ---- the CPU path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("layouts", [("coo", "coo"), ("csr", "csr"), ("coo", "csr"), ("csr", "coo")])
@pytest.mark.parametrize("index_dtype", [torch.int32, torch.int64])
def test_cpu_operands(layouts, index_dtype, dtype):
    if "coo" in layouts and index_dtype == torch.int32 and layouts != ("coo", "coo"):
        # (torch's COO indices are int64, whatever they are built from: a COO and an int32 CSR operand have two index dtypes)
        with pytest.raises(ValueError, match="same index dtype"):
            a, A, b, B, _, _ = sr.case("random_small")
            sparse_spgemm(sr.to_torch(a, A, layouts[0], DTYPES[dtype], index_dtype), sr.to_torch(b, B, layouts[1], DTYPES[dtype], index_dtype))
        return
    a, A, b, B, G, ref = sr.case("random_small")
    At = sr.to_torch(a, A, layouts[0], DTYPES[dtype], index_dtype).requires_grad_(True)
    Bt = sr.to_torch(b, B, layouts[1], DTYPES[dtype], index_dtype).requires_grad_(True)
    C = sparse_spgemm(At, Bt)
    assert C.layout == At.layout and C.dtype == At.dtype and C.shape == (37, 41)
    if C.layout == torch.sparse_csr:
        assert C.crow_indices().dtype == C.col_indices().dtype == index_dtype
    else:
        assert C.is_coalesced()
    sr.assert_on_pattern(C, ref["crow"], ref["col"], ref["C"], ref["C_terms"], dtype, "C")
    gA, gB = torch.autograd.grad(C, (At, Bt), torch.tensor(G).to(DTYPES[dtype]))
    assert gA.layout == At.layout and gB.layout == Bt.layout and gA.dtype == gB.dtype == DTYPES[dtype]
    if gA.layout == torch.sparse_csr:
        assert gA.crow_indices().data_ptr() == At.crow_indices().data_ptr() and gA.col_indices().data_ptr() == At.col_indices().data_ptr()
    else:
        assert gA._indices().data_ptr() == At._indices().data_ptr()
    sr.assert_on_pattern(gA, *sr.csr_of(a), ref["gA"], ref["gA_terms"], dtype, "gradA")
    sr.assert_on_pattern(gB, *sr.csr_of(b), ref["gB"], ref["gB_terms"], dtype, "gradB")


def test_cpu_uncoalesced_coo_is_coalesced_first():
    idx = torch.tensor([[0, 0, 1, 0], [1, 1, 0, 0]])
    A = torch.sparse_coo_tensor(idx, torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), (2, 2)).requires_grad_(True)
    B = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.tensor([5.0, 7.0], dtype=torch.float64), (2, 2), is_coalesced=True)
    C = sparse_spgemm(A, B)
    assert torch.equal(C.to_dense(), A.detach().to_dense() @ B.to_dense())
    (gA,) = torch.autograd.grad(C, A, torch.ones(2, 2, dtype=torch.float64))
    # duplicates are ONE matrix entry: the gradient is that of the coalesced matrix, handed on by torch's coalesce
    assert torch.equal(gA.to_dense(), torch.tensor([[5.0, 7.0], [5.0, 0.0]], dtype=torch.float64))


def test_cpu_needs_input_grad():
    a, A, b, B, G, _ = sr.case("random_small")
    for which in (0, 1):
        ops = [sr.to_torch(a, A, "csr", torch.float64), sr.to_torch(b, B, "csr", torch.float64)]
        ops[which].requires_grad_(True)
        C = sparse_spgemm(*ops)
        C.backward(torch.tensor(G))
        assert ops[which].grad is not None and ops[1 - which].grad is None


def test_cpu_gradient_forms():
    """The upstream gradient on C's own index tensors, dense, and sparse on another pattern (masked) give the same gradients."""
    a, A, b, B, G, ref = sr.case("random_small")
    At = sr.to_torch(a, A, "csr", torch.float64).requires_grad_(True)
    Bt = sr.to_torch(b, B, "csr", torch.float64).requires_grad_(True)
    C = sparse_spgemm(At, Bt)
    Gd = torch.tensor(G)
    rows = np.repeat(np.arange(37), np.diff(ref["crow"]))
    own = torch.sparse_csr_tensor(C.crow_indices(), C.col_indices(), torch.tensor(G[rows, ref["col"]]), C.shape)
    other_mask = np.random.default_rng(3).random(G.shape) < 0.5
    other = torch.from_numpy(np.where(other_mask, G, 0.0)).to_sparse()
    want = torch.autograd.grad(C, (At, Bt), Gd, retain_graph=True)
    got = torch.autograd.grad(C, (At, Bt), own, retain_graph=True)
    assert torch.equal(want[0].values(), got[0].values()) and torch.equal(want[1].values(), got[1].values())
    gA, gB = torch.autograd.grad(C, (At, Bt), other)
    rA, _, rB, _ = sr.gradients(A, a, B, b, np.where(other_mask, G, 0.0))
    assert np.allclose(gA.to_dense().numpy(), np.where(a, rA, 0.0), rtol=0, atol=1e-12)
    assert np.allclose(gB.to_dense().numpy(), np.where(b, rB, 0.0), rtol=0, atol=1e-12)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _pair(dtype=torch.float32, layout="csr", index_dtype=torch.int64):
    a, A, b, B, _, _ = sr.case("random_small")
    return sr.to_torch(a, A, layout, dtype, index_dtype), sr.to_torch(b, B, layout, dtype, index_dtype)


def test_refusals():
    A, B = _pair()
    with pytest.raises(TypeError, match="Both A and B should be instances of torch.Tensor"):
        sparse_spgemm(A, [[1.0]])
    with pytest.raises(TypeError, match="Both A and B should be instances of torch.Tensor"):
        sparse_spgemm(None, B)
    with pytest.raises(ValueError, match="A should be in either COO or CSR sparse format"):
        sparse_spgemm(A.to_dense(), B)
    with pytest.raises(ValueError, match="B should be in either COO or CSR sparse format"):
        sparse_spgemm(A, B.to_dense())
    with pytest.raises(ValueError, match="A should be in either COO or CSR sparse format"):
        sparse_spgemm(A.to_sparse_csc(), B)
    with pytest.raises(ValueError, match="B should be in either COO or CSR sparse format"):
        sparse_spgemm(A, B.to_sparse_csc())
    A3 = torch.sparse_coo_tensor(torch.tensor([[0], [0], [0]]), torch.tensor([1.0]), (2, 37, 29))
    B3 = torch.sparse_coo_tensor(torch.tensor([[0], [0], [0]]), torch.tensor([1.0]), (2, 29, 41))
    with pytest.raises(ValueError, match="batched operands are not supported"):
        sparse_spgemm(A3, B3)
    with pytest.raises(ValueError, match="batched operands are not supported"):
        sparse_spgemm(A, B3)
    with pytest.raises(ValueError, match=r"Incompatible inner dimensions: A\[\.\.\., 29\] vs B\[37, \.\.\.\]"):
        sparse_spgemm(A, A)
    with pytest.raises(ValueError, match="expected A and B to have the same dtype, got torch.float32 and torch.float64"):
        sparse_spgemm(A, B.to(torch.float64))
    with pytest.raises(ValueError, match="values must be float32, float64 or bfloat16, got torch.float16"):
        sparse_spgemm(A.to(torch.float16), B.to(torch.float16))
    A32, _ = _pair(index_dtype=torch.int32)
    with pytest.raises(ValueError, match="expected A and B to have the same index dtype, got torch.int32 and torch.int64"):
        sparse_spgemm(A32, B)
    with pytest.raises(ValueError, match="A and B must be on the same device"):
        sparse_spgemm(A, B.to("meta"))


def test_a_row_of_b_with_a_repeated_column_is_refused():
    A, _ = _pair()
    crow = torch.zeros(30, dtype=torch.int64)
    crow[5:] = 3
    for cols in ([2, 7, 2], [4, 4, 9]):           # apart and adjacent
        B = torch.sparse_csr_tensor(crow, torch.tensor(cols), torch.ones(3), (29, 41))
        with pytest.raises(ValueError, match="a row of B holds a column index more than once"):
            sparse_spgemm(A, B)
    # the same column in two ROWS is what a product is made of
    crow2 = torch.zeros(30, dtype=torch.int64)
    crow2[5:] = 1
    crow2[6:] = 2
    sparse_spgemm(A, torch.sparse_csr_tensor(crow2, torch.tensor([4, 4]), torch.ones(2), (29, 41)))


# ---- the fifth header ---------------------------------------------------------------------------------------------------------------
def test_the_bin_limits_are_the_librarys():
    limits, lanes = _backend.spgemm_bins()
    assert limits == _backend.SPGEMM_BIN_LIMITS and lanes == _backend.SPGEMM_BIN_LANES
    assert list(limits) == sorted(set(limits)) and all(256 % g == 0 for g in lanes)
    # every LDS bin's sort buffer is a power of two that its lanes divide; the global bin's smallest is the next one
    assert all(L & (L - 1) == 0 and L % g == 0 for L, g in zip(limits, lanes))
    assert _backend.SPGEMM_SCRATCH_MIN == 2 * limits[-1]
    # columns + float64 accumulators of the largest LDS bin, and the staging pass, stay inside a 64 KiB static allocation
    assert limits[-1] * 12 + 256 * 20 <= 64 * 1024


FAKE = 0x7F0000001000          # an aligned address that is never dereferenced: every call below is refused, or has no work, on the host


def _addr(k):
    return FAKE + k * 0x100000


def _symbolic(lib, **kw):
    a = dict(itype=0, bin=0, n_bin=3, rows=_addr(0), n_rows=40, n_inner=30, n_cols=50, a_ptr=_addr(1), a_idx=_addr(2), b_ptr=_addr(3),
             b_idx=_addr(4), scratch=None, sptr=None, fill=0, cnt=_addr(5), c_ptr=None, c_idx=None, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_spgemm_symbolic(*a.values())


def _numeric(lib, **kw):
    a = dict(vtype=0, itype=0, bin=0, n_bin=3, rows=_addr(0), n_rows=40, n_inner=30, n_cols=50, a_ptr=_addr(1), a_idx=_addr(2),
             a_val=_addr(3), b_ptr=_addr(4), b_idx=_addr(5), b_val=_addr(6), c_ptr=_addr(7), c_idx=_addr(8), acc=None, c_val=_addr(9),
             device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_spgemm_numeric(*a.values())


def test_host_side_refusals_of_the_entry_points():
    """Refused before a device is touched (device = -1 is itself the last refusal: BAD_ARG)."""
    lib = _backend.load_library()
    assert _symbolic(lib) == BAD_ARG                                   # complete arguments reach the device check
    assert _symbolic(lib, itype=2) == BAD_DTYPE
    assert _symbolic(lib, bin=4) == BAD_ARG and _symbolic(lib, bin=-1) == BAD_ARG
    assert _symbolic(lib, n_bin=41) == BAD_ARG and _symbolic(lib, fill=2) == BAD_ARG
    assert _symbolic(lib, n_cols=2 ** 31 - 1) == TOO_LARGE and _symbolic(lib, n_rows=2 ** 31) == TOO_LARGE
    assert _symbolic(lib, n_bin=0, rows=None, cnt=None) == OK           # no rows: no work
    assert _symbolic(lib, rows=None) == BAD_ARG and _symbolic(lib, cnt=None) == BAD_ARG
    assert _symbolic(lib, fill=1) == BAD_ARG                            # writing needs c_ptr and c_idx
    assert _symbolic(lib, bin=3) == BAD_ARG                             # the global bin needs its scratch
    assert _numeric(lib) == BAD_ARG
    assert _numeric(lib, vtype=3) == BAD_DTYPE and _numeric(lib, itype=-1) == BAD_DTYPE
    assert _numeric(lib, bin=3) == BAD_ARG                              # the global bin needs its accumulators
    assert _numeric(lib, n_bin=0, rows=None) == OK
    assert _numeric(lib, c_val=None) == BAD_ARG and _numeric(lib, n_cols=2 ** 31 - 1) == TOO_LARGE
    assert lib.tsgu_spgemm_row_bound(0, 0, 5, None, None, None, None, -1, None) == OK
    assert lib.tsgu_spgemm_row_bound(0, 4, 5, _addr(0), _addr(1), _addr(2), None, -1, None) == BAD_ARG
    assert lib.tsgu_spgemm_grad_a(0, 0, 4, 5, 6, 0, None, None, None, None, None, None, None, None, None, -1, None) == OK
    assert lib.tsgu_spgemm_grad_a(3, 0, 4, 5, 6, 1, None, None, None, None, None, None, None, None, None, -1, None) == BAD_DTYPE
    assert lib.tsgu_spgemm_grad_a(0, 0, 4, 5, 6, 1, None, None, None, None, None, None, None, None, None, -1, None) == BAD_ARG
    assert lib.tsgu_spgemm_grad_b(0, 0, 4, 5, 6, 0, None, None, None, None, None, None, None, None, None, None, -1, None) == OK
    assert lib.tsgu_spgemm_grad_b(0, 0, 4, 5, 6, -1, None, None, None, None, None, None, None, None, None, None, -1, None) == BAD_ARG
