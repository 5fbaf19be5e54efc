"""sparse_spgemm on the GPU against the float64 restatement of tests/_spgemm_ref.py (pinned to torch.sparse.mm(A, B) and its
autograd on the CPU by tests/test_sparse_spgemm_cpu.py).

Pattern: crow and col exactly the sorted structural product.  Values and both gradients: every entry within 8·ε·Σ|its terms| of
the float64 reference (ε = 2^-24 for float32 and bfloat16, whose sums run in float32, 2^-53 for float64) — the project's
elementwise bound; bfloat16 is the float32-accumulated sum rounded once, so one bf16 ulp (2^-8 relative) of the exact value on
top.  The operands are bfloat16-exact random values: one float64 reference serves the three value types, the products are exact
in float32 and the sums still round.

The shapes are the smallest that reach each path (tests/_spgemm_ref.py; what they claim is asserted without a GPU): random small
with empty rows, rows that meet only empty rows, a single-entry row; an all-empty product; for every bin limit L of the kernels
three rows whose upper bound Σ_k nnz(B[k,:]) is L-1, L, L+1, once from one long row of B and once from eight heavily overlapping
ones; a row with more distinct columns than the largest LDS bin holds (global scratch); the 27-point stencil on 8³ squared.  The
kernels sort a row's candidate columns instead of hashing them; the clustered-column case of a hash table (multiples of a
capacity plus capacity-1 consecutive columns) is kept as one more pattern.
"""

import warnings

import numpy as np
import pytest
import torch

import _spgemm_ref as sr
from torchsparsegradutils_amd import _backend

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}
LIMITS = _backend.SPGEMM_BIN_LIMITS
FORMS = [("csr", "csr", torch.int32), ("csr", "csr", torch.int64), ("coo", "coo", torch.int64), ("csr", "coo", torch.int64),
         ("coo", "csr", torch.int64)]
BOUND_CASES = [(name, L) for L in LIMITS for name in ("bound_one_long_row", "bound_overlapping_rows")]
OTHER_CASES = [("all_empty", None), ("long_row", None), ("clustered", None), ("stencil27", None)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    _backend.load_library()
    yield


def _operands(name, limit, dtype, form, grad=(True, True)):
    a, A, b, B, G, ref = sr.case(name, limit)
    la, lb, idt = form
    At = sr.to_torch(a, A, la, DTYPES[dtype], idt, DEV).requires_grad_(grad[0])
    Bt = sr.to_torch(b, B, lb, DTYPES[dtype], idt, DEV).requires_grad_(grad[1])
    return (a, A, b, B, G, ref), At, Bt


def _index_tensors(T):
    return (T.crow_indices(), T.col_indices()) if T.layout == torch.sparse_csr else (T._indices(),)


def _check_case(name, limit, dtype, form):
    import torchsparsegradutils_amd as t

    (a, A, b, B, G, ref), At, Bt = _operands(name, limit, dtype, form)
    C = t.sparse_spgemm(At, Bt)
    assert C.layout == At.layout and C.dtype == At.dtype and tuple(C.shape) == (a.shape[0], b.shape[1]) and C.is_cuda
    assert all(i.dtype == form[2] for i in _index_tensors(C))
    if C.layout == torch.sparse_coo:
        assert C.is_coalesced()
    crow, col, _ = sr.arrays_of(C)
    rows = np.repeat(np.arange(a.shape[0]), np.diff(crow))
    assert crow[0] == 0 and np.all(np.diff(crow) >= 0) and crow[-1] == len(col)
    assert np.all((np.diff(col) > 0) | (np.diff(rows) > 0)), "columns must be strictly ascending within every row"
    what = f"{name}{'' if limit is None else limit} {form[0]}·{form[1]} {form[2]}"
    sr.assert_on_pattern(C, ref["crow"], ref["col"], ref["C"], ref["C_terms"], dtype, what + " C")
    gA, gB = torch.autograd.grad(C, (At, Bt), torch.tensor(G).to(DTYPES[dtype]).to(DEV))
    assert gA.layout == At.layout and gB.layout == Bt.layout and gA.dtype == gB.dtype == DTYPES[dtype]
    for g, X in ((gA, At), (gB, Bt)):      # on the operands' own index tensors
        assert all(i.data_ptr() == j.data_ptr() for i, j in zip(_index_tensors(g), _index_tensors(X)))
    sr.assert_on_pattern(gA, *sr.csr_of(a), ref["gA"], ref["gA_terms"], dtype, what + " gradA")
    sr.assert_on_pattern(gB, *sr.csr_of(b), ref["gB"], ref["gB_terms"], dtype, what + " gradB")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{f[1]}-{str(f[2]).split('.')[-1]}")
def test_random_small(form, dtype):
    _check_case("random_small", None, dtype, form)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", BOUND_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_rows_at_the_bin_limits(case, dtype):
    k = BOUND_CASES.index(case)
    _check_case(case[0], case[1], dtype, FORMS[k % len(FORMS)])


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: c[0])
def test_other_shapes(case, dtype):
    """An all-empty product, the global-scratch bin, clustered columns, the stencil squared — each in two forms."""
    k = OTHER_CASES.index(case)
    _check_case(case[0], case[1], dtype, FORMS[k % 2])
    _check_case(case[0], case[1], dtype, FORMS[2 + k % 3])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_operands_without_entries(dtype):
    import torchsparsegradutils_amd as t

    dt = DTYPES[dtype]
    for n_a, n_b in ((0, 5), (5, 0), (0, 0)):
        A = torch.sparse_csr_tensor(torch.tensor([0, n_a, n_a, n_a], dtype=torch.int32), torch.arange(n_a, dtype=torch.int32),
                                    torch.ones(n_a, dtype=dt), (3, 6)).to(DEV).requires_grad_(True)
        B = torch.sparse_csr_tensor(torch.tensor([0, 0, n_b, n_b, n_b, n_b, n_b], dtype=torch.int32), torch.arange(n_b, dtype=torch.int32),
                                    torch.ones(n_b, dtype=dt), (6, 7)).to(DEV).requires_grad_(True)
        C = t.sparse_spgemm(A, B)
        assert C.values().numel() == 0 and C.crow_indices().tolist() == [0, 0, 0, 0]
        gA, gB = torch.autograd.grad(C, (A, B), torch.ones(3, 7, dtype=dt, device=DEV))
        assert gA.values().numel() == n_a and gB.values().numel() == n_b
        assert not gA.values().any() and not gB.values().any()
    A = torch.sparse_csr_tensor(torch.tensor([0, 2, 2, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32),
                                torch.ones(2, dtype=dt), (3, 6)).to(DEV).requires_grad_(True)
    C = t.sparse_spgemm(A, B.detach())                               # (entries in A, none in B)
    assert C.values().numel() == 0


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("layout", ["csr", "coo"])
def test_cancellation_keeps_its_stored_zero(layout, dtype):
    import torchsparsegradutils_amd as t

    a, b = np.ones((1, 2), dtype=bool), np.ones((2, 1), dtype=bool)
    A, B = np.array([[1.0, 1.0]]), np.array([[1.0], [-1.0]])
    C = t.sparse_spgemm(sr.to_torch(a, A, layout, DTYPES[dtype], torch.int64, DEV), sr.to_torch(b, B, layout, DTYPES[dtype], torch.int64, DEV))
    crow, col, val = sr.arrays_of(C)
    assert crow.tolist() == [0, 1] and col.tolist() == [0] and val.tolist() == [0.0]


def test_the_pattern_is_cached_and_the_result_carries_the_same_index_tensors():
    import torchsparsegradutils_amd as t
    from torchsparsegradutils_amd import _pattern
    from torchsparsegradutils_amd.sparse_logsumexp import _Operand

    for form in (FORMS[0], FORMS[2]):
        (a, A, b, B, G, ref), At, Bt = _operands("stencil27", None, "float32", form)
        C1 = t.sparse_spgemm(At, Bt)
        first = [i.data_ptr() for i in _index_tensors(C1)]
        # new values on the same index tensors
        make = torch.sparse_csr_tensor if form[0] == "csr" else (lambda *args: torch.sparse_coo_tensor(*args, is_coalesced=True))
        A2 = make(*_index_tensors(At), torch.randn(At._nnz(), device=DEV), At.shape).requires_grad_(True)
        B2 = make(*_index_tensors(Bt), torch.randn(Bt._nnz(), device=DEV), Bt.shape).requires_grad_(True)
        C2 = t.sparse_spgemm(A2, B2)
        assert [i.data_ptr() for i in _index_tensors(C2)] == first
        want = A2.detach().to_dense().double() @ B2.detach().to_dense().double()
        assert float((C2.detach().to_dense().double() - want).abs().max()) < 1e-4          # (27 terms of order one: pattern reuse, not rounding)
        # a following sparse_mm(C, X) works on C's pattern core, the one the backward's restriction finds again
        core = _Operand(C1.detach()).plan.core
        X = torch.randn(512, 8, device=DEV)
        Y = t.sparse_mm(C2, X)
        assert _Operand(C2.detach()).plan.core is core
        assert float((Y.detach().double() - want @ X.double()).abs().max()) < 1e-3
        Y.square().sum().backward()
        assert A2.grad is not None and B2.grad is not None and A2.grad._nnz() == At._nnz()
        # the plan dies with either operand's pattern
        acore = _Operand(At.detach()).plan.core
        assert len(acore.own["spgemm"]) == 1
    del At, Bt, A2, B2, C1, C2, Y
    _pattern.clear_cache()


def test_gradient_forms_agree_with_the_reference():
    """The upstream gradient on C's own index tensors, dense, and sparse on another pattern (masked by C's)."""
    import torchsparsegradutils_amd as t

    for form in (FORMS[0], FORMS[2]):
        (a, A, b, B, G, ref), At, Bt = _operands("random_small", None, "float64", form)
        C = t.sparse_spgemm(At, Bt)
        rows = np.repeat(np.arange(a.shape[0]), np.diff(ref["crow"]))
        gvals = torch.tensor(G[rows, ref["col"]]).to(DEV)
        own = torch.sparse_csr_tensor(C.crow_indices(), C.col_indices(), gvals, C.shape) if form[0] == "csr" else \
            torch.sparse_coo_tensor(C._indices(), gvals, C.shape, is_coalesced=True)
        for Gt in (own, torch.tensor(G).to(DEV)):
            gA, gB = torch.autograd.grad(C, (At, Bt), Gt, retain_graph=True)
            sr.assert_on_pattern(gA, *sr.csr_of(a), ref["gA"], ref["gA_terms"], "float64", "gradA")
            sr.assert_on_pattern(gB, *sr.csr_of(b), ref["gB"], ref["gB_terms"], "float64", "gradB")
        other_mask = np.random.default_rng(3).random(G.shape) < 0.5
        Go = np.where(other_mask, G, 0.0)
        other = torch.tensor(Go).to_sparse().to(DEV)
        if form[0] == "csr":
            other = other.to_sparse_csr()
        gA, gB = torch.autograd.grad(C, (At, Bt), other)
        rA, tA, rB, tB = sr.gradients(A, a, B, b, Go)
        sr.assert_on_pattern(gA, *sr.csr_of(a), rA, tA, "float64", "gradA (other pattern)")
        sr.assert_on_pattern(gB, *sr.csr_of(b), rB, tB, "float64", "gradB (other pattern)")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_two_runs_give_the_same_bits(dtype):
    import torchsparsegradutils_amd as t
    from torchsparsegradutils_amd import _pattern

    gen = torch.Generator().manual_seed(11)
    for name in ("random_small", "stencil27", "long_row"):
        a, _, b, _, _, ref = sr.case(name)
        A = torch.randn(a.shape, generator=gen, dtype=torch.float64).numpy()       # values that round in every product and sum
        B = torch.randn(b.shape, generator=gen, dtype=torch.float64).numpy()
        G = torch.randn(a.shape[0], b.shape[1], generator=gen, dtype=torch.float64).to(DTYPES[dtype]).to(DEV)
        runs = []
        for _ in range(2):
            _pattern.clear_cache()                                                 # the symbolic phase twice as well
            At = sr.to_torch(a, A, "csr", DTYPES[dtype], torch.int32, DEV).requires_grad_(True)
            Bt = sr.to_torch(b, B, "csr", DTYPES[dtype], torch.int32, DEV).requires_grad_(True)
            C = t.sparse_spgemm(At, Bt)
            gA, gB = torch.autograd.grad(C, (At, Bt), G)
            runs.append((C.crow_indices().clone(), C.col_indices().clone(), C.values().detach().clone(), gA.values().clone(), gB.values().clone()))
        for x, y in zip(*runs):
            assert torch.equal(x, y), name


def _sync_warnings(step):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]


def test_the_steady_state_synchronises_no_more_than_sparse_mm():
    import torchsparsegradutils_amd as t

    (a, A, b, B, G, ref), At, Bt = _operands("stencil27", None, "float32", FORMS[0])
    X = torch.randn(512, 8, device=DEV, requires_grad=True)
    GX = torch.randn(512, 8, device=DEV)
    gvals = torch.randn(int(ref["crow"][-1]), device=DEV)

    def ours():
        C = t.sparse_spgemm(At, Bt)
        torch.autograd.grad(C, (At, Bt), torch.sparse_csr_tensor(C.crow_indices(), C.col_indices(), gvals, C.shape))

    def yardstick():
        torch.autograd.grad(t.sparse_mm(At, X), (At, X), GX)

    for _ in range(2):
        ours()
        yardstick()
        t.wait_for_plans()
    mine, theirs = _sync_warnings(ours), _sync_warnings(yardstick)
    print("synchronisations of the third step: sparse_spgemm", len(mine), mine, "sparse_mm", len(theirs), theirs)
    assert len(mine) <= len(theirs)


def test_a_gradient_is_computed_only_where_it_is_needed(monkeypatch):
    import torchsparsegradutils_amd as t

    calls = []
    real_a, real_b = _backend.spgemm_grad_a, _backend.spgemm_grad_b
    monkeypatch.setattr(_backend, "spgemm_grad_a", lambda *args: calls.append("a") or real_a(*args))
    monkeypatch.setattr(_backend, "spgemm_grad_b", lambda *args: calls.append("b") or real_b(*args))
    for grad, want in (((False, True), ["b"]), ((True, False), ["a"])):
        (a, A, b, B, G, ref), At, Bt = _operands("random_small", None, "float32", FORMS[0], grad=grad)
        C = t.sparse_spgemm(At, Bt)
        del calls[:]
        C.backward(torch.tensor(G).float().to(DEV))
        assert calls == want
        assert (At.grad is None) == (not grad[0]) and (Bt.grad is None) == (not grad[1])
