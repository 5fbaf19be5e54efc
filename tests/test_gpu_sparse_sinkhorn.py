"""sparse_sinkhorn on the GPU through the public API: the fused half-step, plan and reverse-sweep kernels against the float64
restatement (tests/_sinkhorn_ref.py), on the structural patterns of _lse_cases (rows on every branch of the range walk, columns
— through the cached transpose — as long groups that cross ranges), T = 3.

The reference.  A matrix of the main pattern has ~4·10³ rows and ~2.7·10⁵ columns, so the restatement runs in its entry-wise form
(`_sinkhorn_ref.entries`: the same float64 arithmetic on the stored entries only; tests/test_sparse_sinkhorn_cpu.py holds it
against the dense form, and the pipeline test below uses the dense form itself).

The potentials' bound, 2T·c·ε·M.  Both half-step maps are non-expansive in the sup norm (LSE is 1-Lipschitz), so the rounding
errors of the 2T half steps add and do not compound.  M is the largest |S_ij| + |u_i| + |v_j| + |log marginal| over the stored
entries, from the float64 reference; ε the accumulator's unit roundoff (2⁻²⁴ for float32 and bfloat16, 2⁻⁵³ for float64); c the
roundings (in units of ε) on one entry's way into its group's potential, counted from csrc/sinkhorn_impl.h and logsumexp_impl.h:
   1   val + other[idx]                        (the staging functor)
   1   st[i] − m                               (MaxSumExp, after the exact maximum)
   2   exp                                     (≤ 1 ulp = 2ε)
   8   the piece's sum (MaxSumExpK): a lane adds its terms with a compensated sum, 2ε + O(k·ε²) whatever their number k (≤ 48 on
       the lane path, ≤ R/64 = 32 on the wave path), then the wave path's 6-level butterfly
   4·(⌈P/64⌉ + 6)   the merge of a group of P > 1 range pieces: ⌈P/64⌉ lane-strided combines and a 6-level butterfly, each an exp
       (2), a product and a sum
   2   log                                     (≤ 1 ulp)
   2   m + log s,  log_marginal − lse
so c = 16 + 4·(⌈P/64⌉ + 6) with P the most pieces of any row or column of the case (16 where nothing crosses a range): 52 for
the main pattern (P = 132), 44 for the boundary patterns.  The sums are of positive terms, so a chain of k roundings moves a total
by at most kε relatively, that is kε absolutely in its logarithm, and M ≥ 1 in every case with entries.
log_P = S + u + v: three times the bound (two potentials and two more additions), plus one rounding to bfloat16 for bfloat16
values — half a unit in the last of its 8 significant bits, at most 2⁻⁸·|log_P| (2⁻⁹·|log_P| is half of what one rounding to
nearest can cost: a value just above 1 + 2⁻⁸ is 2⁻⁸ away from both neighbours).
Column marginals: sparse_logsumexp(log_P, 0, include_zeros=False) − log_b within the potentials' bound; for bfloat16 the
rounding of log_P (carried through the 1-Lipschitz LSE) and of sparse_logsumexp's own bfloat16 result are added.

Gradients have no closed bound: the yardstick is the restatement itself — in float32 against float64 on the same inputs (for the
float32 and bfloat16 runs), or in float64 with the entries shuffled, which is the same problem in another summation order (for
the float64 run).  The GPU may be off by 4 times the yardstick's error, with a floor of 64·ε·max|grad_ref|, per gradient tensor in
the max norm; the bfloat16 gradient of S is rounded once more (autograd hands a bfloat16 leaf a bfloat16 gradient), which adds
half a bfloat16 ulp of its value.  The measured figures are printed (EXPERIMENTS.md records them).

Measured on an MI355X (EXPERIMENTS.md §33): every check passes.  Potentials, log_P and column marginals are 76 – 1700 times
inside their bounds; the gradients are at 0.003 – 4.5 times their yardstick and at most 0.76 of their allowance (float64
nnz_kR_plus_1, dS: 3.6e-14 against 4.8e-14).  Two things the gradient of S needed to get there: the sweep reads −lse of the half
step it differentiates instead of the rounded potential (the weights of a group then sum to one: 2.2e-4 → 5.1e-5 on float32
nnz_kR_trailing), and the sums of a piece are compensated (float64 nnz_kR_plus_1: 5.5e-14 → 3.6e-14).
"""

import functools
import math

import numpy as np
import pytest
import torch

import _lse_cases
import _sinkhorn_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
TORCH = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}
ACC = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.float32}
EPS = {"float32": 2.0 ** -24, "float64": 2.0 ** -53, "bfloat16": 2.0 ** -24}      # unit roundoff of the accumulator
BITS = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}
T = 3
CASES = ("main_randn1", "main_randn3", "nnz_kR_plus_1_needles", "nnz_kR_trailing_needles", "nnz_zero_needles")
EXTRA_COLUMNS = 3      # columns without entries at the end of every matrix


def _tsgu():
    import torchsparsegradutils_amd as tsgu

    return tsgu


def _bits(t):
    return t.detach().contiguous().view(BITS[t.dtype]).cpu()


def _bf16_half_ulp(x):
    """Half a unit in the last place of bfloat16 (8 significant bits) at |x| (float64 tensor)."""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x)[1] - 9)


class Problem:
    """One case on the CPU: the pattern in row-major COO positions, inputs rounded to the run's types (held in float64), the float64
    reference with its gradients, the bound's ingredients, and the gradient yardsticks.  Built once and shared."""

    def __init__(self, dtype, ptr, vals64, seed):
        self.dtype = dtype
        ptr = np.asarray(ptr, dtype=np.int64)
        lens = np.diff(ptr)
        self.n, self.m = ptr.size - 1, int(lens.max(initial=0)) + EXTRA_COLUMNS
        self.ptr = torch.from_numpy(ptr)
        self.cols = torch.from_numpy(_lse_cases.columns(ptr))
        self.rows = torch.repeat_interleave(torch.arange(self.n), torch.from_numpy(lens))
        self.nnz = int(ptr[-1])
        g = torch.Generator().manual_seed(seed)
        self.vals = torch.from_numpy(np.ascontiguousarray(vals64)).to(TORCH[dtype])           # as the GPU gets them
        self.la = torch.randn(self.n, generator=g, dtype=F64).to(ACC[dtype])
        self.lb = torch.randn(self.m, generator=g, dtype=F64).to(ACC[dtype])
        self.cot = tuple(torch.randn(k, generator=g, dtype=F64).to(t) for k, t in
                         ((self.nnz, TORCH[dtype]), (self.n, ACC[dtype]), (self.m, ACC[dtype])))
        args = (self.rows, self.cols, self.vals.to(F64), self.n, self.m, self.la.to(F64), self.lb.to(F64), T)
        self.out, self.grads = ref.with_grads(ref.entries, *args, self.cot)
        lp, u, v = self.out
        R = _lse_cases.range_len(dtype)
        col_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.cols.numpy(), minlength=self.m))])
        self.pieces = int(max(_lse_cases.pieces(ptr, R).max(initial=1), _lse_cases.pieces(col_ptr, R).max(initial=1)))
        self.c = 16 + (4 * (math.ceil(self.pieces / 64) + 6) if self.pieces > 1 else 0)
        if self.nnz:
            marg = torch.maximum(self.la.to(F64).abs()[self.rows], self.lb.to(F64).abs()[self.cols])
            self.M = float((self.vals.to(F64).abs() + u[self.rows].abs() + v[self.cols].abs() + marg).max())
        else:
            self.M = 0.0
        self.bound = 2 * T * self.c * EPS[dtype] * self.M
        # the yardstick of the gradients: never the code under test
        if dtype == "float64":
            p = torch.randperm(self.nnz, generator=g)
            rp, cp = torch.randperm(self.n, generator=g), torch.randperm(self.m, generator=g)
            _, (dS, dla, dlb) = ref.with_grads(ref.entries, rp[self.rows][p], cp[self.cols][p], self.vals[p], self.n, self.m,
                                               torch.empty_like(self.la).index_copy_(0, rp, self.la),
                                               torch.empty_like(self.lb).index_copy_(0, cp, self.lb), T,
                                               (self.cot[0][p], torch.empty_like(self.cot[1]).index_copy_(0, rp, self.cot[1]),
                                                torch.empty_like(self.cot[2]).index_copy_(0, cp, self.cot[2])))
            other = (torch.empty_like(dS).index_copy_(0, p, dS), dla[rp], dlb[cp])
        else:
            _, other = ref.with_grads(ref.entries, self.rows, self.cols, self.vals.float(), self.n, self.m, self.la.float(), self.lb.float(),
                                      T, self.cot)
        self.yard = [float((o.to(F64) - w).abs().max()) if w.numel() else 0.0 for o, w in zip(other, self.grads)]

    def sparse(self, layout, itype, requires_grad=False):
        """(S on the GPU, its value leaf, the permutation from row-major order into its stored order or None)."""
        it = lambda t: t.to(itype).to(DEV)  # noqa: E731
        if layout == "csc":
            order = torch.argsort(self.cols * self.n + self.rows)
            leaf = self.vals[order].to(DEV).requires_grad_(requires_grad)
            ccol = torch._convert_indices_from_coo_to_csr(self.cols[order].contiguous(), self.m, out_int32=False)
            return torch.sparse_csc_tensor(it(ccol), it(self.rows[order]), leaf, (self.n, self.m)), leaf, order
        leaf = self.vals.to(DEV).requires_grad_(requires_grad)
        return torch.sparse_csr_tensor(it(self.ptr), it(self.cols), leaf, (self.n, self.m)), leaf, None


@functools.lru_cache(maxsize=None)
def _problem(dtype, name):
    for i, (nm, ptr, vals) in enumerate(_lse_cases.structural_cases(dtype)):
        if nm == name:
            return Problem(dtype, ptr, vals, 100 + i)
    raise KeyError(name)


def _values(X):
    return X._values() if X.layout == torch.sparse_coo else X.values()


def _rebuild(like, values):
    if like.layout == torch.sparse_csr:
        return torch.sparse_csr_tensor(like.crow_indices(), like.col_indices(), values, like.shape)
    if like.layout == torch.sparse_csc:
        return torch.sparse_csc_tensor(like.ccol_indices(), like.row_indices(), values, like.shape)
    return torch.sparse_coo_tensor(like._indices(), values, like.shape, is_coalesced=True)


def _check_potential(got, want, bound, what):
    got = got.detach().cpu().to(F64)
    inf = want.isinf()
    assert torch.equal(got.isinf(), inf) and torch.equal(got[inf], want[inf]), (what, "infinities")
    assert not got.isnan().any(), (what, "NaN")
    err = float((got[~inf] - want[~inf]).abs().max()) if (~inf).any() else 0.0
    print(f"    {what}: error {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (what, err, bound)


def _check_case(P, layout, itype):
    tsgu = _tsgu()
    dtype = P.dtype
    S, leaf, order = P.sparse(layout, itype, requires_grad=True)
    la = P.la.to(DEV).requires_grad_(True)
    lb = P.lb.to(DEV).requires_grad_(True)
    lp, u, v = tsgu.sparse_sinkhorn(S, la, lb, T)
    pick = (lambda t: t) if order is None else (lambda t: t[order])
    print(f"\n  {dtype} {layout} {itype}: n {P.n} m {P.m} nnz {P.nnz} pieces {P.pieces} c {P.c} M {P.M:.2f}")
    assert lp.layout == S.layout and lp.shape == S.shape and lp.dtype == TORCH[dtype] and u.dtype == v.dtype == ACC[dtype]
    lp_r, u_r, v_r = P.out
    _check_potential(u, u_r, P.bound, "u")
    _check_potential(v, v_r, P.bound, "v")
    assert bool(v_r[-EXTRA_COLUMNS:].isinf().all()), "the columns without entries"
    if P.nnz:
        want = pick(lp_r)
        err = (_values(lp).detach().cpu().to(F64) - want).abs()
        tol = 3 * P.bound + (_bf16_half_ulp(want) if dtype == "bfloat16" else 0)
        print(f"    log_P: error {float(err.max()):.3e}  bound {3 * P.bound:.3e}")
        assert bool((err <= tol).all()), ("log_P", float((err - tol).max()))
        # column marginals (of the columns with entries)
        lse = tsgu.sparse_logsumexp(lp.detach(), 0, include_zeros=False).cpu().to(F64)
        some = v_r.isfinite()
        merr = (lse - P.lb.to(F64))[some].abs()
        if dtype == "bfloat16":      # the rounding of the column's own entries and of the bfloat16 result
            top = torch.zeros(P.m, dtype=F64).scatter_reduce(0, P.cols, lp_r.abs(), "amax", include_self=True)
            mtol = P.bound + (2.0 ** -8) * (top + P.lb.to(F64).abs())[some]
        else:
            mtol = P.bound
        print(f"    column marginals: error {float(merr.max()):.3e}  bound {P.bound:.3e}")
        assert bool((merr <= mtol).all()), ("column marginals", float(merr.max()))
    cot = (_rebuild(lp, pick(P.cot[0]).to(DEV)), P.cot[1].to(DEV), P.cot[2].to(DEV))
    dS, dla, dlb = torch.autograd.grad((lp, u, v), (S, la, lb), cot)
    assert dS.layout == S.layout and dS.dtype == TORCH[dtype] and dla.dtype == dlb.dtype == ACC[dtype]
    for what, got, want, yard in zip(("dS", "dlog_a", "dlog_b"), (_values(dS), dla, dlb), (pick(P.grads[0]), P.grads[1], P.grads[2]), P.yard):
        if not want.numel():
            assert got.numel() == 0
            continue
        got = got.detach().cpu().to(F64)
        assert bool(got.isfinite().all()), (what, "not finite")
        err = (got - want).abs()
        allowed = max(4 * yard, 64 * EPS[dtype] * float(want.abs().max()))
        print(f"    {what}: error {float(err.max()):.3e}  yardstick {yard:.3e}  allowed {allowed:.3e}  max|grad| {float(want.abs().max()):.3e}")
        tol = allowed + (_bf16_half_ulp(want) if dtype == "bfloat16" and what == "dS" else 0)
        assert bool((err <= tol).all()), (what, float(err.max()), allowed)
    return (lp, u, v), (dS, dla, dlb)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("dtype", list(_lse_cases.DTYPES))
def test_structural_cases_csr(dtype, name):
    _check_case(_problem(dtype, name), "csr", torch.int32)


@pytest.mark.parametrize("layout,itype", [("csc", torch.int32), ("csr", torch.int64)], ids=["csc", "int64"])
def test_main_case_in_csc_and_with_int64_indices(layout, itype):
    _check_case(_problem("float32", "main_randn3"), layout, itype)


def test_batched_coo_with_unequal_nnz():
    """Two items with different patterns and entry counts in one block-diagonal walk: each equals its own 2-D reference."""
    tsgu = _tsgu()
    A, B = _problem("float32", "nnz_kR_plus_1_needles"), _problem("float32", "nnz_kR_trailing_needles")
    n, m = max(A.n, B.n), max(A.m, B.m)          # (the items share one shape: the smaller one gets empty rows and columns)
    assert A.nnz != B.nnz
    idx = torch.cat([torch.stack([torch.full_like(P.rows, i), P.rows, P.cols]) for i, P in enumerate((A, B))], dim=1)
    leaf = torch.cat([A.vals, B.vals]).to(DEV).requires_grad_(True)
    S = torch.sparse_coo_tensor(idx.to(DEV), leaf, (2, n, m), is_coalesced=True)

    def pad(x, k, fill=0.0):
        return torch.cat([x, torch.full((k - x.numel(),), fill, dtype=x.dtype)])
    la = torch.stack([pad(P.la, n) for P in (A, B)]).to(DEV).requires_grad_(True)
    lb = torch.stack([pad(P.lb, m) for P in (A, B)]).to(DEV).requires_grad_(True)
    lp, u, v = tsgu.sparse_sinkhorn(S, la, lb, T)
    assert u.shape == (2, n) and v.shape == (2, m) and lp.shape == (2, n, m)
    gu = torch.stack([pad(P.cot[1], n) for P in (A, B)]).to(DEV)
    gv = torch.stack([pad(P.cot[2], m) for P in (A, B)]).to(DEV)
    gP = torch.sparse_coo_tensor(idx.to(DEV), torch.cat([A.cot[0], B.cot[0]]).to(DEV), (2, n, m), is_coalesced=True)
    dS, dla, dlb = torch.autograd.grad((lp, u, v), (leaf, la, lb), (gP, gu, gv))
    at = 0
    for i, P in enumerate((A, B)):
        print(f"\n  item {i}: n {P.n} m {P.m} nnz {P.nnz}")
        _check_potential(u[i, :P.n], P.out[1], P.bound, "u")
        _check_potential(v[i, :P.m], P.out[2], P.bound, "v")
        assert bool(u[i, P.n:].isinf().all()) and bool(v[i, P.m:].isinf().all())
        err = (lp._values()[at:at + P.nnz].detach().cpu().to(F64) - P.out[0]).abs().max()
        assert float(err) <= 3 * P.bound, ("log_P", float(err))
        for what, got, want, yard in zip(("dS", "dlog_a", "dlog_b"), (dS[at:at + P.nnz], dla[i, :P.n], dlb[i, :P.m]), P.grads, P.yard):
            err = float((got.cpu().to(F64) - want).abs().max())
            allowed = max(4 * yard, 64 * EPS["float32"] * float(want.abs().max()))
            print(f"    {what}: error {err:.3e}  yardstick {yard:.3e}  allowed {allowed:.3e}")
            assert err <= allowed, (what, err, allowed)
        at += P.nnz


def test_two_calls_give_the_same_bits():
    tsgu = _tsgu()
    P = _problem("float32", "main_randn3")
    runs = []
    for _ in range(2):
        S, leaf, _ = P.sparse("csr", torch.int32, requires_grad=True)
        la, lb = P.la.to(DEV).requires_grad_(True), P.lb.to(DEV).requires_grad_(True)
        lp, u, v = tsgu.sparse_sinkhorn(S, la, lb, T)
        grads = torch.autograd.grad((lp, u, v), (leaf, la, lb), (_rebuild(lp, P.cot[0].to(DEV)), P.cot[1].to(DEV), P.cot[2].to(DEV)))
        runs.append([_bits(t) for t in (lp.values(), u, v, *grads)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_nothing_of_nnz_size_is_saved_but_the_values():
    tsgu = _tsgu()
    n, m, Ts = 128, 96, 2
    g = torch.Generator().manual_seed(5)
    D = torch.randn(n, m, generator=g)
    S = D.to(DEV).to_sparse_csr().requires_grad_(True)
    nnz = n * m
    assert nnz > 8 * (Ts + 1) * (n + m)
    la, lb = torch.randn(n, generator=g).to(DEV).requires_grad_(True), torch.randn(m, generator=g).to(DEV)
    lp, u, v = tsgu.sparse_sinkhorn(S, la, lb, Ts)
    saved = u.grad_fn.saved_tensors
    big = [t for t in saved if t.numel() >= nnz]
    assert len(big) == 1 and big[0].data_ptr() == S.values().data_ptr(), "only S's own value array"
    assert sum(t.numel() for t in saved) - nnz == Ts * (n + m) + n + m, "u¹..u^T, v¹..v^T (less their marginals) and the two marginals"
    # without a gradient: two buffers, however many iterations (a history of 200 would be 200·(n + m)·4 = 179 200 bytes)
    Tl = 200
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = tsgu.sparse_sinkhorn(S.detach(), la.detach(), lb, Tl)
    torch.cuda.synchronize()
    assert all(t.grad_fn is None for t in out)
    assert Tl * (n + m) * 4 > nnz * 4 + (1 << 16)
    assert torch.cuda.max_memory_allocated() - base < nnz * 4 + (1 << 16), "log_P and a few vectors of n + m, no history"


def test_graph_capture_replays_to_the_eager_bits():
    tsgu = _tsgu()
    P = _problem("float32", "nnz_kR_plus_1_needles")
    S, _, _ = P.sparse("csr", torch.int32)
    la, lb = P.la.to(DEV), P.lb.to(DEV)
    eager = [t.clone() for t in (lambda r: (r[0].values(), r[1], r[2]))(tsgu.sparse_sinkhorn(S, la, lb, 4))]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            lp, u, v = tsgu.sparse_sinkhorn(S, la, lb, 4)
    torch.cuda.current_stream().wait_stream(s)
    for t in (lp.values(), u, v):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (lp.values(), u, v)):
        assert torch.equal(_bits(a), _bits(b))


def test_a_stored_minus_infinity_alone_in_its_row_and_in_its_column():
    """The only entry of a column, and the only entry of a row, are −inf: empty groups for the forward and for the reverse sweep.
    Float64 against the dense restatement, tolerances as in the pipeline test below."""
    tsgu = _tsgu()
    n, m, Ts = 48, 40, 3
    g = torch.Generator().manual_seed(9)
    keep = torch.rand(n, m, generator=g) < 0.3
    keep[torch.arange(n), torch.randint(0, m, (n,), generator=g)] = True
    keep[torch.randint(0, n, (m,), generator=g), torch.arange(m)] = True
    keep[7, :] = False
    keep[:, 13] = False
    keep[7, 2] = keep[3, 13] = True                      # alone in row 7, alone in column 13
    rows, cols = keep.nonzero(as_tuple=True)
    vals = torch.randn(rows.numel(), generator=g, dtype=F64) * 3.0
    alone = ((rows == 7) & (cols == 2)) | ((rows == 3) & (cols == 13))
    vals[alone] = float("-inf")
    la, lb = torch.randn(n, generator=g, dtype=F64), torch.randn(m, generator=g, dtype=F64)
    cot = (torch.randn(rows.numel(), generator=g, dtype=F64), torch.randn(n, generator=g, dtype=F64), torch.randn(m, generator=g, dtype=F64))
    (lp_r, u_r, v_r), grads_r = ref.with_grads(ref.dense, rows, cols, vals, n, m, la, lb, Ts, cot)
    assert u_r[7] == float("inf") and v_r[13] == float("inf")
    leaf = vals.to(DEV).requires_grad_(True)
    crow = torch._convert_indices_from_coo_to_csr(rows.contiguous(), n, out_int32=True)
    S = torch.sparse_csr_tensor(crow.to(DEV), cols.int().to(DEV), leaf, (n, m))
    a, b = la.to(DEV).requires_grad_(True), lb.to(DEV).requires_grad_(True)
    lp, u, v = tsgu.sparse_sinkhorn(S, a, b, Ts)
    got = lp.values().detach().cpu()
    assert bool((got[alone] == float("-inf")).all()) and float((got[~alone] - lp_r[~alone]).abs().max()) <= 3e-11
    _check_potential(u, u_r, 1e-11, "u")
    _check_potential(v, v_r, 1e-11, "v")
    grads = torch.autograd.grad((lp, u, v), (leaf, a, b), (_rebuild(lp, cot[0].to(DEV)), cot[1].to(DEV), cot[2].to(DEV)))
    for what, gg, want in zip(("dS", "dlog_a", "dlog_b"), grads, grads_r):
        gg = gg.cpu()
        assert bool(gg.isfinite().all()), (what, "not finite")
        assert float((gg - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max())), what


def test_topk_then_sinkhorn_pipeline():
    """sparse_topk_mm selects the candidates, sparse_sinkhorn normalises them, the gradient goes back to Q and K: against the dense
    float64 restatement on the selected pattern.  Float64 throughout: 2T·c·ε·M with c ≤ 56 + 8 candidates per row and a few dozen
    per column, M < 100, stays below 1e-11; the gradients, sums of O(T·nnz) such terms, within 1e-9 of the largest entry."""
    tsgu = _tsgu()
    n = m = 256
    d, k, Tp = 32, 8, 5
    g = torch.Generator().manual_seed(21)
    Q0, K0 = torch.randn(n, d, generator=g, dtype=F64), torch.randn(m, d, generator=g, dtype=F64)
    la, lb = torch.randn(n, generator=g, dtype=F64), torch.randn(m, generator=g, dtype=F64)
    Q, K = Q0.to(DEV).requires_grad_(True), K0.to(DEV).requires_grad_(True)
    scale = d ** -0.5
    S = tsgu.sparse_topk_mm(Q, K, k, scale=scale)
    lp, u, v = tsgu.sparse_sinkhorn(S, la.to(DEV), lb.to(DEV), Tp)
    assert lp.crow_indices().data_ptr() == S.crow_indices().data_ptr() and lp.col_indices().data_ptr() == S.col_indices().data_ptr()
    cot = (torch.randn(n * k, generator=g, dtype=F64), torch.randn(n, generator=g, dtype=F64), torch.randn(m, generator=g, dtype=F64))
    some = torch.bincount(S.col_indices().cpu().to(torch.int64), minlength=m) > 0
    cot[2][~some] = 0.0
    dQ, dK = torch.autograd.grad((lp, u, v), (Q, K), (_rebuild(lp, cot[0].to(DEV)), cot[1].to(DEV), cot[2].to(DEV)))
    rows = torch.repeat_interleave(torch.arange(n), k)
    cols = S.col_indices().cpu().to(torch.int64)
    Qr, Kr = Q0.clone().requires_grad_(True), K0.clone().requires_grad_(True)
    lp_r, u_r, v_r = ref.dense(rows, cols, (Qr[rows] * Kr[cols]).sum(1) * scale, n, m, la, lb, Tp)
    dQ_r, dK_r = torch.autograd.grad((lp_r, u_r, v_r), (Qr, Kr), cot)
    _check_potential(u, u_r.detach(), 1e-11, "u")
    _check_potential(v, v_r.detach(), 1e-11, "v")
    assert float((lp.values().detach().cpu() - lp_r.detach()).abs().max()) <= 3e-11
    for what, got, want in (("dQ", dQ, dQ_r), ("dK", dK, dK_r)):
        err = float((got.cpu() - want).abs().max())
        print(f"    {what}: error {err:.3e}  max|grad| {float(want.abs().max()):.3e}")
        assert err <= 1e-9 * max(1.0, float(want.abs().max())), (what, err)
