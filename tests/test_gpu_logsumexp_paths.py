"""The log-sum-exp kernels' range, merge and window paths against float64, for every value and index type.

Two kinds of input go through the public API: the structural cases of _lse_cases (groups placed on the kernels' branch
points, with needle values that make a lost, doubled or misassigned partial visible) as the rows of a CSR matrix and the
columns of a CSC matrix, and one ragged random pattern in every layout (2-D and batched CSR / CSC / COO, coalesced or not).
Forward results are compared with _lse_ref.group_lse under _lse_ref.fwd_bound (fp32 / fp64) or within one bf16 ulp, and
exactly where the float64 value is clear of a rounding midpoint; gradients with Σ_dir g·exp(v − lse) in float64.
"""

import functools

import numpy as np
import pytest
import torch

import _lse_cases
import _lse_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TORCH = {"float32": torch.float32, "float64": torch.float64, "bfloat16": torch.bfloat16}
BITS = {"float32": torch.int32, "float64": torch.int64, "bfloat16": torch.int16}
EPS = {"float32": 2.0 ** -23, "float64": 2.0 ** -52, "bfloat16": 2.0 ** -23}   # bf16 accumulates in fp32
DTYPES = list(_lse_cases.DTYPES)
ITYPES = [torch.int32, torch.int64]


def _tsgu():
    import torchsparsegradutils_amd as tsgu

    return tsgu


def _np(t):
    return t.detach().cpu().to(torch.float64).numpy()


def _bits(t, dtype):
    return t.detach().contiguous().view(BITS[dtype]).cpu()


def _bf16_round(x):
    """float64 → nearest bf16 (ties to even), in float64; and the distance of x from the nearest rounding midpoint."""
    m, e = np.frexp(x)                         # x = m·2^e, 0.5 ≤ |m| < 1: 8 significant bits are m·2^8
    with np.errstate(invalid="ignore"):
        q = np.ldexp(m, 8)
        r = np.ldexp(np.rint(q), e - 8)
        mid = np.ldexp(np.floor(q) + 0.5, e - 8)
    return r, np.abs(x - mid)


def _bf16_ulp(x):
    with np.errstate(divide="ignore"):
        return np.ldexp(1.0, (np.frexp(np.abs(x))[1] - 8).astype(np.int64))


def _same_specials(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, "NaN", np.flatnonzero(np.isnan(got) != np.isnan(ref))[:8])
    for sign in (1, -1):
        g_inf, r_inf = np.isinf(got) & (np.sign(got) == sign), np.isinf(ref) & (np.sign(ref) == sign)
        assert np.array_equal(g_inf, r_inf), (what, sign, "inf", np.flatnonzero(g_inf != r_inf)[:8], got[g_inf != r_inf][:8])


def check_forward(got, ref, k, pcs, dtype, what):
    """Kernel output `got` (tensor) against the float64 group values `ref` (k terms and pcs range pieces per group)."""
    got = _np(got).reshape(-1)
    ref, k, pcs = np.asarray(ref).reshape(-1), np.asarray(k).reshape(-1), np.asarray(pcs).reshape(-1)
    _same_specials(got, ref, what)
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    bound = _lse_ref.fwd_bound(ref[fin], k[fin], pcs[fin], EPS[dtype])
    if dtype != "bfloat16":
        bad = err > bound
        assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(fin)[bad][:8], err[bad][:8], bound[bad][:8])
        return
    assert (err <= _bf16_ulp(ref[fin])).all(), (what, "bf16 ulp", float(err.max()))
    rounded, dmid = _bf16_round(ref[fin])
    clear = dmid > bound
    bad = clear & (got[fin] != rounded)
    assert not bad.any(), (what, "bf16 rounding", int(bad.sum()), got[fin][bad][:8], ref[fin][bad][:8])


def check_grad(got, ref, scale, lse_err, dtype, what):
    """fp32 / fp64: |got − ref| ≤ (4ε·scale + lse_err)·|ref| — the full-size tests' form (scale = |v| + Σ|lse| + 4: the exp of a
    difference of that size) plus the forward bound of the lse the kernel used (lse_err, summed over the directions), which
    carries into exp(v − lse) as the same relative error; bf16: one bf16 ulp of the float64 value of the formula evaluated with
    the kernel's own lse (fp32 arithmetic, one rounding)."""
    got = _np(got).reshape(-1)
    _same_specials(got, ref, what + " grad")
    fin = np.isfinite(ref)
    err = np.abs(got[fin] - ref[fin])
    if dtype == "bfloat16":
        tol = _bf16_ulp(ref[fin]) + 2.0 ** -125
    else:
        tol = (4 * EPS[dtype] * scale[fin] + lse_err[fin]) * np.abs(ref[fin]) + 1e-30
    bad = err > tol
    assert not bad.any(), (what, "grad", int(bad.sum()), np.flatnonzero(fin)[bad][:8], err[bad][:8], tol[bad][:8])


def _lse_err(ref, k, pcs, dtype):
    """The forward bound of every group with a finite value (0 elsewhere: there the gradient is exactly 0 or NaN)."""
    fin = np.isfinite(ref)
    return np.where(fin, _lse_ref.fwd_bound(np.where(fin, ref, 0.0), k, pcs, EPS[dtype]), 0.0)


# ----------------------------------------------------------------------------------------------------------------------------
# structural cases


@functools.lru_cache(maxsize=None)
def _cases(dtype):
    return _lse_cases.structural_cases(dtype)


def _compressed(layout, ptr, idx, vals, G, N, itype):
    p, i = torch.from_numpy(ptr).to(itype).to(DEV), torch.from_numpy(idx).to(itype).to(DEV)
    if layout == "csr":
        return torch.sparse_csr_tensor(p, i, vals, (G, N))
    return torch.sparse_csc_tensor(p, i, vals, (N, G))


def _unaligned(vals):
    buf = torch.zeros(vals.numel() + 1, dtype=vals.dtype, device=vals.device)
    buf[1:] = vals
    return buf[1:]


@pytest.mark.parametrize("itype", ITYPES, ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_structural_cases(dtype, itype):
    """Every structural case as CSR rows (dim=1) and CSC columns (dim=0), both include_zeros: forward and gradient against
    float64; on CSR also the unaligned-values paths, bit for bit against the aligned call."""
    tsgu = _tsgu()
    R = _lse_cases.range_len(dtype)
    td = TORCH[dtype]
    gen = torch.Generator().manual_seed(17)
    for name, ptr, v in _cases(dtype):
        G, N = ptr.size - 1, _lse_cases.axis_len_of(ptr)
        idx = _lse_cases.columns(ptr)
        vt = torch.from_numpy(v).to(td)
        v64 = _np(vt)
        pcs = _lse_cases.pieces(ptr, R)
        grp = np.repeat(np.arange(G), np.diff(ptr))
        vdev = vt.to(DEV)
        for iz in (False, True):
            ref, k = _lse_ref.group_lse(ptr, v64, N if iz else None)
            w = (torch.rand(G, generator=gen, dtype=torch.float64) + 0.5).to(td)
            w64 = _np(w)
            for layout in ("csr", "csc"):
                what = f"{dtype} {itype} {name} {layout} include_zeros={iz}"
                A = _compressed(layout, ptr, idx, vdev.clone(), G, N, itype).requires_grad_(True)
                out = tsgu.sparse_logsumexp(A, 1 if layout == "csr" else 0, include_zeros=iz)
                assert out.shape == (G,) and out.dtype == td
                check_forward(out, ref, k, pcs, dtype, what)
                gA, = torch.autograd.grad(out, A, w.to(DEV))
                assert gA.layout == A.layout
                p_of = (lambda T: T.crow_indices()) if layout == "csr" else (lambda T: T.ccol_indices())   # noqa: E731
                i_of = (lambda T: T.col_indices()) if layout == "csr" else (lambda T: T.row_indices())     # noqa: E731
                assert p_of(gA).data_ptr() == p_of(A).data_ptr() and i_of(gA).data_ptr() == i_of(A).data_ptr()
                lse_used = _np(out) if dtype == "bfloat16" else ref
                with np.errstate(invalid="ignore", over="ignore"):
                    gref = w64[grp] * np.exp(v64 - lse_used[grp])
                scale = np.abs(v64) + np.abs(ref[grp]) + 4
                check_grad(gA.values(), gref, scale, _lse_err(ref, k, pcs, dtype)[grp], dtype, what)
                if layout == "csr" and not iz:
                    U = _compressed(layout, ptr, idx, _unaligned(vdev), G, N, itype).requires_grad_(True)
                    assert U.values().data_ptr() % 16 != 0 or ptr[-1] == 0
                    out_u = tsgu.sparse_logsumexp(U, 1, include_zeros=iz)
                    assert torch.equal(_bits(out_u, dtype), _bits(out, dtype)), what + " unaligned forward"
                    gU, = torch.autograd.grad(out_u, U, w.to(DEV))
                    assert torch.equal(_bits(gU.values(), dtype), _bits(gA.values(), dtype)), what + " unaligned gradient"


# ----------------------------------------------------------------------------------------------------------------------------
# one random pattern through every layout


def _coords_2d(rng, r, c, nnz, long_rows=3):
    """Unique (row, col) of a ragged pattern: ~20 % empty rows, ~10 % empty columns, a few rows of most columns."""
    lens = rng.geometric(r / nnz, r).astype(np.int64) - 1
    lens[rng.random(r) < 0.2] = 0
    live_cols = np.flatnonzero(rng.random(c) >= 0.1)
    lens = np.minimum(lens, live_cols.size)
    lens[rng.choice(r, long_rows, replace=False)] = live_cols.size - rng.integers(0, 50, long_rows)
    rows = np.repeat(np.arange(r), lens)
    cols = np.concatenate([np.sort(rng.choice(live_cols, n, replace=False)) for n in lens])
    return rows, cols


def _pattern(dtype, seed=23):
    """[(name, sparse input on the GPU, (b, r, c))] and per name the coalesced coordinates (bi, ri, ci, values)."""
    td = TORCH[dtype]
    rng = np.random.default_rng(seed)
    items = []
    r, c = 3000, 2000
    ri, ci = _coords_2d(rng, r, c, 120_000)
    v = torch.from_numpy(rng.standard_normal(ri.size) * 3).to(td)
    bi = np.zeros(ri.size, dtype=np.int64)
    items.append(("csr", (1, r, c), bi, ri, ci, v))
    order = np.lexsort((ri, ci))
    items.append(("csc", (1, r, c), bi, ri[order], ci[order], v[torch.from_numpy(order)]))
    items.append(("coo", (1, r, c), bi, ri, ci, v))
    items.append(("coo_uncoalesced", (1, r, c), bi, ri, ci, v))
    for name, (b, r, c), equal in (("bcsr", (3, 700, 1100), True), ("bcsc", (3, 1100, 700), True),
                                   ("bcoo", (3, 700, 1100), False), ("bcoo_tall", (3, 1100, 700), False)):
        parts = [_coords_2d(rng, r, c, [20_000, 35_000, 9_000][i]) for i in range(b)]
        if equal:
            n = min(p[0].size for p in parts)
            parts = [(pr[:n], pc[:n]) for pr, pc in parts]
        if name == "bcsc":
            parts = [(pr[np.lexsort((pr, pc))], pc[np.lexsort((pr, pc))]) for pr, pc in parts]
        bi = np.concatenate([np.full(p[0].size, i) for i, p in enumerate(parts)])
        ri = np.concatenate([p[0] for p in parts])
        ci = np.concatenate([p[1] for p in parts])
        v = torch.from_numpy(rng.standard_normal(ri.size) * 3).to(td)
        items.append((name, (b, r, c), bi, ri, ci, v))
    return items


def _make(name, shape, bi, ri, ci, v, itype, rng):
    """(leaf sparse tensor on the GPU, coalesced (bi, ri, ci) in the stored order of its values or None for uncoalesced)."""
    b, r, c = shape
    batched = name.startswith("b")
    if name in ("csr", "bcsr"):
        crow = np.stack([np.concatenate([[0], np.cumsum(np.bincount(ri[bi == i], minlength=r))]) for i in range(b)])
        col = ci.reshape(b, -1)
        vv = v.reshape(b, -1)
        if not batched:
            crow, col, vv = crow[0], col[0], vv[0]
        A = torch.sparse_csr_tensor(torch.from_numpy(crow).to(itype).to(DEV), torch.from_numpy(col).to(itype).to(DEV),
                                    vv.to(DEV), shape[1:] if not batched else shape)
        return A, (bi, ri, ci)
    if name in ("csc", "bcsc"):
        ccol = np.stack([np.concatenate([[0], np.cumsum(np.bincount(ci[bi == i], minlength=c))]) for i in range(b)])
        row = ri.reshape(b, -1)
        vv = v.reshape(b, -1)
        if not batched:
            ccol, row, vv = ccol[0], row[0], vv[0]
        A = torch.sparse_csc_tensor(torch.from_numpy(ccol).to(itype).to(DEV), torch.from_numpy(row).to(itype).to(DEV),
                                    vv.to(DEV), shape[1:] if not batched else shape)
        return A, (bi, ri, ci)
    idx = np.stack([bi, ri, ci]) if batched else np.stack([ri, ci])
    if name == "coo_uncoalesced":
        # every 7th entry split into two duplicates (a, v − a), and the entries shuffled
        dup = np.arange(0, ri.size, 7)
        a = (v[torch.from_numpy(dup)].to(torch.float64) * 0.25).to(v.dtype)
        v2 = v.clone()
        v2[torch.from_numpy(dup)] = v[torch.from_numpy(dup)] - a
        idx = np.concatenate([idx, idx[:, dup]], axis=1)
        vals = torch.cat([v2, a])
        perm = rng.permutation(idx.shape[1])
        idx, vals = idx[:, perm], vals[torch.from_numpy(perm)]
        A = torch.sparse_coo_tensor(torch.from_numpy(idx).to(DEV), vals.to(DEV), shape[1:] if not batched else shape)
        return A, None
    A = torch.sparse_coo_tensor(torch.from_numpy(idx).to(DEV), v.to(DEV), shape[1:] if not batched else shape,
                                is_coalesced=True)
    return A, (bi, ri, ci)


def _ref_dir(bi, ri, ci, v64, shape, kind, iz, dtype):
    """(lse (b, per), k, pieces, entry → group) of one direction in float64."""
    b, r, c = shape
    key, n, axis = {"row": (bi * r + ri, b * r, c), "col": (bi * c + ci, b * c, r), "all": (bi, b, r * c)}[kind]
    order = np.argsort(key, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))])
    lse, k = _lse_ref.group_lse(ptr, v64[order], axis if iz else None)
    return lse.reshape(b, -1), k.reshape(b, -1), _lse_cases.pieces(ptr, _lse_cases.range_len(dtype)).reshape(b, -1), key


def _grad_of(gA, A, name):
    """Gradient values in the stored order of the (coalesced) input."""
    if A.layout in (torch.sparse_csr, torch.sparse_csc):
        assert gA.layout == A.layout
        p_of = (lambda T: T.crow_indices()) if A.layout == torch.sparse_csr else (lambda T: T.ccol_indices())  # noqa: E731
        i_of = (lambda T: T.col_indices()) if A.layout == torch.sparse_csr else (lambda T: T.row_indices())    # noqa: E731
        assert p_of(gA).data_ptr() == p_of(A).data_ptr() and i_of(gA).data_ptr() == i_of(A).data_ptr(), name
        return gA.values().reshape(-1)
    g = gA.coalesce()
    assert torch.equal(g._indices(), A.coalesce()._indices()), name
    if A.is_coalesced():
        assert torch.equal(gA._indices(), A._indices()), name
    return g._values()


@pytest.mark.parametrize("itype", ITYPES, ids=["i32", "i64"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_pattern_every_layout(dtype, itype):
    """2-D and batched CSR / CSC / COO (coalesced and not): dim 0, 1, [0, 1] (batched 1, 2, [1, 2]) and bidir in the tuple and
    padded layouts, both include_zeros, forward and gradient against float64; repeat calls and bidir against the two single
    calls bit for bit.  COO indices are int64 whatever `itype`, so the COO layouts run once (int64)."""
    tsgu = _tsgu()
    td = TORCH[dtype]
    rng = np.random.default_rng(5)
    gen = torch.Generator().manual_seed(29)
    for name, shape, bi, ri, ci, v in _pattern(dtype):
        if "coo" in name and itype == torch.int32:
            continue
        A0, coords = _make(name, shape, bi, ri, ci, v, itype, rng)
        if coords is None:
            C = A0.detach().cpu().coalesce()
            ix = C._indices().numpy()
            bi_, ri_, ci_ = (ix[0], ix[1], ix[2]) if A0.dim() == 3 else (np.zeros(ix.shape[1], np.int64), ix[0], ix[1])
            v64 = _np(C._values())
        else:
            bi_, ri_, ci_ = coords
            v64 = _np(A0.detach().values() if A0.layout != torch.sparse_coo else A0.detach()._values()).reshape(-1)
        batched = A0.dim() == 3
        b, r, c = shape
        off = 1 if batched else 0
        refs = {}
        for iz in (False, True):
            for kind in ("row", "col", "all"):
                refs[kind, iz] = _ref_dir(bi_, ri_, ci_, v64, shape, kind, iz, dtype)
            calls = [((off,), ("col",)), ((off + 1,), ("row",)), ((off, off + 1), ("all",)), ("bidir", ("col", "row")),
                     ("padded", ("col", "row"))]
            for how, kinds in calls:
                what = f"{dtype} {itype} {name} {how} include_zeros={iz}"
                A = A0.detach().clone().requires_grad_(True) if A0.layout != torch.sparse_coo else \
                    torch.sparse_coo_tensor(A0._indices(), A0._values().detach().clone(), A0.shape,
                                            is_coalesced=A0.is_coalesced() or None).requires_grad_(True)
                if how == "bidir":
                    outs = list(tsgu.sparse_bidir_logsumexp(A, include_zeros=iz))
                elif how == "padded":
                    P = tsgu.sparse_bidir_logsumexp(A, include_zeros=iz, output_layout="padded")
                    G = max(r, c)
                    assert P.shape == ((2, b, G) if batched else (2, G))
                    assert bool((P[0, ..., c:] == float("-inf")).all()) and bool((P[1, ..., r:] == float("-inf")).all()), what
                    outs = [P[0, ..., :c], P[1, ..., :r]]
                else:
                    dim = list(how) if len(how) == 2 else how[0]
                    outs = [tsgu.sparse_logsumexp(A, dim, include_zeros=iz)]
                gsum = np.zeros(v64.size)
                scale = np.abs(v64) + 4
                lse_err = np.zeros(v64.size)
                ws = []
                for o, kind in zip(outs, kinds):
                    lse, k, pcs, key = refs[kind, iz]
                    assert o.dtype == td and o.numel() == lse.size, what
                    check_forward(o, lse, k, pcs, dtype, f"{what} {kind}")
                    w = (torch.rand(o.shape, generator=gen, dtype=torch.float64) + 0.5).to(td)
                    ws.append(w.to(DEV))
                    lse_used = _np(o).reshape(-1) if dtype == "bfloat16" else lse.reshape(-1)
                    with np.errstate(invalid="ignore", over="ignore"):
                        gsum = gsum + _np(w).reshape(-1)[key] * np.exp(v64 - lse_used[key])
                    scale = scale + np.abs(lse.reshape(-1)[key])
                    lse_err = lse_err + _lse_err(lse.reshape(-1), k.reshape(-1), pcs.reshape(-1), dtype)[key]
                gA, = torch.autograd.grad(outs, A, ws)
                check_grad(_grad_of(gA, A, what), gsum, scale, lse_err, dtype, what)
        # bit-level contracts (include_zeros=True): repeat calls, and bidir == the two single calls
        A = A0.detach()
        c1, r1 = tsgu.sparse_bidir_logsumexp(A)
        c2, r2 = tsgu.sparse_bidir_logsumexp(A)
        s1, s2 = tsgu.sparse_logsumexp(A, [off, off + 1]), tsgu.sparse_logsumexp(A, [off, off + 1])
        for x, y in ((c1, c2), (r1, r2), (s1, s2), (c1, tsgu.sparse_logsumexp(A, off)),
                     (r1, tsgu.sparse_logsumexp(A, off + 1))):
            assert torch.equal(_bits(x, dtype), _bits(y, dtype)), f"{dtype} {itype} {name} bits"
        grads = []
        for _ in range(2):
            L = A0.detach().clone().requires_grad_(True) if A0.layout != torch.sparse_coo else \
                torch.sparse_coo_tensor(A0._indices(), A0._values().detach().clone(), A0.shape,
                                        is_coalesced=A0.is_coalesced() or None).requires_grad_(True)
            cc, rr = tsgu.sparse_bidir_logsumexp(L)
            gL, = torch.autograd.grad((cc, rr), L, (torch.ones_like(cc), torch.full_like(rr, 0.5)))
            grads.append(_grad_of(gL, L, name))
        assert torch.equal(_bits(grads[0], dtype), _bits(grads[1], dtype)), f"{dtype} {itype} {name} gradient bits"


@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_values_random_pattern(dtype):
    """The random 2-D pattern with its values at storage offset 1, for CSR, CSC and coalesced COO: bidir and dim=[0, 1]
    forward and gradient bit for bit equal to the aligned call."""
    tsgu = _tsgu()
    rng = np.random.default_rng(9)
    for name, shape, bi, ri, ci, v in _pattern(dtype)[:3]:
        A0, _ = _make(name, shape, bi, ri, ci, v, torch.int64, rng)
        res = []
        for unaligned in (False, True):
            vals = (A0.values() if A0.layout != torch.sparse_coo else A0._values()).detach().clone()
            if unaligned:
                vals = _unaligned(vals)
            if A0.layout == torch.sparse_csr:
                A = torch.sparse_csr_tensor(A0.crow_indices(), A0.col_indices(), vals, A0.shape)
            elif A0.layout == torch.sparse_csc:
                A = torch.sparse_csc_tensor(A0.ccol_indices(), A0.row_indices(), vals, A0.shape)
            else:
                A = torch.sparse_coo_tensor(A0._indices(), vals, A0.shape, is_coalesced=True)
            A.requires_grad_(True)
            got_ptr = (A.values() if A.layout != torch.sparse_coo else A._values()).data_ptr()
            assert (got_ptr % 16 != 0) == unaligned, name
            c, r = tsgu.sparse_bidir_logsumexp(A)
            s = tsgu.sparse_logsumexp(A, [0, 1])
            gA, = torch.autograd.grad((c, r), A, (torch.ones_like(c), torch.full_like(r, 0.5)))
            gS, = torch.autograd.grad(s, A, torch.ones_like(s))
            res.append([_bits(t, dtype) for t in (c, r, s, _grad_of(gA, A, name), _grad_of(gS, A, name))])
        for x, y in zip(*res):
            assert torch.equal(x, y), (dtype, name)
