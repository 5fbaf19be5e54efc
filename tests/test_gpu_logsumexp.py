"""sparse_logsumexp / sparse_bidir_logsumexp on the MI355X: golden parity, bit-level contracts (bidir, determinism, graph
replay), gradients the reference cannot take, and full-size patterns against a float64 reference."""

import numpy as np
import pytest
import torch

import _lse_cases
import _lse_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -23


def _tsgu():
    import torchsparsegradutils_amd as tsgu

    return tsgu


@pytest.mark.filterwarnings("ignore")
def test_golden_parity_on_gpu():
    tsgu = _tsgu()
    z, names = _lse_ref.cases()
    for name in names:
        _lse_ref.check_case(tsgu, z, name, "cuda:0")


@pytest.mark.filterwarnings("ignore")
def test_bidir_is_bitwise_two_calls_and_views_of_padded():
    tsgu = _tsgu()
    z, names = _lse_ref.cases()
    seen = 0
    for name in names:
        meta, _, A = _lse_ref.build(z, name, "cuda:0")
        if meta["fn"] != "bidir" or meta["layout"] != "tuple" or meta["keepdim"]:
            continue
        iz = meta["include_zeros"]
        off = 1 if A.dim() == 3 else 0
        c, r = tsgu.sparse_bidir_logsumexp(A, include_zeros=iz)
        assert torch.equal(c.nan_to_num(), tsgu.sparse_logsumexp(A, off, include_zeros=iz).nan_to_num()), name
        assert torch.equal(r.nan_to_num(), tsgu.sparse_logsumexp(A, off + 1, include_zeros=iz).nan_to_num()), name
        assert c._base is not None and c._base is r._base
        padded = tsgu.sparse_bidir_logsumexp(A, include_zeros=iz, output_layout="padded")
        assert torch.equal(padded[0, ..., : c.size(-1)].nan_to_num(), c.nan_to_num())
        assert torch.equal(padded[1, ..., : r.size(-1)].nan_to_num(), r.nan_to_num())
        G = padded.size(-1)
        assert bool((padded[0, ..., c.size(-1):] == float("-inf")).all()) and bool((padded[1, ..., r.size(-1):] == float("-inf")).all())
        assert G == max(c.size(-1), r.size(-1))
        seen += 1
    assert seen >= 20


def _dense_grad(d, mask, dim, w):
    """Gradient of Σ w · logsumexp(dense) w.r.t. the stored entries (fp64 autograd)."""
    x = d.clone().requires_grad_(True)
    out = torch.logsumexp(x, dim)
    gx, = torch.autograd.grad(out, x, w)
    return gx[mask]


@pytest.mark.parametrize("kind", ["csc", "csr_batched", "csc_batched"])
def test_gradients_the_reference_cannot_take(kind):
    tsgu = _tsgu()
    g = torch.Generator().manual_seed(11)
    shape = (3, 9, 7) if kind.endswith("batched") else (9, 7)
    d = torch.randn(shape, generator=g, dtype=torch.float64)
    pat = torch.rand(shape[-2:], generator=g) < 0.5
    pat[2] = False
    d[..., pat] = 0
    S = (d.to_sparse_csc() if kind.startswith("csc") else d.to_sparse_csr()).to(DEV)
    for dim in ([0] if d.dim() == 2 else [1]) + ([1] if d.dim() == 2 else [2]) + ([[0, 1]] if d.dim() == 2 else [[1, 2]]):
        if kind.startswith("csc"):
            A = torch.sparse_csc_tensor(S.ccol_indices(), S.row_indices(), S.values().clone(), S.shape).requires_grad_(True)
        else:
            A = torch.sparse_csr_tensor(S.crow_indices(), S.col_indices(), S.values().clone(), S.shape).requires_grad_(True)
        out = tsgu.sparse_logsumexp(A, dim)
        w = torch.rand(out.shape, generator=g, dtype=torch.float64) + 0.5
        gA, = torch.autograd.grad(out, A, w.to(DEV))
        assert gA.layout == A.layout
        if kind.startswith("csc"):
            assert gA.ccol_indices().data_ptr() == A.ccol_indices().data_ptr()
            assert gA.row_indices().data_ptr() == A.row_indices().data_ptr()
        else:
            assert gA.crow_indices().data_ptr() == A.crow_indices().data_ptr()
            assert gA.col_indices().data_ptr() == A.col_indices().data_ptr()
        mask = (d != 0)
        want = _dense_grad(d, mask, dim, w)
        # the stored order of the sparse values vs the dense mask order: compare through to_dense
        got = gA.detach().cpu().to_dense()[mask]
        torch.testing.assert_close(got, want, atol=1e-10, rtol=1e-10)


def _c2_pattern():
    from torchsparsegradutils_amd.utils import synthetic

    crow, col = synthetic.stencil27_periodic(100, 100, 100, torch.int32)
    return crow, col


def _bound(lse_ref, k, ptr):
    """|fp32 result − fp64 value| for a group of k exp terms: _lse_ref.fwd_bound, the smaller of (2k + 8)·ε + 4ε·|lse| (k sums of
    rounded exp terms and the rescaling of partials: ≤ 2k roundings of relative ε on a total that is ≥ 1 after the shift, the
    log and the shift add a few ε, and the shift itself is exact up to 4ε·|lse|) and the reduction-depth form over the
    group's range pieces."""
    return _lse_ref.fwd_bound(lse_ref, k, _lse_cases.pieces(ptr, _lse_cases.range_len("float32")), EPS32)


def _check_full(crow, col, val, n_rows, n_cols, include_zeros):
    tsgu = _tsgu()
    A = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), val.to(DEV), (n_rows, n_cols)).requires_grad_(True)
    c, r = tsgu.sparse_bidir_logsumexp(A, include_zeros=include_zeros)
    gr = torch.rand(n_rows, dtype=torch.float32) + 0.5
    gc = torch.rand(n_cols, dtype=torch.float32) + 0.5
    gA, = torch.autograd.grad((c, r), A, (gc.to(DEV), gr.to(DEV)))
    crow_np, col_np, v64 = crow.numpy().astype(np.int64), col.numpy().astype(np.int64), val.numpy().astype(np.float64)
    lr, kr = _lse_ref.group_lse(crow_np, v64, n_cols if include_zeros else None)
    order = np.argsort(col_np, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(col_np, minlength=n_cols))])
    lc, kc = _lse_ref.group_lse(tptr, v64[order], n_rows if include_zeros else None)
    for got, ref, k, ptr in ((r, lr, kr, crow_np), (c, lc, kc, tptr)):
        got = got.detach().cpu().numpy().astype(np.float64)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], ref[~fin])
        err = np.abs(got[fin] - ref[fin])
        assert (err <= _bound(ref, k, ptr)[fin]).all(), float(err.max())
    # gradient: per entry Σ_dir g·exp(v − lse); the fp32 exp of a difference of size ≤ |lse| carries ≤ (|v| + |lse| + 2)·2ε relative
    grad_ref = _lse_ref.group_lse_grad(crow_np, v64, gr.numpy(), lr)
    gcol = np.empty_like(v64)
    gcol[order] = _lse_ref.group_lse_grad(tptr, v64[order], gc.numpy(), lc)
    grad_ref = grad_ref + gcol
    got = gA.values().detach().cpu().numpy().astype(np.float64)
    scale = np.abs(v64) + np.abs(lr[np.repeat(np.arange(n_rows), np.diff(crow_np))]) + np.abs(lc[col_np]) + 4
    assert (np.abs(got - grad_ref) <= 4 * EPS32 * scale * np.abs(grad_ref) + 1e-30).all()
    return A


@pytest.mark.parametrize("include_zeros", [False, True])
def test_c2_pattern_full_size(include_zeros):
    crow, col = _c2_pattern()
    n = crow.numel() - 1
    g = torch.Generator().manual_seed(5)
    val = torch.randn(col.numel(), generator=g) * 3
    _check_full(crow, col, val, n, n, include_zeros)


def test_ragged_long_row_full_size():
    g = torch.Generator().manual_seed(6)
    n_short, long_len, n_cols = 100_000, 1 << 20, 1 << 21
    lens = torch.randint(0, 9, (n_short,), generator=g)
    lens[torch.rand(n_short, generator=g) < 0.2] = 0          # empty rows
    lens = torch.cat([lens[:500], torch.tensor([long_len]), lens[500:], torch.zeros(1000, dtype=torch.int64)])
    crow = torch.zeros(lens.numel() + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(lens, 0)
    nnz = int(crow[-1])
    col = torch.randint(0, n_cols, (nnz,), generator=g, dtype=torch.int64)
    val = torch.randn(nnz, generator=g) * 2
    A = _check_full(crow.int(), col.int(), val, lens.numel(), n_cols, False)
    assert A.shape[0] == lens.numel()


def test_repeat_calls_give_identical_bits():
    tsgu = _tsgu()
    crow, col = _c2_pattern()
    n = crow.numel() - 1
    val = torch.randn(col.numel(), generator=torch.Generator().manual_seed(2))
    res = []
    for _ in range(2):
        A = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), val.to(DEV), (n, n)).requires_grad_(True)
        c, r = tsgu.sparse_bidir_logsumexp(A)
        s = tsgu.sparse_logsumexp(A, [0, 1])
        gA, = torch.autograd.grad((c, r, s), A, (torch.ones_like(c), torch.full_like(r, 0.5), torch.ones_like(s)))
        res.append((c.detach().clone(), r.detach().clone(), s.detach().clone(), gA.values().clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_bf16_rounds_the_fp32_result_once():
    tsgu = _tsgu()
    crow, col = _c2_pattern()
    n = crow.numel() - 1
    vb = torch.randn(col.numel(), generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    A16 = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), vb.to(DEV), (n, n))
    A32 = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), vb.float().to(DEV), (n, n))
    for dim in (0, 1, [0, 1]):
        got = tsgu.sparse_logsumexp(A16, dim)
        assert got.dtype == torch.bfloat16
        assert torch.equal(got, tsgu.sparse_logsumexp(A32, dim).to(torch.bfloat16)), dim


def test_graph_capture_replays_to_the_same_bits():
    tsgu = _tsgu()
    crow, col = _c2_pattern()
    n = crow.numel() - 1
    val = torch.randn(col.numel(), generator=torch.Generator().manual_seed(8)).to(DEV)
    A = torch.sparse_csr_tensor(crow.to(DEV), col.to(DEV), val, (n, n))
    eager = [t.clone() for t in tsgu.sparse_bidir_logsumexp(A)] + [tsgu.sparse_logsumexp(A, [0, 1]).clone()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            c, r = tsgu.sparse_bidir_logsumexp(A)
            t = tsgu.sparse_logsumexp(A, [0, 1])
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, (c, r, t)):
        assert torch.equal(a, b)
