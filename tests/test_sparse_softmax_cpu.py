"""sparse_softmax / sparse_log_softmax without a GPU: names and refusals, the torch-op path against torch.sparse.softmax /
log_softmax on the coalesced float64 COO of the same matrix, special values, the forms an upstream gradient arrives in, index
identity, and the C ABI of include/tsgu_hip_softmax.h (exports, ctypes table, host-side refusals with device = -1).

The oracle is called with non-negative dims: the backward of torch.sparse.softmax on this torch reduces over nothing when it
is handed a negative dim (every entry its own group), which a dense computation contradicts.

Tolerances: the torch-op path computes float32 and bfloat16 inputs in float32, float64 in float64.  Groups here have at most 27
entries and |v - m| < 16, so (L + |v - m| + 16) u < 60 u: 1e-5 relative for float32 (60 · 2^-24 = 3.6e-6), 1e-13 for float64;
bfloat16 adds its one rounding (2^-8 relative: 8 significant bits) for the values, and for the gradients the roundings of the
stored y it is computed from and of the result, each met twice in y (g - sum g y): 2^-6 of the gradient's scale.
"""

import ctypes
import os
import re

import pytest
import torch

from _abi_cases import BAD_ARG, BAD_DTYPE, OK, TOO_LARGE
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, _pattern
from torchsparsegradutils_amd import sparse_log_softmax, sparse_softmax          # (ImportError before the operators existed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = {torch.float32: 1e-5, torch.float64: 1e-13, torch.bfloat16: 2.0 ** -8}
REL_GRAD = {torch.float32: 1e-5, torch.float64: 1e-13, torch.bfloat16: 2.0 ** -6}
FUNCS = {"softmax": (sparse_softmax, torch.sparse.softmax), "log_softmax": (sparse_log_softmax, torch.sparse.log_softmax)}


# ---------------------------------------------------------------------------------------------------------------------------
# inputs and the oracle


def _mask(n, m, density, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand((n, m), generator=g) < density
    mask[n // 2] = False        # an empty row and an empty column
    mask[:, m // 3] = False
    return mask


def _stencil_mask():
    from torchsparsegradutils_amd.encoders import PairwiseEncoder

    enc = PairwiseEncoder(radius=1.8, volume_shape=(1, 4, 4, 4), diag=True, layout=torch.sparse_csr)
    A = enc(torch.ones((len(enc.offsets), 1, 4, 4, 4)))
    return A.to_dense() != 0


def _dense_values(mask, batch, seed):
    g = torch.Generator().manual_seed(seed)
    shape = mask.shape if batch is None else (batch,) + tuple(mask.shape)
    D = torch.randn(shape, generator=g, dtype=torch.float64).clamp(-6, 6)
    D = torch.where(D == 0, torch.ones_like(D), D)
    return D * mask


def _sparse(D, mask, layout, index_dtype, dtype):
    """D (zero outside mask, non-zero inside) in the layout, with the index dtype where the layout has a choice."""
    D = D.to(dtype)
    if layout == "coo":
        return D.to_sparse_coo().coalesce()
    if layout == "coo_uncoalesced":
        C = D.to_sparse_coo().coalesce()
        order = torch.randperm(C._nnz(), generator=torch.Generator().manual_seed(1))
        half = C.values()[order] / 2          # every entry twice, shuffled: coalescing sums them back (exact: a power of two)
        A = torch.sparse_coo_tensor(torch.cat([C.indices()[:, order], C.indices()[:, order.flip(0)]], 1),
                                    torch.cat([half, half.flip(0)]), D.shape)
        assert not A.is_coalesced()
        return A
    if layout == "csr":
        A = D.to_sparse_csr()
        return torch.sparse_csr_tensor(A.crow_indices().to(index_dtype), A.col_indices().to(index_dtype), A.values(), D.shape)
    A = D.to_sparse_csc()
    return torch.sparse_csc_tensor(A.ccol_indices().to(index_dtype), A.row_indices().to(index_dtype), A.values(), D.shape)


def _oracle(D, mask, dim, which, W):
    """Dense float64 (values, gradient for the upstream gradient W) of torch.sparse.<which> on the coalesced COO of every item."""
    ref = FUNCS[which][1]
    items = [D] if D.dim() == 2 else list(D)
    Ws = [W] if D.dim() == 2 else list(W)
    idx = mask.nonzero().t()
    ys, ds = [], []
    for Di, Wi in zip(items, Ws):
        C = torch.sparse_coo_tensor(idx, Di.double()[mask], Di.shape, is_coalesced=True).requires_grad_(True)
        y = ref(C, dim % D.dim() - (D.dim() - 2))
        (d,) = torch.autograd.grad(y, C, torch.sparse_coo_tensor(idx, Wi[mask], Di.shape, is_coalesced=True))
        ys.append(y.detach().to_dense()), ds.append(d.to_dense())
    return (ys[0], ds[0]) if D.dim() == 2 else (torch.stack(ys), torch.stack(ds))


def _stored_order(W, A):
    """The dense W at the stored positions of the sparse A, in A's stored order (the shape of its value array)."""
    if A.layout == torch.sparse_coo:
        return W[tuple(A._indices())]
    csr = A.layout == torch.sparse_csr
    comp, plain = (A.crow_indices(), A.col_indices()) if csr else (A.ccol_indices(), A.row_indices())

    def one(c, p, Wi):
        major = torch.repeat_interleave(torch.arange(c.numel() - 1), (c[1:] - c[:-1]).to(torch.int64))
        return Wi[major, p.to(torch.int64)] if csr else Wi[p.to(torch.int64), major]

    if A.dim() == 2:
        return one(comp, plain, W)
    return torch.stack([one(comp[i], plain[i], W[i]) for i in range(A.size(0))])


def _on_pattern(A, values):
    """A sparse tensor on A's own index tensors."""
    if A.layout == torch.sparse_csr:
        return torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), values, A.shape)
    if A.layout == torch.sparse_csc:
        return torch.sparse_csc_tensor(A.ccol_indices(), A.row_indices(), values, A.shape)
    return torch.sparse_coo_tensor(A._indices(), values, A.shape, is_coalesced=True)


def _grad_with(y, A, W):
    """Gradient of sum(y * W) over the stored entries, W handed over as a sparse gradient on y's pattern.  (torch's own
    to_dense() has no backward for CSC and batched CSR tensors, and `.backward()` cannot accumulate a CSC gradient into a
    leaf's `.grad`: torch.autograd.grad throughout.)"""
    return torch.autograd.grad(y, A, _on_pattern(y, _stored_order(W, y.detach()).to(y.dtype)))[0]


def _close(got, want, rel, scale=None):
    err = (got.double() - want).abs()
    ref = want.abs() if scale is None else scale
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    ok = (err <= rel * ref + 1e-30) | nan | (got.double() == want)
    assert ok.all(), float((err / (ref + 1e-300))[~ok].max())


def _values(A):
    return A._values() if A.layout == torch.sparse_coo else A.values()


LAYOUTS = [("coo", torch.int64), ("coo_uncoalesced", torch.int64), ("csr", torch.int32), ("csr", torch.int64), ("csc", torch.int32),
           ("csc", torch.int64)]


@pytest.mark.parametrize("pattern", ["random", "pairwise"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16], ids=["f32", "f64", "bf16"])
@pytest.mark.parametrize("batch", [None, 3], ids=["2d", "batched"])
@pytest.mark.parametrize("layout,index_dtype", LAYOUTS, ids=[f"{a}-{str(b)[6:]}" for a, b in LAYOUTS])
def test_values_and_gradients_match_the_oracle(layout, index_dtype, batch, dtype, pattern):
    mask = _mask(23, 17, 0.3, 3) if pattern == "random" else _stencil_mask()
    D = _dense_values(mask, batch, 4).to(dtype).double()            # (what the value type holds; the oracle gets exactly this)
    W = torch.randn(D.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(dtype).double()
    bmask = mask.expand(D.shape)
    for dim in (-1, -2, D.dim() - 1):
        for which, (fn, _) in FUNCS.items():
            y64, d64 = _oracle(D, mask, dim, which, W)
            A = _sparse(D, mask, layout, index_dtype, dtype).requires_grad_(True)
            y = fn(A, dim)
            assert y.layout == (torch.sparse_coo if layout.startswith("coo") else A.layout) and y.shape == A.shape and y.dtype == dtype
            yv = _stored_order(y64, y.detach())
            _close(_values(y.detach()), yv, REL[dtype], yv.abs().clamp(min=1.0) if which == "log_softmax" else None)
            g = _grad_with(y, A, W)
            assert g.layout == A.layout
            scale = W.abs() + (W.abs() * bmask).amax((-1, -2), keepdim=True)
            if layout == "coo_uncoalesced":       # (torch's coalesce hands the gradient of the summed entries through as it is)
                _close(g.to_dense()[bmask], d64[bmask], REL_GRAD[dtype], scale.expand(D.shape)[bmask])
            else:
                _close(_values(g), _stored_order(d64, g), REL_GRAD[dtype], _stored_order(scale.expand(D.shape), g))


def test_dtype_casts_the_values_first():
    mask = _mask(9, 8, 0.5, 6)
    D = _dense_values(mask, None, 7)
    A = _sparse(D, mask, "csr", torch.int32, torch.float32).requires_grad_(True)
    y = tsgu.sparse_softmax(A, -1, dtype=torch.float64)
    assert y.dtype == torch.float64
    want = tsgu.sparse_softmax(_sparse(D.float().double(), mask, "csr", torch.int32, torch.float64), -1)
    assert torch.equal(y.values(), want.values())
    (g,) = torch.autograd.grad(y.values().square().sum(), A)
    assert g.dtype == torch.float32 and g.layout == torch.sparse_csr
    assert tsgu.sparse_log_softmax(A, -1, dtype=torch.bfloat16).dtype == torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------------------
# names and errors


def test_names_are_exported():
    assert {"sparse_softmax", "sparse_log_softmax"} <= set(tsgu.__all__)
    assert callable(tsgu.sparse_softmax) and callable(tsgu.sparse_log_softmax)


@pytest.mark.parametrize("name", ["sparse_softmax", "sparse_log_softmax"])
def test_refusals(name):
    fn = getattr(tsgu, name)
    A = torch.eye(3).to_sparse_csr()
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} supports 2-D or batched 3-D sparse tensors, got ndim=1.")):
        fn(torch.ones(3).to_sparse(), 0)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} supports 2-D or batched 3-D sparse tensors, got ndim=4.")):
        fn(torch.ones(2, 2, 2, 2).to_sparse(), 0)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} does not support layout torch.strided.")):
        fn(torch.eye(3), 0)
    with pytest.raises(NotImplementedError, match=re.escape(f"{name} does not support layout torch.sparse_bsr.")):
        fn(torch.eye(4).to_sparse_bsr((2, 2)), 0)
    with pytest.raises(ValueError, match=re.escape(f"{name} requires a sparse tensor with zero dense dimensions.")):
        fn(torch.ones(3, 3, 2).to_sparse(2), 0)
    for bad in (2, -3):
        with pytest.raises(IndexError, match=re.escape(f"Dimension out of range (expected to be in range of [-2, 1], but got {bad})")):
            fn(A, bad)
    B = torch.stack([torch.eye(3), torch.eye(3)]).to_sparse_coo()
    with pytest.raises(IndexError, match=re.escape("Dimension out of range (expected to be in range of [-3, 2], but got 3)")):
        fn(B, 3)
    for batch_dim in (0, -3):
        with pytest.raises(NotImplementedError, match=re.escape("Cannot reduce the batch dimension (0) of a batched 3-D sparse tensor.")):
            fn(B, batch_dim)
    for bad in (torch.float16, torch.int64):
        with pytest.raises(TypeError, match="dtype must be torch.float32, torch.float64 or torch.bfloat16"):
            fn(A, -1, dtype=bad)
    # the messages are sparse_logsumexp's own, under the new names
    with pytest.raises(NotImplementedError) as e:
        tsgu.sparse_logsumexp(torch.ones(3).to_sparse(), 0)
    assert str(e.value).replace("sparse_logsumexp", name) == f"{name} supports 2-D or batched 3-D sparse tensors, got ndim=1."
    with pytest.raises(IndexError) as e:
        tsgu.sparse_logsumexp(A, 2)
    assert str(e.value) == "Dimension out of range (expected to be in range of [-2, 1], but got 2)"


# ---------------------------------------------------------------------------------------------------------------------------
# special values, empty inputs


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
@pytest.mark.parametrize("which", ["softmax", "log_softmax"])
def test_special_values_match_the_oracle(which, layout):
    inf, nan = float("inf"), float("nan")
    rows = [[1.0, nan, 2.0, 0.5], [-inf, -inf, -inf, None], [-inf, 1.0, None, 2.0], [None, None, None, None], [3.0, None, None, None],
            [-inf, None, None, None]]
    mask = torch.tensor([[v is not None for v in r] for r in rows])
    D = torch.tensor([[0.0 if v is None else v for v in r] for r in rows], dtype=torch.float64)
    idx = mask.nonzero().t()
    fn, ref = FUNCS[which]
    for dim in (-1, -2):
        C = torch.sparse_coo_tensor(idx, D[mask], D.shape, is_coalesced=True)
        A = C if layout == "coo" else C.to_sparse_csr() if layout == "csr" else C.to_sparse_csc()
        got = fn(A, dim).to_dense()[mask]
        want = ref(C, dim % 2).to_dense()[mask]
        assert torch.equal(got.isnan(), want.isnan())
        assert torch.allclose(got, want, rtol=1e-14, atol=0, equal_nan=True)
    want_rows = torch.softmax(torch.tensor([-inf, 1.0, 2.0], dtype=torch.float64), 0)
    got = tsgu.sparse_softmax(torch.sparse_coo_tensor(idx, D[mask], D.shape, is_coalesced=True), -1).to_dense()
    assert got[2, 0] == 0 and torch.allclose(got[2, [1, 3]], want_rows[1:], rtol=1e-15) and got[0].isnan().all() and got[1, :3].isnan().all()
    assert tsgu.sparse_log_softmax(torch.sparse_coo_tensor(idx, D[mask], D.shape, is_coalesced=True), -1).to_dense()[2, 0] == -inf


@pytest.mark.parametrize("layout", ["coo", "csr", "csc"])
def test_empty_inputs(layout):
    for shape in ((4, 5), (2, 4, 5), (0, 5), (4, 0)):
        Z = torch.zeros(shape)
        A = (Z.to_sparse_coo() if layout == "coo" else Z.to_sparse_csr() if layout == "csr" else Z.to_sparse_csc()).requires_grad_(True)
        for fn in (tsgu.sparse_softmax, tsgu.sparse_log_softmax):
            for dim in (-1, -2):
                y = fn(A, dim)
                assert y.layout == A.layout and y.shape == A.shape and y._nnz() == 0
                (g,) = torch.autograd.grad(y, A, _on_pattern(y, _values(y.detach())))
                assert g.layout == A.layout and g.shape == A.shape and g._nnz() == 0


# ---------------------------------------------------------------------------------------------------------------------------
# upstream gradient forms, index identity


def _dense_of(A):
    return A.detach().to_dense()


def _index_tensors(A):
    if A.layout == torch.sparse_csr:
        return A.crow_indices(), A.col_indices()
    if A.layout == torch.sparse_csc:
        return A.ccol_indices(), A.row_indices()
    return (A._indices(),)


@pytest.mark.parametrize("which", ["softmax", "log_softmax"])
@pytest.mark.parametrize("layout,index_dtype", [("coo", torch.int64), ("csr", torch.int32), ("csc", torch.int64)])
def test_upstream_gradient_forms(layout, index_dtype, which):
    mask = _mask(12, 10, 0.4, 8)
    D = _dense_values(mask, None, 9)
    W = torch.randn(D.shape, generator=torch.Generator().manual_seed(10), dtype=torch.float64)
    X = torch.randn((10, 3), generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    fn = FUNCS[which][0]
    for dim in (-1, -2):
        def grad_of(loss=None, upstream=None):
            A = _sparse(D, mask, layout, index_dtype, torch.float64).requires_grad_(True)
            y = fn(A, dim)
            g = torch.autograd.grad(loss(y), A)[0] if upstream is None else torch.autograd.grad(y, A, upstream)[0]
            return _dense_of(g)

        order = {"coo": lambda M: M[mask], "csr": lambda M: M[mask], "csc": lambda M: M.t()[mask.t()]}[layout]
        # .values(): the stored order of the layout
        _, d64 = _oracle(D, mask, dim, which, W)
        _close(grad_of(lambda y: ((y.values() if layout != "coo" else y.coalesce().values()) * order(W)).sum())[mask], d64[mask], 1e-12,
               W.abs().max().expand(int(mask.sum())))
        # .to_dense()
        _close(grad_of(lambda y: (y.to_dense() * W).sum())[mask], d64[mask], 1e-12, W.abs().max().expand(int(mask.sum())))
        # torch.sparse.mm(y, X): upstream gradient G Xᵀ on the pattern, G = W[:, :3]
        G = W[:, :3]
        _, dmm = _oracle(D, mask, dim, which, (G @ X.t()) * mask)
        if layout != "csc":                   # (torch.sparse.mm takes COO and CSR operands)
            _close(grad_of(lambda y: (torch.sparse.mm(y, X) * G).sum())[mask], dmm[mask], 1e-12, (G @ X.t()).abs().max().expand(int(mask.sum())))
        # a strided gradient handed to backward: gathered at the stored positions
        _close(grad_of(upstream=W)[mask], d64[mask], 1e-12, W.abs().max().expand(int(mask.sum())))
        # a sparse gradient on another pattern: masked, never densified
        other = _mask(12, 10, 0.5, 12)
        Wo = (W * other).to_sparse_coo()
        Go = Wo if layout == "coo" else Wo.to_sparse_csr() if layout == "csr" else Wo.to_sparse_csc()
        _, dother = _oracle(D, mask, dim, which, W * other)
        _close(grad_of(upstream=Go)[mask], dother[mask], 1e-12, W.abs().max().expand(int(mask.sum())))


def test_a_sparse_gradient_is_never_densified(monkeypatch):
    mask = _mask(12, 10, 0.4, 8)
    A = _sparse(_dense_values(mask, None, 9), mask, "csr", torch.int32, torch.float64).requires_grad_(True)
    other = (torch.rand(12, 10, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * _mask(12, 10, 0.5, 12)).to_sparse_csr()
    y = tsgu.sparse_softmax(A, -1)

    def refuse(self, *a, **k):
        raise AssertionError("to_dense called in backward")

    monkeypatch.setattr(torch.Tensor, "to_dense", refuse)
    torch.autograd.grad(y, A, other)
    y2 = tsgu.sparse_softmax(A, -1)
    torch.autograd.grad(y2, A, torch.sparse_csr_tensor(y2.crow_indices(), y2.col_indices(), torch.ones_like(y2.values()), y2.shape))


@pytest.mark.parametrize("layout,index_dtype", LAYOUTS, ids=[f"{a}-{str(b)[6:]}" for a, b in LAYOUTS])
@pytest.mark.parametrize("batch", [None, 2], ids=["2d", "batched"])
def test_output_and_gradient_carry_the_inputs_index_tensors(layout, index_dtype, batch):
    mask = _mask(9, 8, 0.5, 13)
    A = _sparse(_dense_values(mask, batch, 14), mask, layout, index_dtype, torch.float32).requires_grad_(True)
    mine = _index_tensors(A.detach().coalesce() if layout == "coo_uncoalesced" else A)
    for fn in (tsgu.sparse_softmax, tsgu.sparse_log_softmax):
        for dim in (-1, -2):
            _pattern.clear_cache()
            src = A
            if layout == "coo_uncoalesced":
                src = A.coalesce()               # (the function coalesces such an input itself: its indices are new by necessity)
                mine = _index_tensors(src)
            y = fn(src, dim)
            (g,) = torch.autograd.grad(y, src, _on_pattern(y, torch.ones_like(_values(y.detach()))))
            for out in (y, g):
                assert out.layout == src.layout and out.shape == src.shape
                for a, b in zip(mine, _index_tensors(out)):
                    assert a.data_ptr() == b.data_ptr() and a.dtype == b.dtype == index_dtype and a.shape == b.shape
    y = tsgu.sparse_softmax(A, -1)
    assert y.layout == torch.sparse_coo if layout.startswith("coo") else y.layout == A.layout


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI: the second header


def test_range_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "torchsparsegradutils_amd", "csrc", "logsumexp_impl.h")).read()
    assert int(re.search(r"kLseStageBytes\s*=\s*(\d+)", src).group(1)) == _backend.SOFTMAX_STAGE_BYTES
    assert _backend.segment_softmax_range(torch.float32) == _backend.segment_softmax_range(torch.bfloat16) == 2048
    assert _backend.segment_softmax_range(torch.float64) == 1024


FAKE = 0x7F0000001000          # a 16-byte aligned address that is never dereferenced: every call below is refused on the host


def _forward(lib, **kw):
    a = dict(vtype=0, itype=0, n_groups=4, nnz=5000, ptr=FAKE, perm=None, val=FAKE + 0x100000, log_form=0, out=FAKE + 0x200000,
             workspace=FAKE + 0x300000, workspace_bytes=1 << 20, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_segment_softmax(*a.values())


def _backward(lib, **kw):
    a = dict(vtype=0, itype=0, n_groups=4, nnz=5000, ptr=FAKE, perm=None, y=FAKE + 0x100000, g=FAKE + 0x400000, log_form=0,
             gin=FAKE + 0x200000, workspace=FAKE + 0x300000, workspace_bytes=1 << 20, device=-1, stream=None)
    a.update(kw)
    return lib.tsgu_segment_softmax_backward(*a.values())


@pytest.mark.parametrize("call,operands", [(_forward, ("ptr", "val", "out")), (_backward, ("ptr", "y", "g", "gin"))], ids=["forward", "backward"])
def test_launcher_refusals_on_the_host(call, operands):
    lib = _backend.load_library()
    need = ctypes.c_int64(0)
    assert lib.tsgu_segment_softmax_workspace(0, 5000, ctypes.byref(need)) == OK and need.value == 3 * (4 * 4 + 8)
    # the base call passes every check but the device's: device = -1 is refused by set_device, before any HIP call
    assert call(lib) == BAD_ARG
    assert call(lib, workspace=None, workspace_bytes=0) == BAD_ARG          # (the no-crossing form reaches set_device too)
    for vt in (3, -1):
        assert call(lib, vtype=vt) == BAD_DTYPE
    for it in (2, -1):
        assert call(lib, itype=it) == BAD_DTYPE
    for name in operands:
        assert call(lib, **{name: None}) == BAD_ARG, name
    assert call(lib, n_groups=-1) == BAD_ARG and call(lib, nnz=-1) == BAD_ARG and call(lib, workspace_bytes=-1) == BAD_ARG
    assert call(lib, workspace_bytes=need.value - 1) == BAD_ARG
    assert call(lib, workspace=FAKE + 0x300008) == BAD_ARG                  # misaligned
    assert call(lib, workspace=None) == BAD_ARG                             # bytes without a workspace
    assert call(lib, nnz=1 << 62, workspace_bytes=1 << 62) == TOO_LARGE
    # nothing to do: no group or no entry is not an error (and touches no device)
    assert call(lib, n_groups=0) == OK and call(lib, nnz=0) == OK
    # the refusals do not depend on the device either
    assert call(lib, device=0, vtype=7) == BAD_DTYPE and call(lib, device=0, ptr=None) == BAD_ARG


def test_workspace_query_refusals():
    lib = _backend.load_library()
    out = ctypes.c_int64(-5)
    assert lib.tsgu_segment_softmax_workspace(0, -1, ctypes.byref(out)) == BAD_ARG
    assert lib.tsgu_segment_softmax_workspace(0, 10, None) == BAD_ARG
    assert lib.tsgu_segment_softmax_workspace(5, 10, ctypes.byref(out)) == BAD_DTYPE
    for vt, acc in ((0, 4), (1, 8), (2, 4)):
        assert lib.tsgu_segment_softmax_workspace(vt, 0, ctypes.byref(out)) == OK and out.value == 4 * acc + 8
        n = 5 * (8192 // acc) + 1
        assert lib.tsgu_segment_softmax_workspace(vt, n, ctypes.byref(out)) == OK and out.value == 6 * (4 * acc + 8)
