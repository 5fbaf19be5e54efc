"""sparse_gat_attention / sparse_gatv2_attention without a GPU: the torch-op path of _cpu.py against the dense float64 oracle
(tests/_gat_ref.py), the refusals, and the geometry query of include/tsgu_hip_gat.h.

float64 comparisons at rtol 1e-12: both sides sum at most 19 terms of magnitude O(10) on a grid of 1/32.
"""

import pytest
import torch

import _abi_cases as A
import _gat_ref as gr
from torchsparsegradutils_amd import _backend, sparse_gat_attention, sparse_gatv2_attention

N, M = 23, 19
FN = {"gat": sparse_gat_attention, "gatv2": sparse_gatv2_attention}


def _operands(kind, heads, d, batch=None, seed=3):
    """(mask, B, a, b, c, dO) on the 1/32 grid; heads = 0: the single-head form without the head axis."""
    gen = torch.Generator().manual_seed(seed)
    mask = torch.rand((N, M), generator=gen) < 0.3
    mask[4] = False
    mask[:, 6] = False
    lead, hs = (() if batch is None else (batch,)), ((heads,) if heads else ())
    if kind == "gat":
        shapes = (lead + (N,) + hs, lead + (M,) + hs, lead + (M,) + hs + (d,))
    else:
        shapes = (lead + (N,) + hs + (d,), lead + (M,) + hs + (d,), hs + (d,))
    B, a, b, c, dO = (gr.grid(s, gen) for s in ((lead + (N, M),) + shapes + (lead + (N,) + hs + (d,),)))
    return mask, B, a, b, c, dO


def _oracle(kind, mask, B, a, b, c, dO, slope, use_bias, heads, batched):
    """dense_oracle over the items of a batch ("gatv2": att shared, its gradient summed), results stacked."""
    view = (lambda x, rows: x if heads else x.unsqueeze(rows))           # rows: where the head axis goes
    items = range(B.size(0)) if batched else [None]
    pick = (lambda x, i: x if i is None else x[i])
    res = []
    for i in items:
        ai, bi = view(pick(a, i), 1), view(pick(b, i), 1)
        ci = view(pick(c, i), 1) if kind == "gat" else view(c, 0)
        res.append(gr.dense_oracle(kind, mask, pick(B, i), ai, bi, ci, view(pick(dO, i), 1), slope, use_bias))
    out = {k: torch.stack([r[k] for r in res]) if batched else res[0][k] for k in ("O", "da", "db", "dc", "dB")}
    if kind == "gatv2" and batched:
        out["dc"] = out["dc"].sum(0)
    return out


@pytest.mark.parametrize("kind", gr.KINDS)
@pytest.mark.parametrize("layout,heads,batch,slope", [("csr", 3, None, 0.2), ("csc", 0, None, 0.25), ("coo_uncoalesced", 2, None, 0.0),
                                                      ("csr", 2, 2, 0.2), ("coo", 1, 3, 0.25)])
def test_the_torch_op_path_against_the_dense_oracle(kind, layout, heads, batch, slope):
    d = 5
    mask, B, a, b, c, dO = _operands(kind, heads, d, batch)
    ref = _oracle(kind, mask, B, a, b, c, dO, slope, True, heads, batch is not None)
    S = gr.sparse_from_dense(B, mask, layout, torch.int32 if layout in ("csr", "csc") else torch.int64, torch.float64).requires_grad_(True)
    xa, xb, xc = (x.clone().requires_grad_(True) for x in (a, b, c))
    O = FN[kind](S, xa, xb, xc, negative_slope=slope)
    assert O.shape == dO.shape
    gS, ga, gb, gc = torch.autograd.grad(O, (S, xa, xb, xc), dO)
    assert gS.layout == S.layout and (layout == "coo_uncoalesced" or gr.values_of(gS).shape == gr.values_of(S).shape)
    want_dB = gr.stored_order(ref["dB"], S.detach().coalesce() if layout == "coo_uncoalesced" else S.detach())
    got_dB = gr.values_of(gS.coalesce()) if layout == "coo_uncoalesced" else gr.values_of(gS)
    for name, got, want in (("O", O, ref["O"]), ("da", ga, ref["da"]), ("db", gb, ref["db"]), ("dc", gc, ref["dc"]),
                            ("dB", got_dB, want_dB)):
        torch.testing.assert_close(got.detach().reshape(want.shape), want, rtol=1e-12, atol=1e-12, msg=lambda s, n=name: f"{n}: {s}")
    # values_as_bias=False: the values are not read and A gets no gradient
    S2 = gr.sparse_from_dense(B * float("nan"), mask, "csr" if batch is None else layout.replace("_uncoalesced", ""), torch.int64,
                              torch.float64).requires_grad_(True)
    ref0 = _oracle(kind, mask, B, a, b, c, dO, slope, False, heads, batch is not None)
    O0 = FN[kind](S2, xa, xb, xc, negative_slope=slope, values_as_bias=False)
    O0.backward(dO)
    assert S2.grad is None
    torch.testing.assert_close(O0.detach().reshape(ref0["O"].shape), ref0["O"], rtol=1e-12, atol=1e-12)


def test_refusals():
    mask, B, a, b, c, _ = _operands("gat", 2, 4)
    S = gr.sparse_from_dense(B, mask, "csr", torch.int64, torch.float32)
    a, b, c = a.float(), b.float(), c.float()
    with pytest.raises(ValueError, match=r"sparse_gat_attention: s_dst must be \[n\] or \[n, H\], got \(23, 2, 1\)"):
        sparse_gat_attention(S, a[..., None], b, c)
    with pytest.raises(ValueError, match=r"sparse_gat_attention: s_src must be \(19, 2\) for A of shape \(23, 19\)"):
        sparse_gat_attention(S, a, b[:-1], c)
    with pytest.raises(ValueError, match=r"sparse_gat_attention: V must be \(19, 2, 4\)"):
        sparse_gat_attention(S, a, b, c[:, :1])
    with pytest.raises(TypeError, match=r"sparse_gat_attention: A, s_dst, s_src, V must have one dtype, got torch.float32 for A and torch.float64 for V"):
        sparse_gat_attention(S, a, b, c.double())
    with pytest.raises(TypeError, match=r"sparse_gat_attention: values must be float32, float64 or bfloat16"):
        sparse_gat_attention(S.to(torch.float16), a.half(), b.half(), c.half())
    with pytest.raises(ValueError, match=r"sparse_gat_attention: negative_slope must be a finite number, got inf"):
        sparse_gat_attention(S, a, b, c, negative_slope=float("inf"))
    with pytest.raises(ValueError, match=r"sparse_gat_attention: negative_slope must be a finite number, got True"):
        sparse_gat_attention(S, a, b, c, negative_slope=True)
    with pytest.raises(TypeError, match=r"sparse_gat_attention: V must be a dense tensor"):
        sparse_gat_attention(S, a, b, c.to_sparse())
    xd, xs, att = c[:4].new_zeros((23, 2, 4)), c, c[0]
    with pytest.raises(ValueError, match=r"sparse_gatv2_attention: X_dst must be \[n, d\] or \[n, H, d\], got \(23,\)"):
        sparse_gatv2_attention(S, xd[:, 0, 0], xs, att)
    with pytest.raises(ValueError, match=r"sparse_gatv2_attention: att must be \(2, 4\)"):
        sparse_gatv2_attention(S, xd, xs, att[:1])
    with pytest.raises(ValueError, match=r"sparse_gatv2_attention: X_src must be \(19, 2, 4\)"):
        sparse_gatv2_attention(S, xd, xs[:, :, :3], att)
    # the GPU limits are told by the host-only query the public functions ask
    assert _backend.gat_supported(torch.float32, 128, 8) and _backend.gat_supported(torch.bfloat16, 8, 128)
    assert not _backend.gat_supported(torch.float32, 2, 5) and not _backend.gat_supported(torch.float32, 9, 128)
    assert not _backend.gat_supported(torch.float16, 1, 8)


def test_geometry():
    lib = _backend.load_library()
    # the geometry the GPU tests size their cases from: the stage shrinks with the heads of a tile, to 128 (fp64: 128) at H = 128
    assert _backend.gat_geometry(torch.float32, "gat", 1, 64) == (4, 1024, 64)
    assert _backend.gat_geometry(torch.float32, "gat", 128, 8) == (4, 128, 256)
    assert _backend.gat_geometry(torch.float64, "gat", 128, 8) == (4, 128, 128)
    assert _backend.gat_geometry(torch.float32, "gatv2", 128, 8) == (4, 1024, 256)
    assert lib.tsgu_gat_geometry(9, 0, 1, 8, None, None, None) == A.BAD_DTYPE and lib.tsgu_gat_geometry(0, 2, 1, 8, None, None, None) == A.BAD_ARG
