"""Which kernel family every sparse product launches, step by step (GPU).

`_ops` walks lattice -> row-block tiles -> row pairs -> plan-free for the forward, the transposed forward, the SDDMM and the fused
backward.  Each case below runs a few sparse_mm steps through autograd and records, per step, the `_be` launches of the forward and
of the backward, which plans exist afterwards (and how often the pattern has been counted), and the notes that
sparse_matmul._settle_step_plan reads.  The tables pin the first-sight -> plan switch, the volatile wait, the per-product differences
and the hand-over to the C++ host path (a settled step launches nothing through `_be`)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

LAUNCHES = ("csr_spmm", "csr_sddmm", "csr_mm_backward", "csr_spmm_tile", "csr_sddmm_tile", "csr_spmm_rowpack", "csr_sddmm_rowpack",
            "csr_mm_backward_rowpack", "csr_spmm_lattice", "csr_sddmm_lattice", "coo_sddmm")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from torchsparsegradutils_amd import _backend

    _backend.load_library()
    yield


def _pattern_of(name):
    from torchsparsegradutils_amd.utils import synthetic as sy

    if name == "periodic":
        return sy.box_stencil(16, 16, 16, (True, True, True), 27, None, torch.int32, DEV)
    if name == "truncated":
        return sy.box_stencil(16, 16, 16, (False, False, False), 27, None, torch.int32, DEV)
    if name == "lower":
        return sy.box_stencil(16, 16, 32, (False, False, False), 27, "lower", torch.int32, DEV)
    if name == "mesh":
        return sy.mesh27_blocked(16, 16, 16, 4, torch.int32, DEV)
    if name == "mesh_wide":           # (enough workgroups for the transposed row-pair plan's dictionary form: srcstart)
        return sy.mesh27_blocked(24, 20, 16, 4, torch.int32, DEV)
    if name == "banded":
        return sy.banded_random(8192, 25, 16, torch.int32, DEV)
    if name == "random":
        return sy.rand_csr(4096, 4096, 100_000, torch.int32, DEV)
    if name == "small":
        return sy.stencil27_periodic(8, 8, 8, torch.int32, DEV)
    raise KeyError(name)


def _operand(name, layout, dtype, batch=2):
    """(A without requires_grad, n): `layout` csr / coo / coo_unc (shuffled, not coalesced) / bcsr / bcoo."""
    crow, col = _pattern_of(name)
    n, nnz = crow.numel() - 1, col.numel()
    g = torch.Generator(device=DEV).manual_seed(3)
    if layout in ("csr", "coo", "coo_unc"):
        val = torch.randn(nnz, device=DEV, generator=g).to(dtype)
        A = torch.sparse_csr_tensor(crow, col, val, (n, n))
        if layout == "coo":
            A = A.to_sparse_coo().coalesce()
        elif layout == "coo_unc":
            C = A.to_sparse_coo().coalesce()
            order = torch.randperm(nnz, device=DEV, generator=g)
            A = torch.sparse_coo_tensor(C.indices()[:, order], C.values()[order], (n, n))
            assert not A.is_coalesced()
        return A, n
    val = torch.randn(batch, nnz, device=DEV, generator=g).to(dtype)
    A = torch.sparse_csr_tensor(crow.expand(batch, -1).contiguous(), col.expand(batch, -1).contiguous(), val, (batch, n, n))
    if layout == "bcoo":
        A = torch.stack([A[i].to_sparse_coo() for i in range(batch)]).coalesce()
    return A, n


# (id, pattern, layout, dtype, p, gradients, options); options: steps, lattice / tile / pack switches, async, tview (B a transposed
# view), volatile (the geometry has been seen with three other contents first)
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
CASES = [
    ("periodic-f32-32", "periodic", "csr", F32, 32, "AB", {}),
    ("periodic-f32-128", "periodic", "csr", F32, 128, "AB", {}),
    ("periodic-bf16-16", "periodic", "csr", BF16, 16, "AB", {}),
    ("periodic-f64-16", "periodic", "csr", F64, 16, "AB", {}),
    ("periodic-f32-4", "periodic", "csr", F32, 4, "AB", {}),
    ("periodic-f32-16", "periodic", "csr", F32, 16, "AB", {}),
    ("periodic-bf16-8", "periodic", "csr", BF16, 8, "AB", {}),
    ("periodic-f32-6", "periodic", "csr", F32, 6, "AB", {}),
    ("periodic-f32-32-async", "periodic", "csr", F32, 32, "AB", {"async": True}),
    ("periodic-bcsr-f32-32", "periodic", "bcsr", F32, 32, "AB", {}),
    ("periodic-bcoo-f32-32", "periodic", "bcoo", F32, 32, "AB", {}),
    ("periodic-f32-32-nolattice", "periodic", "csr", F32, 32, "AB", {"lattice": False}),
    ("periodic-f32-32-nolattice-notile", "periodic", "csr", F32, 32, "AB", {"lattice": False, "tile": False}),
    ("periodic-f32-32-nothing", "periodic", "csr", F32, 32, "AB", {"lattice": False, "tile": False, "pack": False}),
    ("periodic-bcsr-f32-16-nolattice", "periodic", "bcsr", F32, 16, "AB", {"lattice": False}),
    ("periodic-f32-32-volatile", "periodic", "csr", F32, 32, "AB", {"volatile": True, "steps": 9}),
    ("periodic-f64-16-volatile", "periodic", "csr", F64, 16, "AB", {"volatile": True, "steps": 9}),
    ("truncated-f32-32", "truncated", "csr", F32, 32, "AB", {}),
    ("truncated-coo-f32-32", "truncated", "coo", F32, 32, "AB", {}),
    ("truncated-coo_unc-f32-32", "truncated", "coo_unc", F32, 32, "AB", {}),
    ("truncated-f32-32-A", "truncated", "csr", F32, 32, "A", {}),
    ("truncated-f32-32-B", "truncated", "csr", F32, 32, "B", {}),
    ("truncated-f64-32", "truncated", "csr", F64, 32, "AB", {}),
    ("truncated-bf16-32", "truncated", "csr", BF16, 32, "AB", {}),
    ("truncated-f32-32-tview", "truncated", "csr", F32, 32, "AB", {"tview": True}),
    ("truncated-bcsr-f32-32", "truncated", "bcsr", F32, 32, "AB", {}),
    ("lower-f32-32", "lower", "csr", F32, 32, "AB", {}),
    ("lower-f32-32-B", "lower", "csr", F32, 32, "B", {}),
    ("mesh-f32-32", "mesh", "csr", F32, 32, "AB", {}),
    ("mesh-f32-32-A", "mesh", "csr", F32, 32, "A", {}),
    ("mesh-f32-32-B", "mesh", "csr", F32, 32, "B", {}),
    ("mesh-f32-16", "mesh", "csr", F32, 16, "AB", {}),
    ("mesh-f32-32-notile", "mesh", "csr", F32, 32, "AB", {"tile": False}),
    ("mesh-f32-32-async", "mesh", "csr", F32, 32, "AB", {"async": True}),
    ("mesh-f32-32-tview", "mesh", "csr", F32, 32, "AB", {"tview": True}),
    ("mesh-f64-32", "mesh", "csr", F64, 32, "AB", {}),
    ("mesh-coo-f32-32", "mesh", "coo", F32, 32, "AB", {}),
    ("mesh-coo_unc-f32-32", "mesh", "coo_unc", F32, 32, "AB", {}),
    ("mesh-coo_unc-f32-32-A", "mesh", "coo_unc", F32, 32, "A", {}),
    ("mesh-bcsr-f32-32", "mesh", "bcsr", F32, 32, "AB", {}),
    ("mesh-bcsr-f32-32-B", "mesh", "bcsr", F32, 32, "B", {}),
    ("mesh-bcsr-f32-16", "mesh", "bcsr", F32, 16, "AB", {}),
    ("mesh-bcoo-f32-32", "mesh", "bcoo", F32, 32, "AB", {}),
    ("mesh_wide-f32-32-notile", "mesh_wide", "csr", F32, 32, "AB", {"tile": False}),
    ("mesh_wide-f32-16", "mesh_wide", "csr", F32, 16, "AB", {}),
    ("mesh_wide-f32-32-notile-volatile", "mesh_wide", "csr", F32, 32, "AB", {"tile": False, "volatile": True, "steps": 7}),
    ("banded-f32-32", "banded", "csr", F32, 32, "AB", {}),
    ("banded-f32-16", "banded", "csr", F32, 16, "AB", {}),
    ("banded-f32-16-B", "banded", "csr", F32, 16, "B", {}),
    ("banded-f32-16-async", "banded", "csr", F32, 16, "AB", {"async": True}),
    ("banded-bf16-64", "banded", "csr", BF16, 64, "AB", {}),
    ("banded-bf16-64-A", "banded", "csr", BF16, 64, "A", {}),
    ("banded-bf16-64-B", "banded", "csr", BF16, 64, "B", {}),
    ("banded-bf16-16", "banded", "csr", BF16, 16, "AB", {}),
    ("banded-f32-8-A", "banded", "csr", F32, 8, "A", {}),
    ("random-f32-32", "random", "csr", F32, 32, "AB", {}),
    ("random-bcsr-f32-32", "random", "bcsr", F32, 32, "AB", {}),
    ("small-f32-32", "small", "csr", F32, 32, "AB", {}),
]


def _kind(obj, names):
    """Type of a noted payload object + its first-seen number in the case (pins which payloads are the very same objects)."""
    key = id(obj)
    if key not in names:
        names[key] = (len(names), obj)
    return f"{type(obj).__name__}#{names[key][0]}"


def _core_state(tag, core):
    def key_str(k):
        return ".".join(key_str(x) if isinstance(x, tuple) else str(x) for x in k)

    parts = [f"{tag} u{core.uses}"]
    for k, v in core.packs.items():
        parts.append(key_str(k) + ("=-" if v is None else "=+"))
    for k in core.pending:
        if k not in core.packs:
            parts.append(key_str(k) + "=~")
    for k in ("lattice", "lattice_t"):
        if k in core.own:
            parts.append(k + ("=-" if core.own[k] is None else "=+"))
    if "volatile" in core.own:
        parts.append(f"volatile={core.own['volatile']}")
    return " ".join(parts)


def _state(plan, names):
    from torchsparsegradutils_amd import _ops

    out = [_core_state("P", plan.core)]
    if plan.core.t is not None:
        out.append(_core_state("T", plan.core.t.core))
    flat = plan.core.flat
    if flat is not None:
        out.append(_core_state("F", flat.core))
        if flat.core.t is not None:
            out.append(_core_state("FT", flat.core.t.core))
    for product in ("fwd", "bwd"):
        got = _ops.launched(plan, product)
        if got is not None:
            out.append(f"{product}={got[0]}*{got[2]}(" + ",".join(_kind(x, names) for x in got[1]) + ")")
    return " | ".join(out)


def _launch_name(name, args):
    if name.endswith("_lattice"):
        lp, cfg = args[0], args[1]
        return name[4:] + ("/march" if getattr(cfg, "march", False) else f"/k{lp.kind}")
    return name[4:] if name.startswith("csr_") else name


def family_table(case, monkeypatch):
    """[one line per step]: the forward's and the backward's `_be` launches, then the plans and notes after the step."""
    from torchsparsegradutils_amd import _backend as be
    from torchsparsegradutils_amd import _lattice, _ops, _pattern, sparse_matmul as sm, sparse_mm, wait_for_plans

    _id, name, layout, dtype, p, grads, opt = case
    log = []
    for fn in LAUNCHES:
        orig = getattr(be, fn)

        def wrapped(*args, _orig=orig, _fn=fn, **kw):
            log.append(_launch_name(_fn, args))
            return _orig(*args, **kw)

        monkeypatch.setattr(be, fn, wrapped)
    monkeypatch.setattr(_lattice, "TUNE", False)
    monkeypatch.setattr(_ops, "PLAN_ASYNC", bool(opt.get("async", False)))
    monkeypatch.setattr(_ops, "ENABLE_LATTICE", opt.get("lattice", True))
    monkeypatch.setattr(_ops, "ENABLE_TILE", opt.get("tile", True))
    monkeypatch.setattr(_ops, "ENABLE_PACK", opt.get("pack", True))
    _pattern.clear_cache()

    A, n = _operand(name, layout, dtype)
    keep = []
    if opt.get("volatile"):
        # three other contents of the same geometry first (row 0 takes another row's columns): the fourth is marked volatile
        crow, col = A.crow_indices(), A.col_indices()
        w = int(crow[1] - crow[0])
        same = torch.nonzero(crow.diff() == w).flatten().tolist()[1:4]
        for r in same:
            c2 = col.clone()
            c2[:w] = col[int(crow[r]):int(crow[r]) + w]
            other = torch.sparse_csr_tensor(crow.clone(), c2, A.values(), A.shape)
            _pattern.from_csr(other)
            keep.append(other)
        A = torch.sparse_csr_tensor(crow.clone(), col.clone(), A.values(), A.shape)
    batched = A.dim() == 3
    g = torch.Generator(device=DEV).manual_seed(4)
    bshape = (A.size(0), n, p) if batched else (n, p)
    B = torch.randn(bshape, device=DEV, generator=g).to(dtype)
    if opt.get("tview"):
        B = B.t().contiguous()          # (the leaf; the operand is its transposed view)
    G = torch.randn(bshape, device=DEV, generator=g).to(dtype)
    A = A.requires_grad_("A" in grads)
    B = B.requires_grad_("B" in grads)
    inputs = tuple(t for t, k in ((A, "A"), (B, "B")) if k in grads)
    if opt.get("tview"):
        B = B.t()
    plan = sm._Operand(A.detach()).plan
    names, rows = {}, []
    for _ in range(opt.get("steps", 5)):
        del log[:]
        C = sparse_mm(A, B)
        fwd = " ".join(log)
        del log[:]
        torch.autograd.grad(C, inputs, G)
        bwd = " ".join(log)
        if opt.get("async"):
            wait_for_plans()
        rows.append(f"F[{fwd}] B[{bwd}] | " + _state(plan, names))
    torch.cuda.synchronize()
    _pattern.clear_cache()
    return rows


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_family_choice_table(case, monkeypatch):
    assert family_table(case, monkeypatch) == EXPECTED[case[0]]


EXPECTED = {  # case id -> one line per step (see family_table)
    'periodic-f32-32': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-f32-128': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*3(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*3(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*4(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*4(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*5(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*5(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-bf16-16': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-f64-16': [
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
    ],
    'periodic-f32-4': [
        'F[spmm_lattice/k0] B[mm_backward]'
        ' | P u0 lattice=+'
        ' | T u0'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=plan-free*1(RowGather#2)',
        'F[spmm_lattice/k0] B[mm_backward]'
        ' | P u0 lattice=+'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=plan-free*2(RowGather#2)',
        'F[spmm_lattice/k0] B[mm_backward]'
        ' | P u0 lattice=+'
        ' | T u0'
        ' | fwd=lattice*3(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=plan-free*3(RowGather#2)',
        'F[spmm_lattice/k0] B[mm_backward]'
        ' | P u0 lattice=+'
        ' | T u0'
        ' | fwd=lattice*4(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=plan-free*4(RowGather#2)',
        'F[spmm_lattice/k0] B[mm_backward]'
        ' | P u0 lattice=+'
        ' | T u0'
        ' | fwd=lattice*5(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=plan-free*5(RowGather#2)',
    ],
    'periodic-f32-16': [
        'F[spmm_lattice/k0] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/k0] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-bf16-8': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'periodic-f32-6': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'periodic-f32-32-async': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-bcsr-f32-32': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0'
        ' | F u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0'
        ' | F u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-bcoo-f32-32': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*3(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*3(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*4(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*4(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*5(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*5(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'periodic-f32-32-nolattice': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u6 64.2048.3072.65536.False.2=+ tile.64.224.1792=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*2(RowPackPlan#0)'
        ' | bwd=row pairs*2(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*3(RowPackPlan#0)'
        ' | bwd=row pairs*3(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u12 64.2048.3072.65536.False.2=+ tile.64.224.1792=-'
        ' | T u8 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*4(RowPackPlan#0)'
        ' | bwd=row pairs*4(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u15 64.2048.3072.65536.False.2=+ tile.64.224.1792=-'
        ' | T u10 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*5(RowPackPlan#0)'
        ' | bwd=row pairs*5(RowPackPlan#1)',
    ],
    'periodic-f32-32-nolattice-notile': [
        'F[spmm] B[mm_backward]'
        ' | P u1'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.False.2=+'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'periodic-f32-32-nothing': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'periodic-bcsr-f32-16-nolattice': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u1'
        ' | FT u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u2 64.2048.3072.65536.True.2=+'
        ' | FT u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u3 64.2048.3072.65536.True.2=+'
        ' | FT u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u4 64.2048.3072.65536.True.2=+'
        ' | FT u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u5 64.2048.3072.65536.True.2=+'
        ' | FT u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'periodic-f32-32-volatile': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=- volatile=2'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u6 64.2048.3072.65536.False.2=+ tile.64.224.1792=- volatile=4'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*2(RowPackPlan#0)'
        ' | bwd=row pairs*2(RowPackPlan#1)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=row pairs*3(RowPackPlan#0)'
        ' | bwd=row pairs*3(RowPackPlan#1)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*1(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*1(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*2(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*2(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
        'F[] B[]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*2(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*2(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
        'F[] B[]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*2(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*2(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
        'F[] B[]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*2(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*2(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
        'F[] B[]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=- lattice=+ volatile=6'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=lattice*2(LatticePlan#2,MarchConfig#3)'
        ' | bwd=lattice*2(LatticePlan#2,MarchConfig#4,LatticePlan#2,MarchConfig#5)',
    ],
    'periodic-f64-16-volatile': [
        'F[spmm] B[sddmm spmm]'
        ' | P u0 volatile=4'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[sddmm spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*1(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*1(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+ volatile=6'
        ' | T u0'
        ' | fwd=lattice*2(LatticePlan#1,LatticeConfig#2)'
        ' | bwd=lattice*2(LatticePlan#1,LatticeConfig#3,LatticePlan#4,LatticeConfig#5)',
    ],
    'truncated-f32-32': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'truncated-coo-f32-32': [
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[spmm_lattice/march] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
        'F[] B[]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#0,MarchConfig#3)',
    ],
    'truncated-coo_unc-f32-32': [
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=plan-free*1()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*2()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u6 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*3()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u8 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*4()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u10 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u10 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*5()',
    ],
    'truncated-f32-32-A': [
        'F[spmm_lattice/march] B[sddmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[sddmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[sddmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*3(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[sddmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*4(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[sddmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*5(LatticePlan#0,MarchConfig#1)',
    ],
    'truncated-f32-32-B': [
        'F[spmm_lattice/march] B[spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*1(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*2(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*3(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*4(LatticePlan#0,MarchConfig#1)',
        'F[spmm_lattice/march] B[spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=lattice*5(LatticePlan#0,MarchConfig#1)',
    ],
    'truncated-f64-32': [
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
    ],
    'truncated-bf16-32': [
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
    ],
    'truncated-f32-32-tview': [
        'F[spmm] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=plan-free*1()'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#1,LatticePlan#0,MarchConfig#2)',
        'F[spmm] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=plan-free*2()'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#1,LatticePlan#0,MarchConfig#2)',
        'F[spmm] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=plan-free*3()'
        ' | bwd=lattice*3(LatticePlan#0,MarchConfig#1,LatticePlan#0,MarchConfig#2)',
        'F[spmm] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=plan-free*4()'
        ' | bwd=lattice*4(LatticePlan#0,MarchConfig#1,LatticePlan#0,MarchConfig#2)',
        'F[spmm] B[sddmm_lattice/march spmm_lattice/march]'
        ' | P u0 lattice=+'
        ' | fwd=plan-free*5()'
        ' | bwd=lattice*5(LatticePlan#0,MarchConfig#1,LatticePlan#0,MarchConfig#2)',
    ],
    'truncated-bcsr-f32-32': [
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0'
        ' | F u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[spmm_lattice/k0] B[sddmm_lattice/k0 spmm_lattice/k1]'
        ' | P u0'
        ' | F u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0'
        ' | F u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,LatticeConfig#2,LatticePlan#3,LatticeConfig#4)',
    ],
    'lower-f32-32': [
        'F[spmm_lattice/k0] B[sddmm_lattice/march spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*1(LatticePlan#0,MarchConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[spmm_lattice/k0] B[sddmm_lattice/march spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#3,LatticeConfig#4)',
        'F[] B[]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)'
        ' | bwd=lattice*2(LatticePlan#0,MarchConfig#2,LatticePlan#3,LatticeConfig#4)',
    ],
    'lower-f32-32-B': [
        'F[spmm_lattice/k0] B[spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*1(LatticePlan#0,LatticeConfig#1)',
        'F[spmm_lattice/k0] B[spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*2(LatticePlan#0,LatticeConfig#1)',
        'F[spmm_lattice/k0] B[spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*3(LatticePlan#0,LatticeConfig#1)',
        'F[spmm_lattice/k0] B[spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*4(LatticePlan#0,LatticeConfig#1)',
        'F[spmm_lattice/k0] B[spmm_lattice/k1]'
        ' | P u0 lattice=+ lattice_t=+'
        ' | fwd=lattice*5(LatticePlan#0,LatticeConfig#1)',
    ],
    'mesh-f32-32': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#2)'
        ' | bwd=tiles*1(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
    ],
    'mesh-f32-32-A': [
        'F[spmm_rowpack] B[sddmm_tile]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_tile] B[sddmm_tile]'
        ' | P u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*1(TilePlan#1)',
        'F[spmm_tile] B[sddmm_tile]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*2(TilePlan#1)',
        'F[spmm_tile] B[sddmm_tile]'
        ' | P u9 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*3(TilePlan#1)',
        'F[spmm_tile] B[sddmm_tile]'
        ' | P u11 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*4(TilePlan#1)',
    ],
    'mesh-f32-32-B': [
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_tile] B[spmm_tile]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#1)',
        'F[spmm_tile] B[spmm_tile]'
        ' | P u4 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#1)',
        'F[spmm_tile] B[spmm_tile]'
        ' | P u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*3(TilePlan#1)',
        'F[spmm_tile] B[spmm_tile]'
        ' | P u6 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*4(TilePlan#1)',
    ],
    'mesh-f32-16': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'mesh-f32-32-notile': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'mesh-f32-32-async': [
        'F[spmm] B[mm_backward]'
        ' | P u3 64.2048.3072.65536.False.2=~ tile.64.224.1792=~ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=~'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_tile] B[mm_backward_rowpack]'
        ' | P u5 tile.64.224.1792=+ 64.2048.3072.65536.False.2=~ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=~'
        ' | fwd=tiles*1(TilePlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u7 tile.64.224.1792=+ 64.2048.3072.65536.False.2=~ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#1)'
        ' | bwd=tiles*1(TilePlan#1,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u9 tile.64.224.1792=+ 64.2048.3072.65536.False.2=~ lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*3(TilePlan#1)'
        ' | bwd=tiles*2(TilePlan#1,TilePlan#3)',
        'F[] B[]'
        ' | P u9 tile.64.224.1792=+ 64.2048.3072.65536.False.2=~ lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*3(TilePlan#1)'
        ' | bwd=tiles*2(TilePlan#1,TilePlan#3)',
    ],
    'mesh-f32-32-tview': [
        'F[spmm] B[mm_backward_rowpack]'
        ' | P u1 lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=plan-free*1()'
        ' | bwd=row pairs*1(RowPackPlan#0)',
        'F[spmm] B[sddmm_tile spmm_tile]'
        ' | P u2 tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=plan-free*2()'
        ' | bwd=tiles*1(TilePlan#1,TilePlan#2)',
        'F[spmm] B[sddmm_tile spmm_tile]'
        ' | P u3 tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=plan-free*3()'
        ' | bwd=tiles*2(TilePlan#1,TilePlan#2)',
        'F[spmm] B[sddmm_tile spmm_tile]'
        ' | P u4 tile.64.224.1792=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=plan-free*4()'
        ' | bwd=tiles*3(TilePlan#1,TilePlan#2)',
        'F[spmm] B[sddmm_tile spmm_tile]'
        ' | P u5 tile.64.224.1792=+ lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=plan-free*5()'
        ' | bwd=tiles*4(TilePlan#1,TilePlan#2)',
    ],
    'mesh-f64-32': [
        'F[spmm] B[sddmm spmm]'
        ' | P u0 lattice=-'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[sddmm spmm]'
        ' | P u0 lattice=-'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[sddmm spmm]'
        ' | P u0 lattice=-'
        ' | T u0'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[sddmm spmm]'
        ' | P u0 lattice=-'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0 lattice=-'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'mesh-coo-f32-32': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#2)'
        ' | bwd=tiles*1(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
    ],
    'mesh-coo_unc-f32-32': [
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=plan-free*1()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*2()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u6 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*3()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u8 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*4()',
        'F[spmm] B[coo_sddmm spmm_rowpack]'
        ' | P u10 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | T u10 64.2048.3072.65536.True.2=+ tile.64.224.1792=-'
        ' | fwd=plan-free*5()',
    ],
    'mesh-coo_unc-f32-32-A': [
        'F[spmm] B[coo_sddmm]'
        ' | P u2 64.2048.3072.65536.True.2=-'
        ' | fwd=plan-free*1()',
        'F[spmm] B[coo_sddmm]'
        ' | P u4 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*2()',
        'F[spmm] B[coo_sddmm]'
        ' | P u6 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*3()',
        'F[spmm] B[coo_sddmm]'
        ' | P u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*4()',
        'F[spmm] B[coo_sddmm]'
        ' | P u10 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*5()',
    ],
    'mesh-bcsr-f32-32': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | F u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | FT u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u0'
        ' | F u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | FT u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#2)'
        ' | bwd=tiles*1(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u0'
        ' | F u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | FT u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u0'
        ' | F u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | FT u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u0'
        ' | F u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | FT u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
    ],
    'mesh-bcsr-f32-32-B': [
        'F[spmm_rowpack] B[spmm]'
        ' | P u0'
        ' | T u0'
        ' | F u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_tile] B[spmm_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*1(TilePlan#1)',
        'F[spmm_tile] B[spmm_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u4 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*2(TilePlan#1)',
        'F[spmm_tile] B[spmm_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*3(TilePlan#1)',
        'F[spmm_tile] B[spmm_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u6 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | fwd=tiles*4(TilePlan#1)',
    ],
    'mesh-bcsr-f32-16': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u1 lattice=-'
        ' | FT u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | FT u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | FT u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | FT u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u0'
        ' | T u0'
        ' | F u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | FT u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'mesh-bcoo-f32-32': [
        'F[spmm_rowpack] B[sddmm_tile spmm_tile]'
        ' | P u4 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u6 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#2)'
        ' | bwd=tiles*1(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u8 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u10 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*3(TilePlan#2)'
        ' | bwd=tiles*3(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u12 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u7 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*4(TilePlan#2)'
        ' | bwd=tiles*4(TilePlan#2,TilePlan#3)',
    ],
    'mesh_wide-f32-32-notile': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u7 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u7 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u9 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u9 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'mesh_wide-f32-16': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[sddmm spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm spmm_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm spmm_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u7 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm spmm_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u9 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'mesh_wide-f32-32-notile-volatile': [
        'F[spmm] B[mm_backward]'
        ' | P u1 volatile=2'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ volatile=6'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+ lattice=- volatile=6'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u7 64.2048.3072.65536.False.2=+ lattice=- volatile=6'
        ' | T u7 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u9 64.2048.3072.65536.False.2=+ lattice=- volatile=6'
        ' | T u9 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u11 64.2048.3072.65536.False.2=+ lattice=- volatile=6'
        ' | T u11 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*5(RowPackPlan#1)'
        ' | bwd=row pairs*5(RowPackPlan#2)',
        'F[spmm_rowpack] B[sddmm_rowpack spmm_rowpack]'
        ' | P u13 64.2048.3072.65536.False.2=+ lattice=- volatile=6'
        ' | T u13 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*6(RowPackPlan#1)'
        ' | bwd=row pairs*6(RowPackPlan#2)',
    ],
    'banded-f32-32': [
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)'
        ' | bwd=row pairs*1(RowPackPlan#1)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u5 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*1(TilePlan#2)'
        ' | bwd=tiles*1(TilePlan#2,TilePlan#3)',
        'F[spmm_tile] B[sddmm_tile spmm_tile]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
        'F[] B[]'
        ' | P u7 64.2048.3072.65536.False.2=+ tile.64.224.1792=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+ tile.64.224.1792=+'
        ' | fwd=tiles*2(TilePlan#2)'
        ' | bwd=tiles*2(TilePlan#2,TilePlan#3)',
    ],
    'banded-f32-16': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'banded-f32-16-B': [
        'F[spmm] B[spmm]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#0)',
    ],
    'banded-f32-16-async': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u2 64.2048.3072.65536.True.2=~ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=~'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
    ],
    'banded-bf16-64': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'banded-bf16-64-A': [
        'F[spmm] B[sddmm_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=plan-free*1()',
        'F[spmm_rowpack] B[sddmm_rowpack]'
        ' | P u4 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm_rowpack]'
        ' | P u6 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=row pairs*2(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm_rowpack]'
        ' | P u8 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=row pairs*3(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm_rowpack]'
        ' | P u10 64.2048.3072.65536.False.2=+ lattice=-'
        ' | fwd=row pairs*4(RowPackPlan#0)',
    ],
    'banded-bf16-64-B': [
        'F[spmm] B[spmm]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u2 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u3 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u4 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#0)',
        'F[spmm_rowpack] B[spmm_rowpack]'
        ' | P u5 64.2048.3072.65536.False.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#0)',
    ],
    'banded-bf16-16': [
        'F[spmm] B[mm_backward]'
        ' | P u1 lattice=-'
        ' | T u1'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*1(RowPackPlan#1)'
        ' | bwd=row pairs*1(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u3 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*2(RowPackPlan#1)'
        ' | bwd=row pairs*2(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*3(RowPackPlan#1)'
        ' | bwd=row pairs*3(RowPackPlan#2)',
        'F[spmm_rowpack] B[mm_backward_rowpack]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | T u5 64.2048.3072.65536.True.2=+'
        ' | fwd=row pairs*4(RowPackPlan#1)'
        ' | bwd=row pairs*4(RowPackPlan#2)',
    ],
    'banded-f32-8-A': [
        'F[spmm] B[sddmm]'
        ' | P u1 lattice=-'
        ' | fwd=plan-free*1()',
        'F[spmm_rowpack] B[sddmm]'
        ' | P u2 64.2048.3072.65536.True.2=+ lattice=-'
        ' | fwd=row pairs*1(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm]'
        ' | P u3 64.2048.3072.65536.True.2=+ lattice=-'
        ' | fwd=row pairs*2(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm]'
        ' | P u4 64.2048.3072.65536.True.2=+ lattice=-'
        ' | fwd=row pairs*3(RowPackPlan#0)',
        'F[spmm_rowpack] B[sddmm]'
        ' | P u5 64.2048.3072.65536.True.2=+ lattice=-'
        ' | fwd=row pairs*4(RowPackPlan#0)',
    ],
    'random-f32-32': [
        'F[spmm] B[mm_backward]'
        ' | P u3 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | T u2 64.2048.3072.65536.True.2=-'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u6 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | T u4 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u9 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | T u6 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u12 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | T u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u12 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | T u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'random-bcsr-f32-32': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u3 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | FT u2 64.2048.3072.65536.True.2=-'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u6 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | FT u4 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u9 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | FT u6 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | F u12 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | FT u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0'
        ' | T u0'
        ' | F u12 64.2048.3072.65536.False.2=- tile.64.224.1792=- lattice=-'
        ' | FT u8 64.2048.3072.65536.True.2=- tile.64.224.1792=-'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
    'small-f32-32': [
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*1()'
        ' | bwd=plan-free*1(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*2()'
        ' | bwd=plan-free*2(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*3()'
        ' | bwd=plan-free*3(RowGather#0)',
        'F[spmm] B[mm_backward]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
        'F[] B[]'
        ' | P u0'
        ' | T u0'
        ' | fwd=plan-free*4()'
        ' | bwd=plan-free*4(RowGather#0)',
    ],
}
