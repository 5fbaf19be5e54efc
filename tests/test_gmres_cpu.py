"""`gmres` without a GPU: the public surface, the staged header csrc/tsgu_hip_gmres.h against its ctypes table and the library, the
host refusals of every launcher (fake pointers, device = -1: nothing is dereferenced), and the torch-op path on CPU tensors in
fp64 against the mirror (tests/_gmres_ref.py) and numpy.linalg.solve.

The solution bound is derived: a column returns only with a true residual of at most threshold_c = max(abstol, reltol |r0|) (or at
maxiter), so |x - x*|_2 <= |A^-1|_2 threshold_c; the float64 evaluation of that residual adds gamma_{r+1}(2^-53) (| |A| |x| | + |b|).
Iteration counts are compared with the mirror's at tolerances where every decision of the mirror is 1 % away from its threshold.
"""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _abi_cases as A
import _gmres_ref as GR
from torchsparsegradutils_amd import _backend, utils
from torchsparsegradutils_amd.utils import GMRESSettings, gmres, gmres_t, last_solve_info

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_gmres.h")
ENTRIES = ("tsgu_gmres_geometry", "tsgu_gmres_project", "tsgu_gmres_subtract", "tsgu_gmres_scale", "tsgu_gmres_scalar",
           "tsgu_gmres_update")
U = 2.0 ** -53


# ---- surface ----------------------------------------------------------------------------------------------------------------------

def test_surface():
    assert {"gmres", "gmres_t", "GMRESSettings"} <= set(utils.__all__)
    s = GMRESSettings()
    assert (s.restart, s.maxiter, s.abstol, s.reltol, s.precon, s.flexible, s.transpose) == (30, None, 1e-8, 1e-6, None, False, False)
    assert s.logger.disabled
    M = torch.eye(4, dtype=torch.float64)
    b = torch.ones(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="restart must be at least 1"):
        gmres(M, b, settings=GMRESSettings(restart=0))
    with pytest.raises(RuntimeError, match="settings.precon must be a tensor, or a callable object!"):
        gmres(M, b, settings=GMRESSettings(precon=3))
    with pytest.raises(RuntimeError, match="transpose=True needs a tensor operator"):
        gmres(M.matmul, b, settings=GMRESSettings(transpose=True))
    with pytest.raises(RuntimeError, match="matmul_closure must be a tensor, or a callable object!"):
        gmres(3, b)
    assert gmres(M, b).shape == (4,) and gmres(M, b.unsqueeze(-1)).shape == (4, 1)
    assert last_solve_info("gmres")["fused"] is False


# ---- the staged header --------------------------------------------------------------------------------------------------------------

def test_the_staged_header_is_bound():
    assert _backend.STAGED_GMRES == {"tsgu_hip_gmres.h": _backend.SIGNATURES_GMRES}
    others = (_backend.ABI, _backend.STAGED, _backend.STAGED_AMG)
    assert not any(set(_backend.STAGED_GMRES) & set(reg) for reg in others)
    names = set(_backend.SIGNATURES_GMRES)
    assert not any(names & set(table) for reg in others for table in reg.values())
    assert not os.path.exists(os.path.join(A.INCLUDE, "tsgu_hip_gmres.h"))
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_GMRES)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_GMRES[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for name, params in protos[1:]:
        assert params[-2:] == [("device", "int"), ("stream", "void*")], name
    text = open(STAGED_HEADER).read()
    assert '#include "../../include/tsgu_hip.h"' in text and "TSGU_ABI_VERSION" in text
    assert lib.tsgu_abi_version() == 7 == _backend.ABI_VERSION


def test_geometry():
    for td, wide in ((torch.float32, 4), (torch.float64, 2)):
        for n, p in ((1, 1), (1000, 1), (1000, 3), (1000, 4), (5000, 64), (5000, 65), (5000, 256), (5000, 256 * wide)):
            cap, group, rows, parts = _backend.gmres_geometry(td, n, p)
            lpr = p // wide if p % wide == 0 else p
            assert cap >= 64 and group == 4 and rows == (256 // lpr) * 4 and parts == -(-n // rows), (td, n, p)
        with pytest.raises(RuntimeError, match="simultaneous right-hand sides"):
            _backend.gmres_geometry(td, 100, 257)
    lib = _backend.load_library()
    outs = [ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()]
    refs = [ctypes.byref(o) for o in outs]
    assert lib.tsgu_gmres_geometry(0, 100, 4, *refs) == A.OK
    for k in range(4):
        assert lib.tsgu_gmres_geometry(0, 100, 4, *[None if j == k else r for j, r in enumerate(refs)]) == A.BAD_ARG
    assert lib.tsgu_gmres_geometry(2, 100, 4, *refs) == A.BAD_DTYPE
    assert lib.tsgu_gmres_geometry(0, 0, 4, *refs) == A.BAD_ARG and lib.tsgu_gmres_geometry(0, 100, 0, *refs) == A.BAD_ARG
    assert _backend.gmres_state_rows(30)["rows"] == 30 * 30 + 6 * 30 + 4


# ---- host refusals: every call below is refused before the device is touched (the base call only by set_device(-1)) ------------------

BASE = {
    "tsgu_gmres_project": dict(vtype=0, n=8, p=4, k=2, w=0x10000, basis=0x20000, slab=32, partial=0x30000, flags=0x40000,
                               inner=1),
    "tsgu_gmres_subtract": dict(vtype=0, n=8, p=4, k=2, w=0x10000, basis=0x20000, slab=32, coef=0x50000, out=0x60000,
                                partial=0x30000, flags=0x40000, inner=1),
    "tsgu_gmres_scale": dict(vtype=0, n=8, p=4, w=0x10000, hnorm=0x50000, out=0x60000, flags=0x40000, inner=1),
    "tsgu_gmres_scalar": dict(vtype=0, phase=1, j=0, m=4, partial=0x30000, n_partial=1, fold=None, scal=0x50000, flags=0x40000,
                              abstol=0.0, reltol=1e-6, maxiter=10, p=4),
    "tsgu_gmres_update": dict(vtype=0, n=8, p=4, k=2, x=0x10000, basis=0x20000, slab=32, y=0x50000, flags=0x40000),
}
ALIGNED = {"tsgu_gmres_project": ("w", "basis"), "tsgu_gmres_subtract": ("w", "basis", "out"), "tsgu_gmres_scale": ("w", "out"),
           "tsgu_gmres_scalar": (), "tsgu_gmres_update": ("x", "basis")}
OPTIONAL = {"fold"}


def _call(name, **changes):
    a = dict(BASE[name])
    a.update(changes)
    return getattr(_backend.load_library(), name)(*a.values(), -1, None)


@pytest.mark.parametrize("name", list(BASE))
def test_host_refusals(name):
    params = dict(A.prototypes(STAGED_HEADER))[name]
    assert [q[0] for q in params[:-2]] == list(BASE[name]), "the base call names the header's parameters"
    cap = _backend.gmres_geometry(torch.float32, 8, 4)[0]
    assert _call(name) == A.BAD_ARG, "device = -1 is refused (and nothing before it)"
    for pn, pt in params[:-2]:
        if pt.endswith("*") and pn not in OPTIONAL:
            assert _call(name, **{pn: None}) == A.BAD_ARG, (name, pn)
        if pn in ALIGNED[name]:
            assert _call(name, **{pn: BASE[name][pn] + 4}) == A.BAD_ARG, (name, pn, "misaligned")
    assert _call(name, vtype=2) == A.BAD_DTYPE and _call(name, vtype=7) == A.BAD_DTYPE
    assert _call(name, p=0) == A.BAD_ARG and _call(name, p=-1) == A.BAD_ARG
    if "n" in BASE[name]:
        assert _call(name, n=0) == A.BAD_ARG
        big = dict(slab=1 << 20) if "slab" in BASE[name] else {}
        for vt, p in ((0, 257), (0, 1028), (1, 259), (1, 514)):
            assert _call(name, vtype=vt, p=p, **big) == A.TOO_LARGE, (name, vt, p)
        # the widest widths are covered: refused only by the device
        assert _call(name, vtype=0, p=1024, **big) == A.BAD_ARG and _call(name, vtype=1, p=512, **big) == A.BAD_ARG
    if "k" in BASE[name]:
        for k in (0, -1, cap + 2):
            assert _call(name, k=k) == A.BAD_ARG, (name, k)
        for slab in (31, 34, 0, -4):          # shorter than a block, or blocks that would not start on 16-byte boundaries
            assert _call(name, slab=slab) == A.BAD_ARG, (name, slab)
    if name == "tsgu_gmres_scalar":
        for ch in (dict(phase=-1), dict(phase=5), dict(m=0), dict(m=cap + 1), dict(j=-1), dict(j=4), dict(n_partial=0),
                   dict(phase=0, partial=None), dict(phase=3, n_partial=0)):
            assert _call(name, **ch) == A.BAD_ARG, ch


# ---- the torch-op path on CPU tensors -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def problems():
    out = {}
    for name, make in (("convdiff", GR.convdiff), ("random", GR.random_shifted)):
        M = make()
        rng = np.random.default_rng(7)
        B = rng.standard_normal((M.shape[0], 3))
        B[:, 1] = 0.0                                                   # a zero column
        B[:, 2] *= 1e-3                                                 # (a column of another scale)
        out[name] = (M, B, 1.0 / np.linalg.svd(M, compute_uv=False)[-1], np.linalg.solve(M, B))
    return out


def _csr(M):
    return torch.from_numpy(M).to_sparse_csr()


def _check(M, B, X, thr, inv_norm, Xs):
    longest = int((M != 0).sum(axis=1).max())
    slack = GR.gamma(longest + 1, U) * (np.linalg.norm(np.abs(M) @ np.abs(X), axis=0) + np.linalg.norm(B, axis=0))
    res = np.linalg.norm(B - M @ X, axis=0)
    assert (res <= thr + slack).all(), (res, thr)
    assert (np.linalg.norm(X - Xs, axis=0) <= inv_norm * (thr + slack)).all()


@pytest.mark.parametrize("name", ["convdiff", "random"])
@pytest.mark.parametrize("m", [1, 2, 5, 30])
def test_solution_and_iteration_counts_against_the_mirror(problems, name, m):
    M, B, inv_norm, Xs = problems[name]
    tol = GR.pick_reltol(M, B, m)
    Xm, its, cyc, margin = GR.solve(M, B, m, abstol=0.0, reltol=tol)
    x = gmres(_csr(M), torch.from_numpy(B), settings=GMRESSettings(restart=m, reltol=tol, abstol=0.0)).numpy()
    info = last_solve_info("gmres")
    assert margin >= 0.01 and info["iterations"].tolist() == its.tolist() and info["cycles"] == cyc.max()
    assert its[1] == 0 and not x[:, 1].any(), "a zero column: x = 0, zero iterations"
    if m < 30:
        assert cyc.max() > 1, "several cycles"
    thr = tol * np.linalg.norm(B, axis=0)
    _check(M, B, x, thr, inv_norm, Xs)
    assert (np.linalg.norm(x - Xm, axis=0) <= 2 * inv_norm * thr + 1e-12).all()
    # coo and dense operands, a vector right-hand side
    xd = gmres(torch.from_numpy(M), torch.from_numpy(B[:, 0]), settings=GMRESSettings(restart=m, reltol=tol, abstol=0.0)).numpy()
    assert last_solve_info("gmres")["iterations"].tolist() == [its[0]]
    _check(M, B[:, :1], xd[:, None], thr[:1], inv_norm, Xs[:, :1])


def test_transpose(problems):
    M, B, inv_norm, Xs = problems["convdiff"]
    Bt = torch.from_numpy(B)
    st = GMRESSettings(reltol=1e-9, abstol=0.0)
    xt = gmres_t(_csr(M), Bt, settings=st)
    assert torch.equal(xt, gmres(_csr(M), Bt, settings=st._replace(transpose=True)))
    assert torch.equal(gmres_t(_csr(M), Bt, settings=st._replace(transpose=True)), gmres(_csr(M), Bt, settings=st))
    thr = 1e-9 * np.linalg.norm(B, axis=0)
    _check(M.T, B, xt.numpy(), thr, inv_norm, np.linalg.solve(M.T, B))
    xd = gmres_t(torch.from_numpy(M), Bt, settings=st)
    _check(M.T, B, xd.numpy(), thr, inv_norm, np.linalg.solve(M.T, B))


def test_preconditioners(problems):
    M, B, inv_norm, Xs = problems["random"]
    rng = np.random.default_rng(9)
    P = np.linalg.inv(M) + 0.02 * rng.standard_normal(M.shape) / np.sqrt(M.shape[0])
    Bt, Pt = torch.from_numpy(B), torch.from_numpy(P)
    tol = GR.pick_reltol(M, B, 30, M=P)
    st = GMRESSettings(reltol=tol, abstol=0.0)
    thr = tol * np.linalg.norm(B, axis=0)
    _, its, _, _ = GR.solve(M, B, 30, abstol=0.0, reltol=tol, M=P)
    _, plain, _, _ = GR.solve(M, B, 30, abstol=0.0, reltol=tol)
    assert its.max() < plain.max()
    calls = []

    def fn(V):
        calls.append(tuple(V.shape))
        return Pt @ V

    for precon in (Pt, fn):
        x = gmres(_csr(M), Bt, settings=st._replace(precon=precon))
        assert last_solve_info("gmres")["iterations"].tolist() == its.tolist()
        _check(M, B, x.numpy(), thr, inv_norm, Xs)
    assert calls and set(calls) == {(M.shape[0], 3)}, "a callable sees the whole (n, p) block"
    # Aᵀ with the tensor preconditioner: Mᵀ is applied
    xt = gmres_t(_csr(M), Bt, settings=st._replace(precon=Pt))
    _check(M.T, B, xt.numpy(), thr, inv_norm, np.linalg.solve(M.T, B))
    assert last_solve_info("gmres")["iterations"].max() < plain.max()

    class Solver:
        seen = []

        def solve(self, R, transpose=False):
            self.seen.append(transpose)
            return (Pt.t() if transpose else Pt) @ R

    obj = Solver()
    for tr in (False, True):
        x = gmres(_csr(M), Bt, settings=st._replace(precon=obj, transpose=tr))
        _check(M.T if tr else M, B, x.numpy(), thr, inv_norm, np.linalg.solve(M.T if tr else M, B))
    assert set(obj.seen) == {False, True}
    # flexible: a preconditioner that changes between applications
    count = [0]

    def changing(V):
        count[0] += 1
        return (Pt @ V) * (1.0 + 0.3 * (count[0] % 3))

    x = gmres(_csr(M), Bt, settings=st._replace(precon=changing, flexible=True))
    _check(M, B, x.numpy(), thr, inv_norm, Xs)


def test_lucky_breakdown_and_exact_initial_guess(problems):
    n = 12
    I2 = (2.0 * torch.eye(n, dtype=torch.float64)).to_sparse_csr()
    b = torch.from_numpy(np.random.default_rng(1).standard_normal((n, 2)))
    x = gmres(I2, b)
    assert last_solve_info("gmres")["iterations"].tolist() == [1, 1] and last_solve_info("gmres")["cycles"] == 1, "h_{1,0} = 0 at step 0"
    # x = (b (1 / beta)) (beta / 2): a division, three multiplications and the sums of beta, each within one rounding of n terms
    assert bool(((x - b / 2).abs() <= GR.gamma(n + 4, U) * (b / 2).abs()).all())
    M, B, inv_norm, Xs = problems["convdiff"]
    x0 = torch.from_numpy(Xs)
    x = gmres(_csr(M), torch.from_numpy(B), initial_guess=x0, settings=GMRESSettings(abstol=1e-8, reltol=0.0))
    assert torch.equal(x, x0) and last_solve_info("gmres")["iterations"].tolist() == [0, 0, 0]


def test_frozen_columns_and_maxiter(problems):
    M, B, inv_norm, Xs = problems["convdiff"]
    Bw = B.copy()
    Bw[:, 1] = M[:, 3] + M[:, 17]                               # b = A (e_3 + e_17): a column that stops cycles before the others
    m = 4
    st = GMRESSettings(restart=m, reltol=1e-10, abstol=0.0)
    A_t = _csr(M)
    X = gmres(A_t, torch.from_numpy(Bw), settings=st)
    its = last_solve_info("gmres")["iterations"]
    cyc = [-(-int(i) // m) for i in its]
    assert len(set(cyc)) > 1, "the columns stop in different cycles"
    # the same block cut off at the end of the cycle in which the earliest column stops: that column has the bits it has in the
    # full solve, where the others ran on for more cycles
    early = int(np.argmin(cyc))
    cut = gmres(A_t, torch.from_numpy(Bw), settings=st._replace(maxiter=cyc[early] * m))
    assert last_solve_info("gmres")["iterations"].tolist() == [min(int(i), cyc[early] * m) for i in its]
    assert torch.equal(cut[:, early], X[:, early]), "a column is frozen bit for bit while the others run"
    assert not torch.equal(cut, X)
    for c in range(3):
        alone = gmres(A_t, torch.from_numpy(Bw[:, c:c + 1].copy()), settings=st)
        assert last_solve_info("gmres")["iterations"].tolist() == [int(its[c])], "a column's stopping point is its own"
    # the cut-off: maxiter inner steps per column, then the column is finished whatever its residual
    X = gmres(A_t, torch.from_numpy(B), settings=st._replace(maxiter=6))
    assert last_solve_info("gmres")["iterations"].tolist() == [6, 0, 6] and last_solve_info("gmres")["cycles"] == 2
    Xm, itm, _, _ = GR.solve(M, B, m, maxiter=6, abstol=0.0, reltol=1e-10)
    assert itm.tolist() == [6, 0, 6] and np.abs(X.numpy() - Xm).max() <= 1e-12 * np.abs(Xm).max()
    X = gmres(A_t, torch.from_numpy(B), settings=st._replace(maxiter=0))
    assert not X.any() and last_solve_info("gmres")["iterations"].tolist() == [0, 0, 0]


def test_restart_above_the_cap_takes_the_torch_path(problems):
    M, B, inv_norm, Xs = problems["convdiff"]
    cap = _backend.gmres_geometry(torch.float64, M.shape[0], 1)[0]
    x = gmres(_csr(M), torch.from_numpy(B), settings=GMRESSettings(restart=cap + 6, reltol=1e-9, abstol=0.0))
    assert last_solve_info("gmres")["restart"] == cap + 6 and last_solve_info("gmres")["cycles"] == 1
    _check(M, B, x.numpy(), 1e-9 * np.linalg.norm(B, axis=0), inv_norm, Xs)
    assert "gmres" in sys.modules["torchsparsegradutils_amd.utils"].last_solve_info.__doc__
