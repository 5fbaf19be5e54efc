"""The float64 mirror of the Krylov step kernels (tests/_krylov_ref.py) checked on its own, without a GPU: the mirrored steps, chained
the way the drivers chain the kernels, reproduce oracle/oracle.py's linear_cg and the MINRES / BiCGSTAB solutions stored in
tests/golden/generic_small.npz to 1e-12.  Also the library's three size queries at the widths the step kernels accept and refuse,
and the message the drivers raise for a refused width (host code only: no launch)."""

import numpy as np
import pytest
import torch

import _golden as G
import _krylov_ref as K
from oracle import oracle
from torchsparsegradutils_amd import _backend

W = np.longdouble if K.LONG_OK else np.float64


def T(a):
    return K.Tr(np.asarray(a, dtype=W))


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.fixture(scope="module")
def systems():
    z = G.load("generic_small.npz")
    return z


def _normalised(B):
    nrm = np.sqrt((B * B).sum(0, keepdims=True))
    return B / nrm, nrm


# ---- CG --------------------------------------------------------------------------------------------------------------------

def _cg_start(S, B, stop_after):
    rhs, nrm = _normalised(B)
    n, p = rhs.shape
    r = T(rhs)
    return n, p, r, T(np.zeros((n, p))), nrm, (np.sqrt((rhs * rhs).sum(0)) < stop_after).astype(np.int64)


@pytest.mark.parametrize("tol", [1e-12, 1e-3])      # (the reference's eps guards freeze CG near 1e-6: 1e-12 runs every iteration)
@pytest.mark.parametrize("R", [1, 5, 12, 64])
def test_cg_four_steps_reproduce_the_oracle(systems, R, tol):
    S, B = systems["S"], systems["csr_2d6_cg_B"]
    eps, stop_after, max_iter = 1e-10, 1e-10, 40
    n, p, r, x, nrm, conv = _cg_start(S, B, stop_after)
    A = np.asarray(S, dtype=W)
    scal = T(np.zeros((4, p)))
    scal = K._set_rows(scal, {0: K.coldot(r, r)})
    flags = np.concatenate([[0, 0], conv, np.zeros(p, dtype=np.int64)])
    pv = r
    for k in range(max_iter):
        Ap = T(A @ pv.v)
        pap = K.block_sums(K.Tr(pv.v * Ap.v), R)
        if k % 2:       # the one-launch form of steps 1 + 2 must be the two steps
            got = K.cg_update1_alpha(r, Ap, x, pv, pap, scal, flags, eps, R)
            if got is not None:
                r, x, scal, part = got
        else:
            scal = K.cg_alpha(pap, scal, flags, eps, p)
            got = K.cg_update1(r, Ap, x, pv, scal, flags, R)
            if got is not None:
                r, x, part = got
        scal, flags = K.cg_beta(part, scal, flags, eps, stop_after, tol, -1, min(10, max_iter - 1), p)
        nxt = K.cg_update2(r, pv, scal, flags)
        pv = pv if nxt is None else nxt
    rows, cols = np.nonzero(S)
    crow, col = G.coo_to_csr_arrays(np.stack([rows, cols]), n)
    xo, iters, _ = oracle.linear_cg(crow, col, S[rows, cols], B, tol, max_iter=max_iter, eps=eps, stop_updating_after=stop_after)
    assert flags[0] == (iters < max_iter) and flags[1] == iters and (iters < max_iter) == (tol == 1e-3)
    assert rel(x.v * nrm, xo) < 1e-12


def test_cg_two_launch_form_reproduces_the_oracle(systems):
    S, B = systems["S"], systems["csr_2d6_cg_B"].copy()
    B[:, 2] = 0.0                                              # a zero right-hand side: norm masked, column frozen at once
    eps, stop_after, tol, max_iter, R, n_hist = 1e-10, 1e-10, 1e-3, 40, 5, 4
    rhs_norm = np.sqrt((B * B).sum(0, keepdims=True))
    zero = rhs_norm[0] < eps
    rhs = B / np.where(zero, 1.0, rhs_norm)
    n, p = rhs.shape
    A = np.asarray(S, dtype=W)
    r, x = T(rhs), T(np.zeros((n, p)))
    scal = K._set_rows(T(np.zeros((5, p))), {0: K.coldot(r, r)})
    flags = np.zeros(4 + 3 * p, dtype=np.int64)
    flags[4:4 + p] = np.sqrt((rhs * rhs).sum(0)) < stop_after
    flags[4 + 2 * p:] = zero
    hist = T(np.zeros((n_hist, 2, p)))
    pv, par, first_alpha = r, 0, None
    for k in range(max_iter):
        Ap = T(A @ pv.v)
        got = K.cg2_residual(r, Ap, K.block_sums(K.Tr(pv.v * Ap.v), R), scal, flags, par, eps, R)
        if got is not None:
            r, scal, part = got
            first_alpha = scal.v[2].copy() if k == 0 else first_alpha
        p2, x2, scal, flags, hist = K.cg2_direction(r, pv, x, part, scal, flags, par, eps, stop_after, tol, min(10, max_iter - 1),
                                                    hist, n_hist)
        if p2 is not None:
            pv, x = p2, x2
        par ^= 1
    rows, cols = np.nonzero(S)
    crow, col = G.coo_to_csr_arrays(np.stack([rows, cols]), n)
    xo, iters, _ = oracle.linear_cg(crow, col, S[rows, cols], B, tol, max_iter=max_iter, eps=eps, stop_updating_after=stop_after)
    assert flags[0] == 1 and flags[1] == 1 and flags[2] == iters            # the done word followed into both halves
    assert rel(x.v * np.where(zero, 1.0, rhs_norm), xo) < 1e-12
    assert np.all(x.v[:, 2] == 0) and np.all(scal.v[4, 2] == 0)
    assert np.array_equal(hist.v[0, 0], first_alpha) and np.all(hist.v[:, :, [0, 1, 3, 4, 5]] != 0)


# ---- MINRES ------------------------------------------------------------------------------------------------------------------

def _minres(S, B, shifts, value, tol, eps=1e-25, max_iter=1000, R=5, precond_diag=None):
    """The drivers' sequence (scalar 0 -> vector 0 -> scalar 1 -> vector 1 [-> scalar 2 on every tenth iteration])."""
    rhs, nrm = _normalised(B)
    n, p = rhs.shape
    A = np.asarray(S, dtype=W)
    ns = len(shifts)
    M = None if precond_diag is None else np.asarray(precond_diag, dtype=W).reshape(-1, 1)
    z = [T(np.zeros((n, p))), T(rhs)]
    q1 = None if M is None else K.Tr(M * z[1].v)
    beta0 = np.sqrt((z[1].v * (z[1].v if M is None else q1.v)).sum(0))
    z[1] = K.Tr(z[1].v / beta0)
    q = None if M is None else [None, K.Tr(q1.v / beta0)]
    w = [T(np.zeros((ns, n, p))), T(np.zeros((ns, n, p)))]
    sol = T(np.zeros((ns, n, p)))
    sc = np.zeros((ns, 12, p), dtype=W)
    sc[0, 1] = sc[0, 11] = beta0
    sc[:, 6] = beta0
    sc[:, 2] = sc[:, 4] = 1
    scal, flags = K.Tr(sc), np.zeros(2, dtype=np.int64)
    sh = np.asarray(shifts, dtype=W)
    for i in range(min(max_iter, n + 1) + 2):
        check = (i + 1) % 10 == 0
        qp = z[1] if q is None else q[1]
        prod = T(A @ qp.v)
        scal, flags = K.minres_scalar(0, K.block_sums(K.Tr(prod.v * qp.v), R), scal, flags, eps, tol, sh, value)
        got = K.minres_lanczos(z[0], z[1], prod, scal, flags, value, R)
        if got is None:
            break
        z[0], part = got
        if q is None:
            scal, flags = K.minres_scalar(1, part, scal, flags, eps, tol, sh, value)
            z[0], _, w[0], sol, norms = K.minres_update(z[0], z[1], w[0], w[1], sol, scal, flags, R, check)
        else:
            q[0] = K.Tr(M * z[0].v)
            scal, flags = K.minres_scalar(1, K.block_sums(K.Tr(z[0].v * q[0].v), R), scal, flags, eps, tol, sh, value)
            z[0], q[0], w[0], sol, norms = K.minres_update(z[0], q[1], w[0], w[1], sol, scal, flags, R, check, qc=q[0])
            q.reverse()
        if check:
            scal, flags = K.minres_scalar(2, norms, scal, flags, eps, tol, sh, value)
        z.reverse()
        w.reverse()
    return sol.v * nrm[None], flags


def test_minres_steps_reproduce_the_stored_solution(systems):
    S, B = systems["S"], systems["csr_2d6_minres_B"]
    x, flags = _minres(S, B, [0.0], 1.0, 1e-12)
    assert rel(x[0], systems["csr_2d6_minres_x"]) < 1e-12
    assert flags[1] == min(1000, S.shape[0] + 1) + 2 or flags[0] == 1


@pytest.mark.parametrize("precond", [False, True])
def test_minres_steps_with_shifts_value_and_preconditioner_match_the_oracle(systems, precond):
    S, B = systems["S"], systems["csr_2d6_minres_B"]
    n = S.shape[0]
    rows, cols = np.nonzero(S)
    crow, col = G.coo_to_csr_arrays(np.stack([rows, cols]), n)
    shifts, value = [0.0, 0.5, 2.0], 0.75
    dinv = 1.0 / np.diag(S) if precond else None
    xo = oracle.minres(crow, col, S[rows, cols], B, shifts=shifts, value=value, precond_diag=dinv, tolerance=1e-12)
    x, _ = _minres(S, B, shifts, value, 1e-12, precond_diag=dinv)
    assert rel(x, xo) < 1e-12


# ---- BiCGSTAB ------------------------------------------------------------------------------------------------------------------

def _bicgstab(Amat, B, abstol, reltol, matvec_max=None, R=5, precond_diag=None, x0=None):
    """The drivers' sequence of the eleven steps of an iteration, every column in lock-step."""
    n, p = B.shape
    A = np.asarray(Amat, dtype=W)
    M = None if precond_diag is None else np.asarray(precond_diag, dtype=W).reshape(-1, 1)
    matvec_max = 2 * n if matvec_max is None else matvec_max
    if x0 is None:
        x, r0, nmv0 = T(np.zeros((n, p))), T(B), 1
    else:
        x, r0, nmv0 = T(x0), T(B), 0
    scal, flags = T(np.zeros((8, p))), np.zeros(2 + 3 * p, dtype=np.int64)
    args = (abstol, reltol, matvec_max, nmv0)
    scal, flags = K.bicg_scalar(0, K.block_sums(K.Tr(r0.v * r0.v), R), scal, flags, *args)
    r, pv, v, s = r0, T(np.zeros((n, p))), T(np.zeros((n, p))), T(np.zeros((n, p)))
    for _ in range(matvec_max + 2):
        if flags[0]:
            break
        scal, flags = K.bicg_scalar(1, None, scal, flags, *args)
        pv = K.bicg_update_p(pv, r, v, scal, flags)
        q = pv if M is None else K.Tr(M * pv.v)
        v = T(A @ q.v)
        scal, flags = K.bicg_scalar(2, K.block_sums(K.Tr(r0.v * v.v), R), scal, flags, *args)
        s, part = K.bicg_update_s(s, r, v, scal, flags, R)
        scal, flags = K.bicg_scalar(3, part, scal, flags, *args)
        zz = s if M is None else K.Tr(M * s.v)
        t = T(A @ zz.v)
        scal, flags = K.bicg_scalar(4, K.bicg_dots3(t, s, r0, flags, R), scal, flags, *args)
        x, r, part = K.bicg_update_x(x, r, s, t, q, scal, flags, R, z=None if M is None else zz)
        scal, flags = K.bicg_scalar(5, part, scal, flags, *args)
    return x.v, flags


def test_bicgstab_steps_reproduce_the_stored_solutions(systems):
    x, flags = _bicgstab(systems["nonsym_T"], systems["nonsym_B"], 1e-15, 1e-13)
    assert flags[0] == 1 and rel(x, systems["nonsym_x"]) < 1e-12
    x, flags = _bicgstab(systems["S"], systems["csr_2d6_bicgstab_B"], 1e-14, 1e-12)
    assert flags[0] == 1 and rel(x, systems["csr_2d6_bicgstab_x"]) < 1e-12


@pytest.mark.parametrize("case", ["budget", "precond", "guess"])
def test_bicgstab_steps_match_the_columnwise_oracle(systems, case):
    """Per column: its own threshold, the early exit after the half step, the matvec budget, a preconditioner, an initial guess."""
    Tm, B = systems["nonsym_T"], systems["nonsym_B"].copy()
    n = Tm.shape[0]
    B[:, 1] *= 1e-3
    rows, cols = np.nonzero(Tm)
    crow, col = G.coo_to_csr_arrays(np.stack([rows, cols]), n)
    kw = dict(budget=dict(matvec_max=7), precond=dict(precond_diag=1.0 / np.diag(Tm)), guess=dict(x0=0.1 * systems["nonsym_G"]))[case]
    x, flags = _bicgstab(Tm, B, 1e-8, 1e-6, **kw)
    p = B.shape[1]
    for c in range(p):
        kwo = dict(kw)
        if "x0" in kwo:
            kwo["x0"] = kwo["x0"][:, c]
        xo, n_mv = oracle.bicgstab(crow, col, Tm[rows, cols], B[:, c].copy(), **kwo)
        assert rel(x[:, c], xo) < 1e-12, (case, c)
        assert flags[2 + 2 * p + c] == n_mv, (case, c)


# ---- the size queries and the drivers' message -----------------------------------------------------------------------------------

def _vt(dtype):
    return _backend.vtype_of(torch.empty(0, dtype=dtype))


def _geometry(p, wide):
    """(lanes per row, rows per workgroup) of an [n][p] array the way the step kernels lay it out: 16-byte lanes where p is a
    multiple of the lane width, 256 threads, four row passes; None where a row needs more than 256 lanes."""
    vec = wide if p % wide == 0 else 1
    lpr = -(-p // vec)
    return None if lpr > 256 else (lpr, (256 // lpr) * 4)


WIDTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 192, 255, 256, 257, 258, 260, 510, 512, 514, 1020, 1024, 1026, 1028, 2048]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_size_queries_across_widths(dtype):
    lib = _backend.load_library()
    vt, wide = _vt(dtype), 16 // torch.empty((), dtype=dtype).element_size()
    assert lib.tsgu_cg_fold_rows() == 256
    for p in WIDTHS:
        g = _geometry(p, wide)
        accepted = p <= 256 or (p % wide == 0 and p <= 256 * wide)
        assert (g is not None) == accepted, p
        for n in (1, 7, 1000, 100003):
            nb = lib.tsgu_cg_num_blocks(vt, n, p)
            nb2 = lib.tsgu_cg2_num_blocks(vt, n, p)
            ncd = lib.tsgu_coldot_max_blocks(n, p)
            if g is None:
                assert nb == -1 and nb2 == -1, (p, n)
            else:
                R = g[1]
                assert nb == -(-n // R), (p, n)
                if p <= 256:      # the two-launch form: as many groups of passes per workgroup as leave at most 1024 partial rows
                    groups = -(-nb // 1024)
                    assert nb2 == -(-n // (R * groups)) and nb2 <= 1024, (p, n)
                else:
                    assert nb2 == -1, (p, n)
            # the column dot sizes its partial rows for scalar lanes (the most rows it can write), and only up to 256 columns:
            # _backend.coldot walks wider operands in slabs of 256 columns
            assert ncd == (-(-n // ((256 // p) * 4)) if p <= 256 else -1), (p, n)
            if p <= 256 and g is not None:
                assert ncd >= nb


@pytest.mark.parametrize("dtype,p", [(torch.float32, 257), (torch.float32, 1026), (torch.float32, 1028), (torch.float64, 259),
                                      (torch.float64, 516), (torch.float64, 1024)])
def test_refused_width_message_states_the_rule(dtype, p):
    wide = 16 // torch.empty((), dtype=dtype).element_size()
    for who in ("linear_cg", "minres", "bicgstab"):
        with pytest.raises(RuntimeError) as err:
            _backend.krylov_num_blocks(who, torch.empty(0, dtype=dtype), 100, p)
        msg = str(err.value)
        assert msg.startswith(f"{who}: {p} simultaneous right-hand sides")
        assert "up to 256" in msg and f"multiples of {wide} up to {256 * wide}" in msg
        assert "more than 1024" not in msg


@pytest.mark.parametrize("dtype,p", [(torch.float32, 256), (torch.float32, 260), (torch.float32, 1024), (torch.float64, 258),
                                      (torch.float64, 512), (torch.float32, 255), (torch.float64, 1)])
def test_accepted_widths_get_their_block_count(dtype, p):
    wide = 16 // torch.empty((), dtype=dtype).element_size()
    R = _geometry(p, wide)[1]
    assert _backend.krylov_num_blocks("linear_cg", torch.empty(0, dtype=dtype), 1001, p) == -(-1001 // R)
