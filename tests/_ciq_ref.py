"""Float64 numpy restatement of the contour-quadrature rule of `sparse_inv_sqrt_mm` and of one `tsgu_ciq_update` / `tsgu_ciq_stop`
step (csrc/tsgu_hip_ciq.h), with the magnitudes the kernel test's rounding bound is built from.  No torch, no scipy."""

import math

import numpy as np


# ---- the rule (Hale, Higham, Trefethen 2008, method 3) --------------------------------------------------------------------------------

def agm(m):
    """AGM scale of parameter m: lists a, c with a[0] = 1, b[0] = sqrt(1 - m), c[0] = sqrt(m) (Abramowitz and Stegun 16.4)."""
    a, b, c = [1.0], [math.sqrt(1.0 - m)], [math.sqrt(m)]
    while abs(c[-1]) > 1e-17 * a[-1] and len(a) < 64:
        a_new, b_new, c_new = 0.5 * (a[-1] + b[-1]), math.sqrt(a[-1] * b[-1]), 0.5 * (a[-1] - b[-1])
        a.append(a_new)
        b.append(b_new)
        c.append(c_new)
    return a, c


def ellipk(m):
    return math.pi / (2.0 * agm(m)[0][-1])


def ellipj(u, m):
    a, c = agm(m)
    n = len(a) - 1
    phi = (2.0 ** n) * a[n] * np.asarray(u, dtype=np.float64)
    for j in range(n, 0, -1):
        phi = 0.5 * (phi + np.arcsin(np.clip(c[j] * np.sin(phi) / a[j], -1.0, 1.0)))
    sn, cn = np.sin(phi), np.cos(phi)
    return sn, cn, np.sqrt(cn * cn + (1.0 - m) * sn * sn)


def rule(lo, hi, N, functions=None):
    """(sigma, omega) for a spectrum in [lo, hi]; `functions` = (ellipk, ellipj) replaces the elliptic functions (scipy's, in the
    test that compares against them)."""
    K, J = functions or (ellipk, ellipj)
    mp = 1.0 - lo / hi
    Kp = float(K(mp))
    u = (np.arange(1, N + 1, dtype=np.float64) - 0.5) * Kp / N       # the formula as written: u_q = (q - 1/2) K' / N
    sn, cn, dn = J(u, mp)[:3]
    return lo * sn ** 2 / cn ** 2, 2.0 * Kp * math.sqrt(lo) / (math.pi * N) * dn / cn ** 2


def apply_scalar(sigma, omega, lam):
    """r(lam) = sum_q omega_q / (lam + sigma_q) for an array of lam."""
    lam = np.asarray(lam, dtype=np.float64)
    return (omega[None, :] / (lam[:, None] + sigma[None, :])).sum(axis=1)


def scalar_error(sigma, omega, lam):
    """max |r(lam) sqrt(lam) - 1| over the array lam."""
    lam = np.asarray(lam, dtype=np.float64)
    return float(np.abs(apply_scalar(sigma, omega, lam) * np.sqrt(lam) - 1.0).max())


# ---- matrices ---------------------------------------------------------------------------------------------------------------------------

def laplacian5(a, b, shift):
    n = a * b
    M = np.zeros((n, n))
    for i in range(a):
        for j in range(b):
            r = i * b + j
            M[r, r] = 4.0 + shift
            if i > 0:
                M[r, r - b] = -1.0
            if i < a - 1:
                M[r, r + b] = -1.0
            if j > 0:
                M[r, r - 1] = -1.0
            if j < b - 1:
                M[r, r + 1] = -1.0
    return M


def laplacian7(a, b, c, shift):
    n = a * b * c
    M = np.zeros((n, n))
    for i in range(a):
        for j in range(b):
            for k in range(c):
                r = (i * b + j) * c + k
                M[r, r] = 6.0 + shift
                if i > 0:
                    M[r, r - b * c] = -1.0
                if i < a - 1:
                    M[r, r + b * c] = -1.0
                if j > 0:
                    M[r, r - c] = -1.0
                if j < b - 1:
                    M[r, r + c] = -1.0
                if k > 0:
                    M[r, r - 1] = -1.0
                if k < c - 1:
                    M[r, r + 1] = -1.0
    return M


MATRICES = {
    "lap6x7": lambda: laplacian5(6, 7, 0.3),            # n = 42, spectrum [0.6503, 7.9497]
    "lap4x5x3": lambda: laplacian7(4, 5, 3, 0.1),       # n = 60
}
LARGE = {"lap12x11x10": lambda: laplacian7(12, 11, 10, 0.1)}   # n = 1320: more than one workgroup


def csr_arrays(M):
    n = M.shape[0]
    rows, cols = np.nonzero(M)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.add.at(crow, rows + 1, 1)
    return np.cumsum(crow), cols.astype(np.int64), M[rows, cols].astype(np.float64)


def dense_power(M, power):
    """(M^power, eigenvalues) by eigh."""
    lam, V = np.linalg.eigh(M)
    return (V * lam ** power) @ V.T, lam


def grad_a_dense(M, B, G, sigma, omega):
    """The issue's gradient formula with dense solves: -sum_q omega_q X^g_q (X^b_q)^T, a dense (n, n) array (unsymmetrised)."""
    n = M.shape[0]
    out = np.zeros((n, n))
    for s, w in zip(sigma, omega):
        inv = np.linalg.inv(M + s * np.eye(n))
        out -= w * (inv @ G) @ (inv @ B).T
    return out


# ---- one update step ---------------------------------------------------------------------------------------------------------------------

def update_step(zc, zp, wpp, wp, acc, keep, scal, omega, done, stop):
    """tsgu_ciq_update in float64 on float64 copies of the inputs: zc, zp, acc [n][p]; wpp, wp [S][n][p]; keep [n][S][p] or None;
    scal [S][12][p]; omega [S]; done [p]; stop: flags[0].  Returns (outputs, magnitudes): dicts with keys z, w, acc, keep — the
    magnitudes are, per element, the sum of the absolute values of the terms the element is computed from (what a rounding is
    relative to); they are 0 where the kernel must leave the element untouched."""
    zc, zp, wpp, wp, acc, scal, omega = (np.array(x, dtype=np.float64) for x in (zc, zp, wpp, wp, acc, scal, omega))
    keep = None if keep is None else np.array(keep, dtype=np.float64)
    out = {"z": zc.copy(), "w": wpp.copy(), "acc": acc.copy(), "keep": None if keep is None else keep.copy()}
    mag = {k: (None if v is None else np.zeros_like(v)) for k, v in out.items()}
    if stop:
        return out, mag
    S = omega.size
    live = np.asarray(done) == 0
    beta = scal[0, 1][None, :]
    out["z"] = zc / beta
    mag["z"] = np.abs(out["z"])
    t = np.zeros_like(acc)
    t_mag = np.zeros_like(acc)
    for q in range(S):
        sub, subsub, diag, scale = scal[q, 7][None, :], scal[q, 8][None, :], scal[q, 9][None, :], scal[q, 10][None, :]
        terms = (np.abs(zp) + np.abs(sub * wp[q]) + np.abs(subsub * wpp[q])) / np.abs(diag)
        wc = ((zp - sub * wp[q]) - subsub * wpp[q]) / diag
        up = wc * scale
        out["w"][q][:, live] = wc[:, live]
        mag["w"][q][:, live] = terms[:, live]
        t += omega[q] * up
        t_mag += np.abs(omega[q]) * terms * np.abs(scale)
        if keep is not None:
            out["keep"][:, q, :][:, live] = (keep[:, q, :] + up)[:, live]
            mag["keep"][:, q, :][:, live] = (np.abs(keep[:, q, :]) + terms * np.abs(scale))[:, live]
    out["acc"][:, live] = (acc + t)[:, live]
    mag["acc"][:, live] = (np.abs(acc) + t_mag)[:, live]
    return out, mag


def stop_step(scal, tol, est, done, flags):
    """tsgu_ciq_stop: returns (est, done, flags) after the launch."""
    scal = np.asarray(scal)
    est, done, flags = np.array(est), np.array(done), np.array(flags)
    if flags[0] != 0:
        return est, done, flags
    a = np.abs(scal[:, 6, :])
    with np.errstate(invalid="ignore"):
        m = np.where(np.isnan(a).any(axis=0), np.nan, np.nanmax(np.where(np.isnan(a), -np.inf, a), axis=0))
        new_done = ((done != 0) | (m <= tol)).astype(done.dtype)
    flags[0] = 1 if new_done.all() else 0
    return m.astype(est.dtype), new_done, flags
