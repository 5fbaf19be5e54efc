"""The least-squares problems of the LSMR tests (tests/test_gpu_lsmr.py, tests/test_lsmr_cpu.py).

`tall(n, dmin)` is a (3n, n) matrix: a diagonal block graded from `dmin` to 4 on top of a (2n, n) band of five entries per row,
uniform in [-0.1, 0.1].  Its Gram matrix is D² + BᵀB with ‖B‖ ≤ 0.5, so its singular values lie in [dmin, sqrt(16.25)] and the
condition number is 4 / dmin up to the band: dmin sets the conditioning.  For n = 192 (seed 0):
  dmin = 0.4   cond = 9.3   the problems of the accuracy and column tests
  dmin = 0.1   cond = 25    the long solve: more than 100 iterations to atol = btol = 1e-12 (tests/test_lsmr_cpu.py checks both)"""

import numpy as np
import torch

N = 192
DMIN, DMIN_LONG = 0.4, 0.1


def tall(n=N, dmin=DMIN, seed=0):
    """Dense float64 (3n, n)."""
    rng = np.random.default_rng(seed)
    A = np.zeros((3 * n, n))
    A[np.arange(n), np.arange(n)] = np.linspace(dmin, 4.0, n)
    i = np.arange(2 * n)
    for j in range(5):
        A[n + i, (i // 2 + j) % n] = 0.1 * rng.uniform(-1.0, 1.0, 2 * n)
    return torch.from_numpy(A)


def rhs(m, k, seed=1):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((m, k)))


def cond(A):
    s = torch.linalg.svdvals(A)
    return float(s[0] / s[-1])


def dense_lstsq(A, B, damp=0.0):
    """argmin ‖(A; damp·I) x − (B; 0)‖ in float64."""
    n = A.shape[1]
    if damp:
        A = torch.cat([A, damp * torch.eye(n, dtype=A.dtype)])
        B = torch.cat([B, torch.zeros((n, B.shape[1]), dtype=B.dtype)])
    return torch.linalg.lstsq(A, B, driver="gelsd").solution


def _rot(a, b):
    r = np.hypot(a, b)
    safe = np.where(r > 0, r, 1.0)
    return a / safe, b / safe, r


def _ratio(num, den):
    return np.where(den != 0, num / np.where(den != 0, den, 1.0), 0.0)


def ref_scalar(phase, sums, scal, flags, damp, atol, btol, ctol, eps):
    """One launch of tsgu_lsmr_scalar in float64 numpy, from the column sums it folds: (scal, flags) after it, as
    include/tsgu_hip_lsmr.h states the phases (the recurrences are those of utils/lsmr.py's host-driven loop)."""
    S, F = scal.copy(), flags.copy()
    p = S.shape[1]
    if F[0]:
        return S, F
    done, norm = F[2:2 + p] != 0, np.sqrt(np.maximum(sums, 0.0))
    if phase == 0:
        beta, alpha = norm, S[0]
        S[1] = beta
        S[22] = _ratio(1.0, beta)
        S[23] = np.where(beta > 0, _ratio(beta, alpha), -1.0)
    elif phase == 1:
        beta = S[1]
        alpha = np.where(beta > 0, norm, S[0])
        chat, shat, alphahat = _rot(S[2], np.full(p, damp))
        rhoold, rhobarold, zetaold = S[3].copy(), S[4].copy(), S[7].copy()
        c, s, rho = _rot(alphahat, beta)
        thetanew, S[2] = s * alpha, c * alpha
        thetabar, rhotemp = S[6] * rho, S[5] * rho
        S[5], S[6], S[4] = _rot(rhotemp, thetanew)
        S[7], S[8] = S[5] * S[8], -S[6] * S[8]
        S[24] = _ratio(thetabar * rho, rhoold * rhobarold)
        S[25] = np.where(done, 0.0, _ratio(S[7], rho * S[4]))
        S[26] = _ratio(thetanew, rho)
        S[27] = np.where(alpha > 0, alpha, 1.0)
        betaacute, betacheck = chat * S[9], -shat * S[9]
        betahat, S[9] = c * betaacute, -s * betaacute
        thetatildeold = S[13].copy()
        ct, st, rhotildeold = _rot(S[11], thetabar)
        S[13], S[11] = st * S[4], ct * S[4]
        S[10] = -st * S[10] + ct * betahat
        S[12] = (zetaold - thetatildeold * S[12]) / np.where(rhotildeold != 0, rhotildeold, 1.0)
        taud = (S[7] - S[13] * S[12]) / np.where(S[11] != 0, S[11], 1.0)
        S[14] = S[14] + betacheck ** 2
        S[19] = np.sqrt(S[14] + (S[10] - taud) ** 2 + S[9] ** 2)
        S[15] = S[15] + beta ** 2
        S[20] = np.sqrt(S[15])
        S[15] = S[15] + alpha ** 2
        S[16] = np.maximum(S[16], rhobarold)
        if F[1] + 1 > 1:
            S[17] = np.minimum(S[17], rhobarold)
        with np.errstate(divide="ignore"):
            S[21] = np.maximum(S[16], rhotemp) / np.minimum(S[17], rhotemp)
        S[0], S[3] = alpha, rho
        S[22], S[23] = _ratio(1.0, alpha), _ratio(alpha, beta)
        F[2 + p:] = np.where(done, F[2 + p:], F[1] + 1)
        F[1] += 1
    else:
        normb = np.where(S[18] > 0, S[18], 1.0)
        test1, test2, test3 = S[19] / normb, np.abs(S[8]) / (S[20] * S[19] + eps), 1.0 / (S[21] + eps)
        t1 = test1 / (1.0 + S[20] * norm / normb)
        rtol = btol + atol * S[20] * norm / normb
        stop = (1 + test3 <= 1) | (1 + test2 <= 1) | (1 + t1 <= 1) | (test3 <= ctol) | (test2 <= atol) | (test1 <= rtol)
        F[2:2 + p] = done | stop
        F[0] = int(np.all(F[2:2 + p] != 0))
    return S, F


def ref_vector(which, scal, y, a1, h=None, hbar=None):
    """One launch of tsgu_lsmr_vector in float64 numpy: (outputs, error bound of each in units of the value type's u).
    BIDIAG: y <- s_prod a1 - s_self y.  UPDATE (y = x, a1 = v~): hbar, x, h.  A bound counts one rounding per operation of the
    contract and one for a coefficient rounded to the value type: three on the longest path of every output, plus what hbar's
    error contributes to x."""
    if which == 0:
        t1, t2 = scal[22] * a1, scal[23] * y
        return (t1 - t2,), (3 * (np.abs(t1) + np.abs(t2)),)
    t = scal[24] * hbar
    hb, e_hb = h - t, 3 * (np.abs(h) + np.abs(t))
    step = scal[25] * hb
    x = np.where(scal[25] != 0, y + step, y)
    e_x = np.where(scal[25] != 0, np.abs(scal[25]) * e_hb + 3 * (np.abs(y) + np.abs(step)), 0.0)
    q, t = a1 / scal[27], scal[26] * h
    return (x, q - t, hb), (e_x, 3 * (np.abs(q) + np.abs(t)), e_hb)


def relerr(x, X):
    return float((x.double().cpu().reshape(X.shape) - X).norm() / X.norm())
