"""Float64 numpy restatement of `sparse_expm_mm`: the coefficient rule, the dense Chebyshev expansion and its adjoint, one
`tsgu_cheb_step` / `tsgu_cheb_combine` launch (csrc/tsgu_hip_expm.h) with the magnitudes the kernel test's rounding bound is built
from, and the test matrices.  No torch, no scipy."""

import math

import numpy as np


# ---- the coefficients ------------------------------------------------------------------------------------------------------------------

def ive(x, tolerance):
    """(ive_0 ... ive_M of x >= 0, K): Miller's backward recurrence f_{k-1} = f_{k+1} + (2k/x) f_k from M beyond x, normalised by
    ive_0 + 2 sum_{k>=1} ive_k = 1; K the smallest index with 2 sum_{k>K} ive_k <= tolerance."""
    if x == 0:
        return np.ones(1), 0
    M = int(x + 20.0 * max(1.0, x) ** (1.0 / 3.0) + 60.0)
    f = np.zeros(M + 2)
    f[M] = 1e-300
    for k in range(M, 0, -1):
        f[k - 1] = f[k + 1] + 2.0 * k / x * f[k]
        if f[k - 1] > 1e250:
            f *= 1e-250
    f = f[: M + 1] / (f[0] + 2.0 * f[1: M + 1].sum())
    tail = 2.0 * np.cumsum(f[::-1])[::-1]
    ok = tail <= tolerance
    K = max(int(np.argmax(ok)) - 1, 0) if ok.any() else M
    return f, K


def coefficients(t, lo, hi, tolerance, K=None):
    """(c_0 ... c_K, a, b) for the scalar time t and a spectrum in [lo, hi] (K: the rule's unless given)."""
    rho, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
    if rho == 0:
        return np.array([math.exp(t * lo)]), 0.0, 0.0
    z = t * rho
    f, k_rule = ive(abs(z), tolerance)
    K = k_rule if K is None else K
    c = np.zeros(K + 1)
    m = min(K + 1, f.size)
    c[:m] = f[:m]
    c[1:] *= 2.0
    if z < 0:
        c[1::2] *= -1.0
    return c * math.exp(t * mid + abs(z)), 1.0 / rho, -mid / rho


def chebyshev_sum(c, x):
    """sum_k c_k T_k(x) for an array x in [-1, 1] with T_k(x) = cos(k acos x): no recurrence, so no growth of its rounding."""
    theta = np.arccos(np.asarray(x, dtype=np.float64))
    return sum(ck * np.cos(k * theta) for k, ck in enumerate(c))


# ---- the dense expansion and its adjoint ---------------------------------------------------------------------------------------------------

def dense_expm(M, t):
    """exp(t M) for a symmetric M by eigh."""
    lam, V = np.linalg.eigh(M)
    return (V * np.exp(t * lam)) @ V.T


def dense_truth(M, B, G, times):
    """The exact exponential and its derivatives by eigh, for `times` of shape (T, 1) or (T, p) and G of shape (T, n, p):
    (Y (T, n, p), grad_B (n, p), dense grad_A (n, n) unsymmetrised, grad_t (T, p) per time and column) of L = sum_j <G_j, Y_j>.
    grad_A is the Daleckii-Krein formula V [(V^T g b^T V) o Phi] V^T with Phi_ab = (e^{t l_a} - e^{t l_b}) / (l_a - l_b), summed
    over times and columns — what autograd through a dense matrix exponential returns."""
    lam, V = np.linalg.eigh(M)
    T, n, p = G.shape
    times = np.broadcast_to(np.asarray(times, dtype=np.float64), (T, p))
    VB, VG = V.T @ B, np.einsum("an,jnc->jac", V.T, G)
    E = np.exp(times[:, None, :] * lam[None, :, None])                  # (T, n, p): e^{t_jc lam_a}
    Y = np.einsum("na,jac->jnc", V, E * VB[None])
    gB = np.einsum("na,jac->nc", V, E * VG)
    gt = np.einsum("jnc,jnc->jc", G, np.einsum("na,jac->jnc", V, E * lam[None, :, None] * VB[None]))
    inner = np.zeros((n, n))
    diff = lam[:, None] - lam[None, :]
    for j in range(T):
        for t in np.unique(times[j]):
            cols = times[j] == t
            d = t * diff
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(d == 0, 1.0, np.expm1(d) / np.where(d == 0, 1.0, d))
            phi = np.exp(t * lam)[None, :] * t * ratio
            inner += (VG[j][:, cols] @ VB[:, cols].T) * phi
    return Y, gB, V @ inner @ V.T, gt


def expansion(M, B, c, a, b):
    """(sum_k c_k w_k, [w_0 ... w_K]) with dense products."""
    Ah = a * M + b * np.eye(M.shape[0])
    W = [B]
    if len(c) > 1:
        W.append(Ah @ B)
    for k in range(1, len(c) - 1):
        W.append(2.0 * Ah @ W[k] - W[k - 1])
    return sum(ck * w for ck, w in zip(c, W)), W


def adjoint(M, G, c, a, b, W):
    """(grad_B = mu_0, dense grad_A = a sum_{k<K} f_k mu_{k+1} w_k^T, unsymmetrised)."""
    K = len(c) - 1
    Ah = a * M + b * np.eye(M.shape[0])
    mu = [None] * (K + 3)
    mu[K + 1] = mu[K + 2] = np.zeros_like(G)
    gA = np.zeros_like(M)
    for k in range(K, -1, -1):
        mu[k] = c[k] * G + (1.0 if k == 0 else 2.0) * Ah @ mu[k + 1] - mu[k + 2]
    for k in range(K):
        gA += (1.0 if k == 0 else 2.0) * a * mu[k + 1] @ W[k].T
    return mu[0], gA


def gershgorin(M):
    d = np.diag(M)
    r = np.abs(M).sum(axis=1) - np.abs(d)
    return float((d - r).min()), float((d + r).max())


# ---- matrices -----------------------------------------------------------------------------------------------------------------------------

def laplacian7(a, b, c):
    """The 7-point Laplacian on an a x b x c lattice (Dirichlet): positive definite, spectrum inside (0, 12)."""
    n = a * b * c
    M = np.zeros((n, n))
    for i in range(a):
        for j in range(b):
            for k in range(c):
                r = (i * b + j) * c + k
                M[r, r] = 6.0
                for ok, off in ((i > 0, -b * c), (i < a - 1, b * c), (j > 0, -c), (j < b - 1, c), (k > 0, -1), (k < c - 1, 1)):
                    if ok:
                        M[r, r + off] = -1.0
    return M


def random_symmetric(n=200, per_row=6, seed=4):
    """A random symmetric pattern with about `per_row` entries per row, indefinite, no lattice."""
    rng = np.random.default_rng(seed)
    M = np.zeros((n, n))
    count = n * (per_row - 1) // 2
    i, j = rng.integers(0, n, count), rng.integers(0, n, count)
    v = rng.standard_normal(count)
    keep = i != j
    M[np.minimum(i, j)[keep], np.maximum(i, j)[keep]] = v[keep]
    M = M + M.T
    M[np.arange(n), np.arange(n)] = rng.standard_normal(n)
    return M


MATRICES = {
    "lap6x5x4": lambda: laplacian7(6, 5, 4),          # n = 120: takes the lattice families
    "random200": random_symmetric,                     # n = 200, indefinite
    "one": lambda: np.array([[0.75]]),                 # the 1 x 1 matrix
}


def csr_arrays(M):
    n = M.shape[0]
    rows, cols = np.nonzero(M)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.add.at(crow, rows + 1, 1)
    return np.cumsum(crow), cols.astype(np.int64), M[rows, cols].astype(np.float64)


# ---- one launch ----------------------------------------------------------------------------------------------------------------------------

def step(prod, x, prev, alpha, beta, gamma, src, src_slot, chunk, slot, stop):
    """tsgu_cheb_step in float64 on float64 copies of the inputs.  Returns (new prev, new chunk or None, mag): `mag` is, per
    element of [n][p], the sum of the absolute values of the terms the element is computed from; None under a set stop word
    (nothing is written)."""
    x, prev = np.array(x, dtype=np.float64), np.array(prev, dtype=np.float64)
    chunk = None if chunk is None else np.array(chunk, dtype=np.float64)
    if stop:
        return prev, chunk, None
    new = beta * x
    mag = np.abs(beta * x)
    if gamma != 0:
        new = new - gamma * prev
        mag = mag + np.abs(gamma * prev)
    if prod is not None:
        new = new + alpha * np.array(prod, dtype=np.float64)
        mag = mag + np.abs(alpha * np.array(prod, dtype=np.float64))
    if src is not None:
        s = np.array(src, dtype=np.float64)[:, src_slot, :]
        new = new + s
        mag = mag + np.abs(s)
    if chunk is not None:
        chunk[:, slot, :] = new
    return new, chunk, mag


def combine(mode, accumulate, chunk, coef, planes, stop):
    """tsgu_cheb_combine in float64: chunk [n][m][p], coef [m][T][p], planes [T][n][p].  Returns (output, mag): mode 0 the planes,
    mode 1 the chunk; `mag` the per-element sum of the absolute terms, None under a set stop word."""
    chunk, coef, planes = (np.array(v, dtype=np.float64) for v in (chunk, coef, planes))
    if stop:
        return (planes if mode == 0 else chunk), None
    if mode == 0:
        out = np.einsum("sjc,isc->jic", coef, chunk)
        mag = np.einsum("sjc,isc->jic", np.abs(coef), np.abs(chunk))
        if accumulate:
            out, mag = out + planes, mag + np.abs(planes)
        return out, mag
    return np.einsum("sjc,jic->isc", coef, planes), np.einsum("sjc,jic->isc", np.abs(coef), np.abs(planes))


# ---- what the end-to-end tests compare ------------------------------------------------------------------------------------------------------
# A case is a dict with M, lo, hi, B (n, p), G (T, n, p), t2 (T, 1 or p), tarr (the times as the caller passes them), the truth Y,
# gB, gA (at the stored entries), gt (T, p) and S = e^{max(t lo, t hi)} as (T, p).

def make_case(M, B, G, times, lo, hi):
    n = M.shape[0]
    crow, col, _ = csr_arrays(M)
    rows = np.repeat(np.arange(n), np.diff(crow))
    tarr = np.asarray(times, dtype=np.float64)
    t2 = tarr.reshape(1, 1) if tarr.ndim == 0 else tarr.reshape(-1, 1) if tarr.ndim == 1 else tarr
    Y, gB, gA, gt = dense_truth(M, B, G, t2)
    S = np.exp(np.maximum(t2 * lo, t2 * hi))
    return dict(M=M, lo=lo, hi=hi, B=B, G=G, t2=t2, tarr=tarr, Y=Y, gB=gB, gA=gA[rows, col], gt=gt, S=np.broadcast_to(S, gt.shape))


def _like_t(c, per):
    """(T, p) figures per time and column, summed to the shape of the caller's t."""
    return per.sum() if c["tarr"].ndim == 0 else per.sum(axis=1) if c["tarr"].ndim == 1 else per


def errors(c, Y, gB, gA, gt):
    """Per quantity, the error in the norm its bound is stated in: values (T, p) column 2-norms, grad_B (p,) column 2-norms,
    grad_A the 2-norm over the stored entries, grad_t absolute, in t's shape (left out when gt is None)."""
    e = {"values": np.linalg.norm(Y - c["Y"], axis=1), "grad_B": np.linalg.norm(gB - c["gB"], axis=0),
         "grad_A": np.asarray(np.linalg.norm(gA - c["gA"]))}
    if gt is not None:
        e["grad_t"] = np.abs(gt - _like_t(c, c["gt"]))
    return e


def error_bounds(c, K, a, tolerance, factor=10.0):
    """`factor` times the truncation bounds, shaped like `errors` (derivation: the docstring of tests/test_gpu_sparse_expm.py):
    values tol S |b_c|;  grad_B sum_j tol S_j |g_jc|;  grad_t |g_jc| max(|lo|, |hi|) (value bound);
    grad_A 12 (K+1)^2 a tol sum_j S_j |G_j|_F |B|_F.  The fp64 tests allow ten times them, the fp32 floor is the bounds themselves."""
    S, B, G = c["S"], c["B"], c["G"]
    nb, ng = np.linalg.norm(B, axis=0), np.linalg.norm(G, axis=1)
    values = factor * tolerance * S * nb[None, :]
    return {"values": values, "grad_B": (factor * tolerance * S * ng).sum(axis=0),
            "grad_A": np.asarray(factor * 12.0 * (K + 1) ** 2 * a * tolerance
                                 * (S.max(axis=1) * np.linalg.norm(G.reshape(G.shape[0], -1), axis=1)).sum() * np.linalg.norm(B)),
            "grad_t": _like_t(c, ng * max(abs(c["lo"]), abs(c["hi"])) * values)}
