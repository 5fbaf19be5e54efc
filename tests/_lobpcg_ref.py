"""numpy restatement of utils/lobpcg.py and what the LOBPCG tests share: the matrices, the float64 spectra, the criteria.

`lobpcg` is the recurrence of the package written on dense numpy arrays: the tall-skinny products (Gram matrices, block
recombinations, residual) in the WORKING dtype, the Rayleigh–Ritz problem in float64 — the same split as the package's.  It
imports nothing from the package.  The pattern builders are those of tests/_fsai_ref.py."""

import math

import numpy as np

from _fsai_ref import band, dense, dominant_values, random_pattern, stencil  # noqa: F401  (shared with the tests)


# ---- matrices -----------------------------------------------------------------------------------------------------------------

def laplacian_values(ptr, idx):
    """Graph Laplacian + boundary of a pattern: the diagonal = (entries of a full interior row − 1), off-diagonal −1."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    full = int(np.diff(ptr).max()) - 1
    return np.where(idx == rows, float(full), -1.0)


def path_case():
    """Path graph Laplacian, n = 64: eigenvalues 2 − 2cos(jπ / (n + 1)); the smallest ones have small gaps."""
    ptr, idx = band(64, 1)
    return ptr, idx, laplacian_values(ptr, idx)


def stencil7_case():
    ptr, idx = stencil(8, 8, 8, 7)
    return ptr, idx, laplacian_values(ptr, idx)


def stencil27_case():
    ptr, idx = stencil(6, 5, 4, 27)
    return ptr, idx, dominant_values(ptr, idx, seed=5, symmetric=True)


def random_case():
    ptr, idx = random_pattern(300, 8, seed=11)
    return ptr, idx, dominant_values(ptr, idx, seed=12, symmetric=True)


def coupled_case(n=200, coupling=0.05):
    """diag(1 … n) + weak coupling of neighbours: all gaps are close to 1."""
    ptr, idx = band(n, 1)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    return ptr, idx, np.where(idx == rows, rows + 1.0, coupling)


# name -> (builder, k)
CASES = {"path": (path_case, 3), "stencil7": (stencil7_case, 4), "stencil27": (stencil27_case, 3), "random": (random_case, 3),
         "coupled": (coupled_case, 3)}
# about twice the iterations the restatement needs at most over the cases, both dtypes and both ends (194: the smallest pairs of
# the 27-point case in float64; tests/test_sparse_lobpcg_cpu.py checks that it converges on every case within half of this)
NITER = 400
# a scaled Cholesky pivot below PIVOT_FLOOR·sqrt(u) counts as a breakdown (utils/lobpcg.py: the same number)
PIVOT_FLOOR = 32.0

_BUILT = {}


def case(name):
    """(ptr, idx, val float64, k, dense float64 matrix, ascending float64 spectrum) of a named case, built once."""
    if name not in _BUILT:
        build, k = CASES[name]
        ptr, idx, val = build()
        D = dense(ptr, idx, val)
        assert np.array_equal(D, D.T)
        _BUILT[name] = (ptr, idx, val, k, D, np.linalg.eigvalsh(D))
    return _BUILT[name]


def initial_block(n, k, seed=3):
    return np.random.default_rng(seed).standard_normal((n, k))


def wanted(spectrum, k, largest):
    return spectrum[::-1][:k] if largest else spectrum[:k]


# ---- the recurrence -----------------------------------------------------------------------------------------------------------

def _scaled_cholesky(G, floor):
    d = np.diag(G)
    if not np.all(np.isfinite(G)) or not np.all(d > 0):
        return None
    s = 1.0 / np.sqrt(d)
    Gs = G * s[:, None] * s[None, :]
    try:
        L = np.linalg.cholesky((Gs + Gs.T) * 0.5)
    except np.linalg.LinAlgError:
        return None
    if np.diag(L).min() < floor:
        return None
    return s, np.linalg.inv(L)


def _rayleigh_ritz(GS, GA, k, floor):
    got = _scaled_cholesky(GS, floor)
    if got is None:
        return None
    s, Li = got
    GAs = GA * s[:, None] * s[None, :]
    M = Li @ ((GAs + GAs.T) * 0.5) @ Li.T
    w, Z = np.linalg.eigh((M + M.T) * 0.5)
    return w[:k], s[:, None] * (Li.T @ Z[:, :k])


def lobpcg(A, X0, largest=True, niter=500, tol=None, dtype=np.float64, precondition=None):
    """(eigenvalues (k,), eigenvectors (n, k), info) for the dense symmetric `A`: utils/lobpcg.py on numpy arrays of `dtype`."""
    A = np.asarray(A, dtype=dtype)
    sign = -1.0 if largest else 1.0
    u = np.finfo(dtype).eps
    tol = math.sqrt(u) if tol is None else tol
    floor = PIVOT_FLOOR * math.sqrt(u)
    n, k = X0.shape
    f64 = lambda M: np.asarray(M, dtype=np.float64)          # noqa: E731
    wd = lambda M: np.asarray(M, dtype=dtype)                # noqa: E731
    product = lambda V: wd(sign * (A @ V))                   # noqa: E731
    X0 = wd(X0)
    s, Li = _scaled_cholesky(f64(X0.T @ X0), floor)
    X = wd(X0 @ wd(s[:, None] * Li.T))
    AX = product(X)
    a_norm = math.sqrt(float(np.sum(np.diag(f64(AX.T @ AX)))) / k)
    lam, C = _rayleigh_ritz(np.eye(k), f64(X.T @ AX), k, floor)
    X, AX = wd(X @ wd(C)), wd(AX @ wd(C))
    lam = wd(lam)
    P = AP = None
    info = dict(iterations=0, converged=False, restarts=0, breakdown=False, a_norm=a_norm, tolerance=tol)
    it = 0
    while True:
        R = wd(AX - wd(X * lam))
        norms = np.sqrt(np.sum(f64(R * R), axis=0))
        info.update(iterations=it, residual_norms=norms)
        if np.all(norms <= tol * a_norm):
            info["converged"] = True
            break
        if it >= niter:
            break
        W = R if precondition is None else wd(precondition(R))
        for _ in range(2):
            W = wd(W - X @ wd(X.T @ W))
        got = _scaled_cholesky(f64(W.T @ W), 0.0)
        if got is None:
            info["breakdown"] = True
            break
        sw, Lw = got
        W = wd(W @ wd(sw[:, None] * Lw.T))
        AW = product(W)
        S = np.concatenate([X, W] + ([P] if P is not None else []), axis=1)
        AS = np.concatenate([AX, AW] + ([AP] if P is not None else []), axis=1)
        GS, GA = f64(wd(S.T @ S)), f64(wd(S.T @ AS))
        m = S.shape[1]
        sel = list(range(2 * k)) + [2 * k + j for j in range(k) if P is not None and not norms[j] <= tol * a_norm]       # (soft locking)
        got = _rayleigh_ritz(GS[np.ix_(sel, sel)], GA[np.ix_(sel, sel)], k, floor)
        if got is None and len(sel) > 2 * k:
            info["restarts"] += 1
            sel = sel[: 2 * k]
            got = _rayleigh_ritz(GS[np.ix_(sel, sel)], GA[np.ix_(sel, sel)], k, floor)
        if got is None:
            info["breakdown"] = True
            break
        lam64 = got[0]
        C = np.zeros((m, k))
        C[sel] = got[1]
        C = wd(C)
        Cp = C.copy()
        Cp[:k] = 0
        X, AX, P, AP = wd(S[:, :m] @ C), wd(AS[:, :m] @ C), wd(S[:, :m] @ Cp), wd(AS[:, :m] @ Cp)
        lam = wd(lam64)
        it += 1
    return wd(sign * lam) if largest else lam, X, info


def unit_roundoff(dtype):
    """u of the bounds: half the spacing of the floats at 1 (2^-24, 2^-53)."""
    return float(np.finfo(dtype).eps) / 2


# ---- criteria -----------------------------------------------------------------------------------------------------------------

def pair_residuals(D, lam, V):
    """‖A·x_j − λ_j·x_j‖₂ / ‖x_j‖₂ per returned pair, in float64."""
    lam, V = np.asarray(lam, dtype=np.float64), np.asarray(V, dtype=np.float64)
    return np.linalg.norm(D @ V - V * lam, axis=0) / np.linalg.norm(V, axis=0)


def eigenvalue_bounds(D, spectrum, lam, V, largest, u):
    """(|λ̂_j − λ_j|, ‖A·x̂_j − λ̂_j·x̂_j‖₂ / ‖x̂_j‖₂ + n·u·‖A‖₂) per pair: the residual bound for symmetric matrices."""
    n = D.shape[0]
    k = len(lam)
    err = np.abs(np.asarray(lam, dtype=np.float64) - wanted(spectrum, k, largest))
    return err, pair_residuals(D, lam, V) + n * u * max(abs(spectrum[0]), abs(spectrum[-1]))


def orthonormality(V):
    V = np.asarray(V, dtype=np.float64)
    return float(np.abs(V.T @ V - np.eye(V.shape[1])).max())


def gaps(spectrum, k, largest):
    """Distance of each wanted eigenvalue to the rest of the spectrum."""
    order = spectrum[::-1] if largest else spectrum
    out = []
    for j in range(k):
        others = np.delete(order, j)
        out.append(np.abs(others - order[j]).min())
    return np.array(out)
