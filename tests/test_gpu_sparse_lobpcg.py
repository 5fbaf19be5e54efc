"""sparse_lobpcg on the GPU: the three tall-skinny kernels through `_backend` against extended-precision references computed
from the rounded inputs (bounds that hold for any summation order), their bit-stability across workgroup counts, and the public
API with the criteria of tests/test_sparse_lobpcg_cpu.py, preconditioned runs and the count of device→host reads."""

import warnings

import numpy as np
import pytest
import torch

import _lobpcg_ref as lr
import test_sparse_lobpcg_cpu as cpu
import torchsparsegradutils_amd as tsgu
from torchsparsegradutils_amd import _backend, sparse_lobpcg, utils

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NS = (1, 63, 64, 65, 1025, 4099)
ROWS, FOLD = 2048, 256                     # rows of a chunk, partials one fold level takes (csrc/lobpcg_impl.h)
N_TWO_LEVELS = (FOLD + 1) * ROWS + 3       # more chunks than the fold's first stage takes at once
DT = {"float32": (torch.float32, np.float64), "float64": (torch.float64, np.longdouble)}       # (dtype, the reference's precision)


def unit(dtype):
    return float(torch.finfo(dtype).eps) / 2


def gamma(m, u):
    return m * u / (1 - m * u)


def view(n, w, wide, dtype, seed):
    """An (n, w) operand: contiguous (ld = w), or the middle block of an (n, 3w) allocation (ld = 3w)."""
    g = torch.Generator().manual_seed(seed)
    full = torch.randn((n, 3 * w if wide else w), generator=g, dtype=torch.float64).to(dtype).to(DEV)
    return full[:, w:2 * w] if wide else full


def ext(t, ref):
    return t.cpu().numpy().astype(ref)


def test_geometry_matches_the_constants():
    assert _backend.tall_geometry(torch.float32)[:3] == (32, 96, ROWS)


# ---- tall_gram ------------------------------------------------------------------------------------------------------------------

def check_gram(Y, Z, ref):
    u = unit(Y.dtype)
    n = Y.size(0)
    C = _backend.tall_gram(Y, Z)
    again = _backend.tall_gram(Y, Z)
    one = _backend.tall_gram(Y, Z, workgroups=1)
    three = _backend.tall_gram(Y, Z, workgroups=3)
    assert torch.equal(C, again) and torch.equal(C, one) and torch.equal(C, three), "bits depend on the call or the workgroup count"
    Ye, Ze = ext(Y, ref), ext(Z, ref)
    err = np.abs(ext(C, ref) - Ye.T @ Ze)
    bound = gamma(n, u) * (np.abs(Ye).T @ np.abs(Ze))
    assert np.all(err <= bound), (n, tuple(Y.shape), tuple(Z.shape), float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("a,b", [(1, 1), (3, 5), (16, 16), (17, 33), (48, 96), (96, 96)])
@pytest.mark.parametrize("dt", list(DT))
def test_tall_gram_within_the_any_order_bound(dt, a, b):
    dtype, ref = DT[dt]
    for n in NS:
        for wide in (False, True):
            check_gram(view(n, a, wide, dtype, 1), view(n, b, not wide, dtype, 2), ref)


@pytest.mark.parametrize("dt", list(DT))
def test_tall_gram_of_an_operand_with_itself(dt):
    dtype, ref = DT[dt]
    for n, w, wide in ((65, 17, False), (4099, 96, True), (1025, 48, True)):
        Y = view(n, w, wide, dtype, 3)
        check_gram(Y, Y, ref)
        assert torch.equal(_backend.tall_gram(Y, Y), _backend.tall_gram(Y, Y.clone()))
    S = view(4099, 32, False, dtype, 4)         # the loop's shape: a (n, 3k) basis, whole and by its leading blocks
    check_gram(S[:, :24], S[:, :24], ref)


@pytest.mark.parametrize("dt", list(DT))
def test_tall_gram_folds_in_two_levels(dt):
    dtype, ref = DT[dt]
    check_gram(view(N_TWO_LEVELS, 3, False, dtype, 5), view(N_TWO_LEVELS, 5, False, dtype, 6), ref)


# ---- tall_combine ---------------------------------------------------------------------------------------------------------------

def check_combine(n, widths_in, widths_out, dtype, ref, null=(), betas=None, wide=True, seed=0, key=lambda t, i: (t, i)):
    """`key(t, i)`: slots with one key share one coefficient matrix (the entry holds at most six distinct ones)."""
    u = unit(dtype)
    g = torch.Generator().manual_seed(seed)
    ins = [view(n, w, wide, dtype, 10 + i) for i, w in enumerate(widths_in)]
    outs = [view(n, w, wide, dtype, 30 + t) for t, w in enumerate(widths_out)]
    before = [o.clone() for o in outs]
    made = {}

    def matrix(t, i):
        if key(t, i) not in made:
            made[key(t, i)] = torch.randn((widths_in[i], widths_out[t]), generator=g, dtype=torch.float64).to(dtype).to(DEV)
        return made[key(t, i)]

    coefs = [[None if (t, i) in null else matrix(t, i) for i in range(len(widths_in))] for t in range(len(widths_out))]
    _backend.tall_combine(ins, outs, coefs, betas=betas)
    first = [o.clone() for o in outs]
    for o, b in zip(outs, before):
        o.copy_(b)
    _backend.tall_combine(ins, outs, coefs, betas=betas, workgroups=2)
    for t, wo in enumerate(widths_out):
        assert torch.equal(outs[t], first[t]), "bits depend on the workgroup count"
        want = np.zeros((n, wo), dtype=ref)
        mag = np.zeros((n, wo), dtype=ref)
        m = 0
        if betas is not None and betas[t] != 0:
            want += ref(betas[t]) * ext(before[t], ref)
            mag += abs(betas[t]) * np.abs(ext(before[t], ref))
            m += 2
        for i, c in enumerate(coefs[t]):
            if c is not None:
                want += ext(ins[i], ref) @ ext(c, ref)
                mag += np.abs(ext(ins[i], ref)) @ np.abs(ext(c, ref))
                m += widths_in[i]
        err = np.abs(ext(outs[t], ref) - want)
        assert np.all(err <= gamma(max(m, 1), u) * mag), (n, widths_in, widths_out, t, float(err.max()))


@pytest.mark.parametrize("w", [1, 8, 17, 32])
@pytest.mark.parametrize("dt", list(DT))
def test_tall_combine_within_the_bound(dt, w):
    dtype, ref = DT[dt]
    for n in NS:
        check_combine(n, [w], [w], dtype, ref, wide=n % 2 == 0)
        check_combine(n, [w] * 3, [w], dtype, ref, null=((0, 1),))
        # the loop's last step: six blocks in, four out, the coefficient slots of X', A·X', P', A·P'
        null = [(0, i) for i in (3, 4, 5)] + [(1, i) for i in (0, 1, 2)] + [(2, i) for i in (0, 3, 4, 5)] + [(3, i) for i in (0, 1, 2, 3)]
        check_combine(n, [w] * 6, [w] * 4, dtype, ref, null=tuple(null), key=lambda t, i: i % 3)
        check_combine(n, [w], [w], dtype, ref, betas=[1.0])
        check_combine(n, [w, w], [w, w], dtype, ref, betas=[-0.5, 0.0], null=((1, 0),))


@pytest.mark.parametrize("dt", list(DT))
def test_tall_combine_of_mixed_widths_and_shared_coefficients(dt):
    dtype, ref = DT[dt]
    check_combine(4099, [3, 32, 17], [5, 32], dtype, ref)
    # the same matrix in two slots is held once: six inputs and four outputs fit with three distinct matrices
    n, w = 1025, 32
    S, AS, O = (torch.randn((n, 3 * w), dtype=torch.float64).to(dtype).to(DEV) for _ in range(3))
    O2 = torch.zeros_like(O)
    middle = O[:, w:2 * w].clone()
    blk = lambda T, j: T[:, j * w:(j + 1) * w]          # noqa: E731
    C = torch.randn((3 * w, w), dtype=torch.float64).to(dtype).to(DEV)
    Cb = [C[j * w:(j + 1) * w] for j in range(3)]
    none = [None] * 3
    ins = [blk(S, j) for j in range(3)] + [blk(AS, j) for j in range(3)]
    _backend.tall_combine(ins, [blk(O, 0), blk(O2, 0), blk(O, 2), blk(O2, 2)], [Cb + none, none + Cb, [None] + Cb[1:] + none, none + [None] + Cb[1:]])
    Se, ASe, Ce = ext(S, ref), ext(AS, ref), ext(C, ref)
    Cp = Ce.copy()
    Cp[:w] = 0
    u = unit(dtype)
    for got, want, mag in ((blk(O, 0), Se @ Ce, np.abs(Se) @ np.abs(Ce)), (blk(O2, 0), ASe @ Ce, np.abs(ASe) @ np.abs(Ce)),
                           (blk(O, 2), Se @ Cp, np.abs(Se) @ np.abs(Cp)), (blk(O2, 2), ASe @ Cp, np.abs(ASe) @ np.abs(Cp))):
        assert np.all(np.abs(ext(got, ref) - want) <= gamma(3 * w, u) * mag)
    assert torch.equal(blk(O, 1), middle), "a block between two outputs was written"


def test_tall_combine_refuses_aliasing():
    S = torch.randn((100, 24), device=DEV)
    C = torch.randn((8, 8), device=DEV)
    X, W, P = S[:, :8], S[:, 8:16], S[:, 16:]
    _backend.tall_combine([X], [W], [[C]])                                # blocks of one allocation do not alias
    with pytest.raises(RuntimeError, match="tsgu_tall_combine failed"):
        _backend.tall_combine([X], [X], [[C]])
    with pytest.raises(RuntimeError, match="tsgu_tall_combine failed"):
        _backend.tall_combine([X], [S[:, 4:12]], [[C]])
    with pytest.raises(RuntimeError, match="tsgu_tall_combine failed"):
        _backend.tall_combine([X], [W, W], [[C], [C]])
    with pytest.raises(RuntimeError, match="tsgu_tall_combine failed"):
        _backend.tall_combine([P], [P], [[C]], betas=[1.0])                # (beta reads the output: it still is no input)


# ---- lobpcg_residual ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 17, 32])
@pytest.mark.parametrize("dt", list(DT))
def test_lobpcg_residual(dt, k):
    dtype, ref = DT[dt]
    u = unit(dtype)
    for n in NS + ((N_TWO_LEVELS,) if k == 1 else ()):
        AX, X = view(n, k, n % 2 == 0, dtype, 7), view(n, k, n % 2 == 1, dtype, 8)
        lam = torch.randn(k, dtype=torch.float64).to(dtype).to(DEV)
        R, ss = _backend.lobpcg_residual(AX, X, lam)
        R1, ss1 = _backend.lobpcg_residual(AX, X, lam, workgroups=1)
        R3, ss3 = _backend.lobpcg_residual(AX, X, lam, workgroups=3)
        assert torch.equal(R, R1) and torch.equal(R, R3) and torch.equal(ss, ss1) and torch.equal(ss, ss3)
        AXe, Xe, le = ext(AX, ref), ext(X, ref), ext(lam, ref)
        err = np.abs(ext(R, ref) - (AXe - Xe * le))
        assert np.all(err <= 2 * u * (np.abs(AXe) + np.abs(Xe) * np.abs(le))), (n, k, float(err.max()))
        Re = ext(R, ref)
        exact = (Re * Re).sum(axis=0)
        assert np.all(np.abs(ext(ss, ref) - exact) <= gamma(n, u) * exact), (n, k)


# ---- the public API -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_eigenvalues_orthonormality_and_agreement_with_the_cpu_path(name, dt, largest):
    """The eigenvalue criterion and the orthonormality allowance of the CPU tests on cuda:0, and the two paths against each other
    within the sum of their residual bounds (iterates are not compared: the summation orders differ)."""
    lam, V, info = cpu.solved(name, dt, largest, "csr", torch.int64, DEV)
    err, bound = cpu.check_pairs(name, dt, largest, lam, V, info)
    k = lr.CASES[name][1]
    u = lr.unit_roundoff(cpu.DTYPES[dt][1])
    got, ref = lr.orthonormality(V), lr.orthonormality(cpu.restated(name, dt, largest)[1])
    print(f"orthonormality: GPU path {got:.3e}, restatement {ref:.3e}")
    assert got <= 4 * ref + k * u
    lam_c, V_c, _ = cpu.solved(name, dt, largest)
    _, _, _, _, D, spectrum = lr.case(name)
    bound_c = lr.eigenvalue_bounds(D, spectrum, lam_c, V_c, largest, u)[1]
    assert np.all(np.abs(lam - lam_c) <= bound + bound_c)


@pytest.mark.parametrize("layout,itype", [op for op in cpu.OPERANDS if op != ("csr", torch.int64)])
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", list(lr.CASES))
def test_eigenvalues_of_the_other_operand_kinds(name, dt, largest, layout, itype):
    """Every CPU eigenvalue case as COO and as CSR with int32 indices too (CSR int64 is the test above): other plans, other kernels."""
    lam, V, info = cpu.solved(name, dt, largest, layout, itype, DEV)
    cpu.check_pairs(name, dt, largest, lam, V, info)


def test_restart_without_p_inside_the_loop():
    cpu.check_restart_case(*cpu.restart_case(DEV))


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("name", ["coupled", "stencil27"])
def test_gradient_against_dense_eigvalsh(name, dt, largest):
    got, want, tol, Asp = cpu.gradient_case(name, dt, largest, DEV)
    print(f"{name} {dt} largest={largest}: max |err| {np.abs(got - want).max():.3e}, tolerance {tol:.3e}")
    assert np.all(np.abs(got - want) <= tol)
    g = Asp.grad
    assert g.layout == torch.sparse_csr and g.device == Asp.device and g.dtype == Asp.dtype
    assert torch.equal(g.crow_indices(), Asp.crow_indices()) and torch.equal(g.col_indices(), Asp.col_indices())


def shifted(name, dtype):
    """(A + I as a CSR tensor on the GPU, its dense float64 copy, its spectrum): SPD for the Laplacian cases."""
    ptr, idx, val, k, D, spectrum = lr.case(name)
    n = D.shape[0]
    rows = np.repeat(np.arange(n), np.diff(ptr))
    A = torch.sparse_csr_tensor(torch.from_numpy(ptr), torch.from_numpy(idx), torch.from_numpy(val + (idx == rows)).to(dtype), (n, n))
    return A.to(DEV), D + np.eye(n), spectrum + 1.0


@pytest.mark.parametrize("kind", ["none", "fsai", "ic0", "dense"])
@pytest.mark.parametrize("dt", list(DT))
def test_preconditioned_smallest_pairs(dt, kind):
    dtype = cpu.DTYPES[dt][0]
    name = "stencil27" if kind == "dense" else "stencil7"
    A, D, spectrum = shifted(name, dtype) if name == "stencil7" else (cpu.operand(name, dtype, device=DEV), *lr.case(name)[4:])
    M = {"none": lambda: None, "fsai": lambda: tsgu.sparse_fsai(A), "ic0": lambda: tsgu.sparse_ic0(A),
         "dense": lambda: torch.from_numpy(np.linalg.inv(D)).to(dtype).to(DEV)}[kind]()
    k = 4 if name == "stencil7" else 3
    X = torch.from_numpy(lr.initial_block(D.shape[0], k)).to(dtype).to(DEV)
    lam, V = sparse_lobpcg(A, k, X=X, preconditioner=M, largest=False, niter=lr.NITER)
    info = utils.last_solve_info("lobpcg")
    u = unit(dtype)
    err, bound = lr.eigenvalue_bounds(D, spectrum, lam.double().cpu().numpy(), V.double().cpu().numpy(), False, u)
    print(f"{name} {dt} preconditioner {kind}: iterations {info['iterations']}, restarts {info['restarts']}")
    assert info["converged"] and max(info["residual_norms"]) <= info["tolerance"] * info["a_norm"]
    assert np.all(err <= bound), (err, bound)


def count_reads(A, X, niter):
    """(synchronising calls torch reports during one solve of `niter` iterations, where they were made)."""
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            sparse_lobpcg(A, X.size(1), X=X, largest=False, niter=niter, tol=0.0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert utils.last_solve_info("lobpcg")["iterations"] == niter
    sync = [w for w in seen if "synchroniz" in str(w.message)]
    return len(sync), sorted({f"{w.filename.rsplit('/', 1)[-1]}:{w.lineno}" for w in sync})


def test_one_device_to_host_read_per_iteration():
    """`tol = 0` never converges, so the loop runs `niter` iterations; the synchronising calls torch reports are counted for
    three values of `niter`, after two runs that let the pattern's plans settle (a plan that is built or adopted on the way reads
    its index arrays once).  Their differences are the reads of the extra iterations: 3 + niter was measured (the Gram matrix of
    the initial block, ‖A‖_est with the first rotation, the residual norms of the pairs that are handed out)."""
    A = cpu.operand("random", torch.float32, device=DEV)
    X = torch.from_numpy(lr.initial_block(300, 3)).float().to(DEV)
    sparse_lobpcg(A, 3, X=X, largest=False, niter=40, tol=0.0)
    count_reads(A, X, 5)
    (five, at5), (twelve, at12), (nineteen, at19) = count_reads(A, X, 5), count_reads(A, X, 12), count_reads(A, X, 19)
    print(f"synchronising calls: {five} for 5 iterations, {twelve} for 12, {nineteen} for 19; made at {at5}, {at12}, {at19}")
    assert twelve - five == 7 and nineteen - twelve == 7
    assert five - 5 <= 6, "the constant: the reads around the loop"
