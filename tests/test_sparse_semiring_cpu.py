"""sparse_semiring_mm without a GPU: the numpy oracle (tests/_semiring_ref.py) against a dense float64 restatement, the torch-op path
against the oracle, gradcheck, the refusals, and the host refusals of the entries of include/tsgu_hip_semiring.h.

float64 comparisons: both sides sum at most 12 exponentials of O(1) shifted candidates; 1e-12 leaves three digits over 12·2⁻⁵³·|C|.
"""

import ctypes
import os

import numpy as np
import pytest
import torch

import _abi_cases as A
import _semiring_ref as sr
from torchsparsegradutils_amd import _backend, _cpu, sparse_semiring_mm

N, M, P = 23, 17, 5
ZERO = {"log": -np.inf, "max_plus": -np.inf, "min_plus": np.inf}


def _case(seed=0):
    rng = np.random.default_rng(seed)
    lens = list(rng.integers(0, 13, size=N))
    lens[3] = 0
    crow, col = sr.random_csr(N, M, lens, seed)
    val, B = rng.standard_normal(len(col)) * 3, rng.standard_normal((M, P)) * 3
    val[crow[5]] = -np.inf                                   # an absent entry among finite ones
    return crow, col, val, B


def _csr(crow, col, val, dtype=torch.float64):
    return torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val).to(dtype), (N, M))


@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_the_oracle_and_the_torch_op_path_against_a_dense_restatement(semiring):
    crow, col, val, B = _case()
    dense = torch.full((N, M), ZERO[semiring], dtype=torch.float64)
    rows = np.repeat(np.arange(N), np.diff(crow))
    dense[rows, col] = torch.from_numpy(val)
    T = dense[:, :, None] + torch.from_numpy(B)[None]
    want = {"log": lambda: torch.logsumexp(T, 1), "max_plus": lambda: T.amax(1), "min_plus": lambda: T.amin(1)}[semiring]()
    C, arg, _ = sr.forward(crow, col, val, B, semiring)
    assert torch.equal(torch.isinf(want), torch.from_numpy(np.isinf(C))) and np.isinf(C[3]).all()
    torch.testing.assert_close(torch.from_numpy(C), want, rtol=0, atol=1e-12)
    got = sparse_semiring_mm(_csr(crow, col, val), torch.from_numpy(B), semiring)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    if arg is not None:
        Ccpu, argcpu = _cpu.semiring_mm(torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(B), (N, M), semiring)
        assert torch.equal(argcpu, torch.from_numpy(arg)) and (arg[3] == -1).all() and sr.same_bits(Ccpu, torch.from_numpy(C))


@pytest.mark.parametrize("layout", ["csr", "coo"])
@pytest.mark.parametrize("semiring", sr.SEMIRINGS)
def test_gradcheck_and_gradients_against_the_oracle(semiring, layout):
    crow, col, val, B = _case(1)
    G = np.random.default_rng(2).standard_normal((N, P))
    a = _csr(crow, col, val).requires_grad_(True) if layout == "csr" else _csr(crow, col, val).to_sparse_coo().requires_grad_(True)
    b = torch.from_numpy(B).requires_grad_(True)
    gA, gB = torch.autograd.grad(sparse_semiring_mm(a, b, semiring), (a, b), torch.from_numpy(G))
    C, arg, wt = sr.forward(crow, col, val, B, semiring)
    dval, _, dB, _ = sr.gradients(crow, col, val, B, G, semiring, C, arg, None if wt is None else wt * 0, 0.0)
    assert gA.layout == a.layout and np.isfinite(dval).all() and (semiring != "log" or dval[crow[5]] == 0)     # an absent entry: weight 0
    torch.testing.assert_close(gA.values() if layout == "csr" else gA.coalesce().values(), torch.from_numpy(dval), rtol=0, atol=1e-11)
    torch.testing.assert_close(gB, torch.from_numpy(dB), rtol=0, atol=1e-11)
    if semiring == "log" and layout == "csr":
        fin = np.where(np.isfinite(val), val, 0.0)            # (gradcheck perturbs every value: finite ones only)
        vals = torch.from_numpy(fin).requires_grad_(True)
        f = lambda v, bb: sparse_semiring_mm(torch.sparse_csr_tensor(torch.from_numpy(crow), torch.from_numpy(col), v, (N, M)), bb, "log")  # noqa: E731
        keep = torch.from_numpy(np.diff(crow) > 0)
        assert torch.autograd.gradcheck(lambda v, bb: f(v, bb)[keep], (vals, b), atol=1e-6, rtol=1e-4)


def test_refusals():
    crow, col, val, B = _case()
    S, Bt = _csr(crow, col, val), torch.from_numpy(B)
    with pytest.raises(ValueError, match=r"semiring must be one of 'log', 'max_plus' or 'min_plus', got 'sum'"):
        sparse_semiring_mm(S, Bt, "sum")
    with pytest.raises(TypeError, match=r"A should be in either COO or CSR sparse format, got torch.strided"):
        sparse_semiring_mm(S.to_dense(), Bt)
    with pytest.raises(TypeError, match=r"B must be a dense \(strided\) tensor"):
        sparse_semiring_mm(S, S)
    with pytest.raises(TypeError, match=r"expected A and B to have the same dtype, got torch.float64 and torch.float32"):
        sparse_semiring_mm(S, Bt.float())
    with pytest.raises(TypeError, match=r"values must be float32, float64 or bfloat16, got torch.float16"):
        sparse_semiring_mm(_csr(crow, col, val, torch.float16), Bt.half())
    with pytest.raises(ValueError, match=r"Incompatible inner dimensions: A\[\.\.\., 17\] vs B\[\.\.\., 5\]"):
        sparse_semiring_mm(S, Bt.t())
    with pytest.raises(ValueError, match=r"A and B must both be 2D or both be 3D tensors"):
        sparse_semiring_mm(S, Bt[None])
    with pytest.raises(ValueError, match=r"B needs at least one column"):
        sparse_semiring_mm(S, Bt[:, :0])


def test_the_translation_unit_includes_the_header():
    src = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "semiring.hip")
    assert os.path.exists(src) and '#include "../../include/tsgu_hip_semiring.h"' in open(src).read(), "the translation unit the Makefile's wildcard picks up"


def test_host_refusals_of_the_entries():
    """Fake pointers and device = -1: the refusals come before anything is dereferenced or launched."""
    lib = _backend.load_library()
    q = 4096
    assert _backend.semiring_geometry(torch.float32, 32) == (32, 2048, 32) and _backend.semiring_geometry(torch.bfloat16, 4096)[2] == 512
    assert lib.tsgu_semiring_geometry(9, 4, None, None, None) == A.BAD_DTYPE and lib.tsgu_semiring_geometry(0, 0, None, None, None) == A.BAD_ARG
    fwd = lambda vt=0, it=0, s=0, n=4, nnz=8, p=4, ptr=q, B=q, C=q, acc=None, arg=None, ld=4: lib.tsgu_csr_semiring_mm(   # noqa: E731
        vt, it, s, n, 6, nnz, ptr, q, q, B, ld, p, C, ld, acc, ld, arg, ld, -1, None)
    assert fwd(vt=9) == A.BAD_DTYPE and fwd(it=5) == A.BAD_DTYPE and fwd(s=3) == A.BAD_ARG and fwd(s=-1) == A.BAD_ARG
    assert fwd(n=-1) == A.BAD_ARG and fwd(p=0) == A.BAD_ARG and fwd(ptr=None) == A.BAD_ARG and fwd(B=None) == A.BAD_ARG
    assert fwd(C=None) == A.BAD_ARG and fwd(ld=3) == A.BAD_ARG and fwd(acc=q + 2) == A.BAD_ARG and fwd(nnz=1 << 31) == A.TOO_LARGE
    assert fwd(s=1) == A.BAD_ARG and fwd(s=2, arg=q + 1) == A.BAD_ARG, "the tropical forward needs arg, in whole int32 entries"
    assert fwd(n=0) == A.OK, "no rows: nothing to do"
    assert fwd() == A.BAD_ARG and fwd(s=1, arg=q) == A.BAD_ARG, "device -1 is refused after the operands passed"
    bv = lambda s=0, nnz=8, val=q, acc=q, arg=None, G=q: lib.tsgu_csr_semiring_mm_bwd_values(   # noqa: E731
        0, 0, s, 4, 6, nnz, q, q, val, q, 4, acc, 4, arg, 4, G, 4, 4, q, -1, None)
    assert bv(nnz=0, G=None, acc=None) == A.OK and bv(val=None) == A.BAD_ARG and bv(acc=None) == A.BAD_ARG and bv(G=None) == A.BAD_ARG
    assert bv(s=1) == A.BAD_ARG and bv(s=1, arg=q, val=None, acc=None) == A.BAD_ARG, "... the last for the device"
    bd = lambda s=0, perm=q, val=q, B=q, acc=q, arg=None, dB=q: lib.tsgu_csr_semiring_mm_bwd_dense(   # noqa: E731
        0, 0, s, 4, 6, 8, q, q, perm, val, B, 4, acc, 4, arg, 4, q, 4, 4, dB, 4, -1, None)
    assert bd(perm=None) == A.BAD_ARG and bd(val=None) == A.BAD_ARG and bd(B=None) == A.BAD_ARG and bd(acc=None) == A.BAD_ARG
    assert bd(dB=None) == A.BAD_ARG and bd(s=2) == A.BAD_ARG and bd() == A.BAD_ARG and bd(s=2, arg=q, B=None, acc=None, val=None) == A.BAD_ARG
