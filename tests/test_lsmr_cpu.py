"""LSMR without a GPU: the staged header against its ctypes table and the library, and the two constructions of
tests/_lsmr_cases.py (their condition numbers; the long problem needs more than 100 iterations of the host-driven loop)."""

import ctypes
import os

import _abi_cases as A
import _lsmr_cases as C
from torchsparsegradutils_amd import _backend
from torchsparsegradutils_amd.utils import last_solve_info, lsmr

STAGED_HEADER = os.path.join(os.path.dirname(os.path.abspath(_backend.__file__)), "csrc", "tsgu_hip_lsmr.h")
ENTRIES = ("tsgu_lsmr_scal_rows", "tsgu_lsmr_scalar", "tsgu_lsmr_vector")


def test_the_staged_header_is_bound():
    assert _backend.STAGED_LSMR == {"tsgu_hip_lsmr.h": _backend.SIGNATURES_LSMR}
    protos = A.prototypes(STAGED_HEADER)
    assert tuple(n for n, _ in protos) == ENTRIES == tuple(_backend.SIGNATURES_LSMR)
    raw = ctypes.CDLL(_backend.LIB_PATH)
    lib = _backend.load_library()
    for name, params in protos:
        assert hasattr(raw, name), f"{name} is declared in the staged header but not exported by libtsgu_hip.so"
        restype, argtypes = _backend.SIGNATURES_LSMR[name]
        assert [A.klass_of_ctype(t) for t in argtypes] == [A.klass_of_decl(t) for _, t in params], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    assert lib.tsgu_lsmr_scal_rows() == 28 > max(_backend.LSMR_ROW.values())


def test_the_constructions():
    A_, L_ = C.tall(), C.tall(dmin=C.DMIN_LONG)
    assert 8 < C.cond(A_) < 12 and 20 < C.cond(L_) < 30
    B = C.rhs(L_.shape[0], 1)
    x, its = lsmr(L_, B, atol=1e-12, btol=1e-12, maxiter=400)
    info = last_solve_info("lsmr")
    assert 100 < its < 400 and info["iterations"] == its and info["tolerance_reached"] and not info["fused"]
    assert C.relerr(x, C.dense_lstsq(L_, B)) <= 1e-9
