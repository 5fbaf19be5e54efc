"""LSMR without a GPU: the scalar block's row table against the library, and the two constructions of
tests/_lsmr_cases.py (their condition numbers; the long problem needs more than 100 iterations of the host-driven loop)."""

import _lsmr_cases as C
from torchsparsegradutils_amd import _backend
from torchsparsegradutils_amd.utils import last_solve_info, lsmr


def test_the_scalar_rows():
    assert _backend.load_library().tsgu_lsmr_scal_rows() == 28 > max(_backend.LSMR_ROW.values())


def test_the_constructions():
    A_, L_ = C.tall(), C.tall(dmin=C.DMIN_LONG)
    assert 8 < C.cond(A_) < 12 and 20 < C.cond(L_) < 30
    B = C.rhs(L_.shape[0], 1)
    x, its = lsmr(L_, B, atol=1e-12, btol=1e-12, maxiter=400)
    info = last_solve_info("lsmr")
    assert 100 < its < 400 and info["iterations"] == its and info["tolerance_reached"] and not info["fused"]
    assert C.relerr(x, C.dense_lstsq(L_, B)) <= 1e-9
