"""tsgu_csr_geometry — the lane geometry of the plan-free kernels (csr_spmm, csr_sddmm, coo_sddmm, csr_mm_backward) as the launchers
pick it — against the table the GPU tests are written for, and the pattern builders of _csr_ref.py against their claims for every
geometry.  No GPU: the query answers on the host and the builders are numpy."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import _abi_cases as A
import _csr_cases as cc
import _csr_ref as cr
from torchsparsegradutils_amd import _backend

VT = {torch.float32: 0, torch.float64: 1, torch.bfloat16: 2}


def _raw(kernel, vt, n, nnz, p, longest, wide_ok, strided, missing=None):
    outs = [ctypes.c_int(-99), ctypes.c_int(-99), ctypes.c_int(-99), ctypes.c_int64(-99), ctypes.c_int(-99), ctypes.c_int(-99)]
    refs = [None if k == missing else ctypes.byref(o) for k, o in enumerate(outs)]
    rc = _backend.load_library().tsgu_csr_geometry(kernel, vt, n, nnz, p, longest, wide_ok, strided, *refs)
    return rc, tuple(o.value for o in outs)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_the_table_of_widths(dtype):
    w = cc.WIDE[dtype]
    # 16-byte lanes: k lanes per row; long rows (100 entries per row), so that one lane of columns keeps its 8 entry lanes
    lanes = {1: (1, 8, 1), 2: (2, 4, 1), 3: (4, 2, 1), 4: (4, 2, 1), 8: (8, 1, 1), 16: (16, 1, 1), 32: (32, 1, 1), 64: (64, 1, 1), 65: (64, 1, 2),
             130: (64, 1, 3)}
    scalar = {1: (1, 8, 1), 3: (4, 2, 1), 5: (8, 1, 1), 9: (16, 1, 1), 17: (32, 1, 1), 33: (64, 1, 1), 65: (64, 1, 2), 129: (64, 1, 3)}
    assert tuple(lanes) == cc.MULTIPLES and tuple(scalar) == cc.SCALARS
    for kernel in cc.KERNELS:
        if kernel == cc.BACKWARD and dtype == torch.float64:
            continue
        ep_of = (lambda ep: 1) if kernel == cc.COO else (lambda ep: ep)
        for k, (cl, ep, tiles) in lanes.items():
            if kernel == cc.BACKWARD and tiles != 1:
                with pytest.raises(RuntimeError, match="tsgu_csr_geometry"):
                    _backend.csr_geometry(kernel, dtype, 1000, 100000, w * k)
                continue
            got = _backend.csr_geometry(kernel, dtype, 1000, 100000, w * k)
            assert got[:4] == (w, cl, ep_of(ep), tiles), (kernel, k, got)
            assert got[5] == cc.STAGE[kernel] and (kernel == cc.SPMM or got[4] == 1)
            # the same width without 16-byte lanes: w·k scalar lanes
            got = _backend.csr_geometry(kernel, dtype, 1000, 100000, w * k, wide_ok=False) if w * k <= 64 or kernel != cc.BACKWARD else None
            if got is not None:
                ncl = w * k
                want_cl = min(64, 1 << (ncl - 1).bit_length())
                assert got[:4] == (1, want_cl, ep_of(1 if want_cl >= 8 else 8 // want_cl), -(-ncl // want_cl)), (kernel, k, got)
        for p, (cl, ep, tiles) in scalar.items():
            if kernel == cc.BACKWARD and tiles != 1:
                continue
            for ok in (True, False):
                assert _backend.csr_geometry(kernel, dtype, 1000, 100000, p, wide_ok=ok)[:4] == (1, cl, ep_of(ep), tiles), (kernel, p)
        for p, mode in cc.widths(dtype):
            if kernel != cc.BACKWARD or cc.single_tile(dtype, p, mode):
                assert cc.query(kernel, dtype, p, mode)(1000, 100000, 0)[:4] == cc.expected(kernel, dtype, p, mode, 1000, 100000, 0)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
def test_one_lane_per_row_and_the_column_strided_operand(dtype):
    w = cc.WIDE[dtype]

    def geo(*a, **k):
        return _backend.csr_geometry(cc.SPMM, dtype, *a, **k)[:4]

    assert geo(1000, 16000, w) == (w, 1, 1, 1) and geo(1000, 16001, w) == (w, 1, 8, 1)
    assert geo(1000, 7000, w, 48) == (w, 1, 1, 1) and geo(1000, 7000, w, 49) == (w, 1, 8, 1)      # 4·(7 + 1) + 16 = 48
    assert geo(1000, 7000, 2 * w) == (w, 2, 4, 1) and geo(1000, 7000, 1) == (1, 1, 8, 1) and geo(1000, 7000, w, wide_ok=False)[0] == 1
    for kernel in (cc.SDDMM, cc.BACKWARD):
        if kernel != cc.BACKWARD or dtype != torch.float64:
            assert _backend.csr_geometry(kernel, dtype, 1000, 7000, w)[:4] == (w, 1, 8, 1)
    # column-strided: one scalar lane per row or 8 entry lanes, one column per tile, whatever the width allows
    for p in (1, w, 3 * w, 300):
        assert geo(1000, 16000, p, col_strided=True) == (1, 1, 1, p) and geo(1000, 16001, p, 5, col_strided=True) == (1, 1, 8, p)
        assert geo(0, 0, p, col_strided=True) == (1, 1, 8, p)
        for kernel in (cc.SDDMM, cc.COO):      # honoured for the product alone
            assert _backend.csr_geometry(kernel, dtype, 1000, 16000, p, col_strided=True) == _backend.csr_geometry(kernel, dtype, 1000, 16000, p)


def test_row_runs_are_the_block_count_of_the_dot_epilogue():
    lib = _backend.load_library()
    seen = set()
    for dtype, n, nnz, p, longest in itertools.product(cc.DTYPES, (0, 1, 8, 255, 256, 257, 1000, 4099, 1 << 22), (0, 1, 300, 7000, 11000, 100000, 1 << 26),
                                                       (1, 2, 4, 8, 12, 33, 64, 256, 1000, 1040), (0, 5, 4000)):
        vec, cl, ep, tiles, runs, stage = _backend.csr_geometry(cc.SPMM, dtype, n, nnz, p, longest, wide_ok=True)
        assert 1 <= runs <= 8 and stage == 2048 and 256 % (cl * ep) == 0
        rows = 256 // (cl * ep) * runs
        assert -(-n // rows) == lib.tsgu_spmm_num_blocks(VT[dtype], n, nnz, p, longest), (dtype, n, nnz, p, longest)
        seen.add(runs)
    assert seen == set(range(1, 9))


def test_refusals():
    ok = (cc.SPMM, 0, 8, 8, 8, 0, 1, 0)
    assert _raw(*ok) == (A.OK, (4, 2, 4, 1, 8, 2048))
    for vt in (-1, 3, 7):
        for kernel in cc.KERNELS:
            assert _raw(kernel, vt, 8, 8, 8, 0, 1, 0) == (A.BAD_DTYPE, (-99,) * 6)
    assert _raw(cc.BACKWARD, 1, 8, 8, 8, 0, 1, 0) == (A.BAD_DTYPE, (-99,) * 6)
    assert _raw(cc.BACKWARD, 0, 8, 8, 8, 0, 1, 0) == (A.OK, (4, 2, 4, 1, 1, 1024)) and _raw(cc.BACKWARD, 2, 8, 8, 8, 0, 1, 0)[0] == A.OK
    for kernel in (-1, 4, 99):
        assert _raw(kernel, 0, 8, 8, 8, 0, 1, 0) == (A.BAD_ARG, (-99,) * 6)
    for k in (2, 3, 4, 5):      # a negative size
        args = list(ok)
        args[k] = -1
        assert _raw(*args) == (A.BAD_ARG, (-99,) * 6), k
    for missing in range(6):
        assert _raw(*ok, missing=missing) == (A.BAD_ARG, (-99,) * 6), missing
    # the fused backward where its launcher refuses: more than one column tile (and no column at all)
    for vt, p in ((0, 260), (0, 65), (2, 520), (2, 65), (0, 0)):
        assert _raw(cc.BACKWARD, vt, 8, 8, p, 0, 1, 0) == (A.BAD_ARG, (-99,) * 6), (vt, p)
    assert _raw(cc.BACKWARD, 0, 8, 8, 256, 0, 1, 0)[0] == A.OK and _raw(cc.BACKWARD, 0, 8, 8, 256, 0, 0, 0)[0] == A.BAD_ARG
    assert _raw(cc.BACKWARD, 2, 8, 8, 512, 0, 1, 0)[0] == A.OK and _raw(cc.BACKWARD, 0, 8, 8, 64, 0, 0, 0) == (A.OK, (1, 64, 1, 1, 1, 1024))
    # what the launchers accept the query answers: no rows, no entries, no columns
    assert _raw(cc.SPMM, 0, 0, 0, 0, 0, 1, 0)[0] == A.OK and _raw(cc.SDDMM, 1, 0, 0, 0, 0, 1, 0) == (A.OK, (2, 1, 8, 0, 1, 2048))
    with pytest.raises(RuntimeError, match="tsgu_csr_geometry"):
        _backend.csr_geometry(cc.BACKWARD, torch.float32, 8, 8, 260)


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
@pytest.mark.parametrize("kernel", list(cc.KERNELS), ids=list(cc.KERNELS.values()))
def test_every_builder_delivers_its_claim_for_every_geometry(kernel, dtype):
    if kernel == cc.BACKWARD and dtype == torch.float64:
        with pytest.raises(RuntimeError, match="unsupported value/index dtype"):
            cc.query(kernel, dtype, 8)(8, 8, 0)
        return
    seen, runs = set(), set()
    specs = [(p, mode, False) for p, mode in cc.widths(dtype) if kernel != cc.BACKWARD or cc.single_tile(dtype, p, mode)]
    if kernel == cc.SPMM:
        specs += [(3, "ok", True), (cc.WIDE[dtype], "ok", True)]
    for (p, mode, strided), name in itertools.product(specs, cr.BUILDERS):
        pat = cr.build(name, cc.query(kernel, dtype, p, mode, strided), np.random.default_rng(len(seen)))
        cr.check_claim(pat, spmm_rules=kernel == cc.SPMM)
        g = pat.geom
        longest = int(pat.lens.max()) if pat.honest else 0
        if not strided:
            assert (g.vec, g.cl, g.ep, g.tiles) == cc.expected(kernel, dtype, p, mode, pat.n, len(pat.col), longest), (p, mode, name, g)
        else:
            assert (g.vec, g.cl, g.tiles) == (1, 1, p) and g.ep == (1 if len(pat.col) <= 16 * pat.n else 8)
        seen.add((g.vec > 1, g.cl, g.ep))
        runs.add(g.runs)
    # every (16-byte lanes?, column lanes, entry lanes) dispatch_geom can reach for the kernel, scalar one lane per row (the
    # column-strided operand) included
    reach = {(v, cl, ep) for v in (False, True) for cl, ep in ((1, 8), (2, 4), (4, 2), (8, 1), (16, 1), (32, 1), (64, 1))}
    if kernel == cc.COO:
        reach = {(v, cl, 1) for v, cl, _ in reach}
    if kernel == cc.SPMM:
        reach |= {(True, 1, 1), (False, 1, 1)}
    assert seen == reach, sorted(reach ^ seen)
    if kernel == cc.SPMM:
        assert {1, 8} < runs and any(1 < r < 8 for r in runs), runs
    else:
        assert runs == {1}


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=cc.IDS)
@pytest.mark.parametrize("kernel", list(cc.KERNELS), ids=list(cc.KERNELS.values()))
def test_the_gpu_cases_reach_every_geometry_and_path(kernel, dtype):
    """What test_gpu_csr_kernels.py runs for a kernel and value type: each case asserts its own geometry and claim (`cc.pattern`);
    together they hold every lane geometry the kernel can take with row-major operands, one and several column tiles, slices
    that fit and slices that stream, 1, 2 to 7 and 8 row runs, and both index types."""
    if kernel == cc.BACKWARD and dtype == torch.float64:
        return
    only = kernel == cc.BACKWARD
    got = [cc.pattern(kernel, dtype, i, only) for i in range(cc.N_CASES)]
    geoms = {(pat.geom.vec > 1, pat.geom.cl, pat.geom.ep) for _, _, _, pat in got}
    reach = {(v, cl, 1 if kernel == cc.COO else ep) for v in (False, True) for cl, ep in ((1, 8), (2, 4), (4, 2), (8, 1), (16, 1), (32, 1), (64, 1))}
    if kernel == cc.SPMM:
        reach.add((True, 1, 1))
    assert geoms == reach, sorted(reach ^ geoms)
    assert {pat.geom.tiles for _, _, _, pat in got} == ({1} if only else {1, 2, 3})
    slices = [int(cr.slices(pat.crow, pat.geom).max()) for _, _, _, pat in got]
    stage = cc.STAGE[kernel]
    every = {int(s) for _, _, _, pat in got for s in cr.slices(pat.crow, pat.geom)}
    assert {0, stage - 1, stage, stage + 1, 2 * stage + 1} <= every and max(every) == 2 * stage + 1
    assert {it for _, _, it, _ in got} == {torch.int32, torch.int64}
    if kernel == cc.SPMM:
        runs = {pat.geom.runs for _, _, _, pat in got}
        assert {1, 8} < runs and any(1 < r < 8 for r in runs), runs
        assert any(pat.geom.runs > 1 and s > stage for s, (_, _, _, pat) in zip(slices, got)), "MULTI with a streaming slice"


def test_the_cases_hold_every_width_and_builder():
    for dtype in cc.DTYPES:
        for only in (False, True):
            ws = [w for w in cc.widths(dtype) if not only or cc.single_tile(dtype, *w)]
            got = [cc.case(cc.SPMM, dtype, i, only) for i in range(cc.N_CASES)]
            assert {(p, mode) for p, mode, _, _ in got} == set(ws) and {name for _, _, name, _ in got} == set(cr.BUILDERS)
            for name in cr.BUILDERS:      # each builder with both index types
                assert {it for _, _, nm, it in got if nm == name} == {torch.int32, torch.int64}
