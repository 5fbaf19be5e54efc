"""The cases of the plan-free CSR kernel tests (test_csr_geometry_cpu.py, test_gpu_csr_kernels.py): widths, what geometry each is
meant to hit, and the pairing of widths with the pattern builders of _csr_ref.py.  Host only: the geometry is asked of the library
(`_backend.csr_geometry`), which touches no device."""

import functools

import numpy as np
import torch

import _csr_ref as cr

SPMM, SDDMM, COO, BACKWARD = 0, 1, 2, 3
KERNELS = {SPMM: "csr_spmm", SDDMM: "csr_sddmm", COO: "coo_sddmm", BACKWARD: "csr_mm_backward"}
DTYPES = [torch.float32, torch.float64, torch.bfloat16]
IDS = ["f32", "f64", "bf16"]
WIDE = {torch.float32: 4, torch.float64: 2, torch.bfloat16: 8}
STAGE = {SPMM: 2048, SDDMM: 2048, COO: 2048, BACKWARD: 1024}

MULTIPLES = (1, 2, 3, 4, 8, 16, 32, 64, 65, 130)      # of `wide`: 16-byte lanes
SCALARS = (1, 3, 5, 9, 17, 33, 65, 129)               # no multiple of any `wide`: scalar lanes

# lanes a row needs (p / vec, rounded up) -> (column_lanes, entry_lanes, column_tiles)
LANES = {1: (1, 8, 1), 2: (2, 4, 1), 3: (4, 2, 1), 4: (4, 2, 1), 5: (8, 1, 1), 8: (8, 1, 1), 9: (16, 1, 1), 16: (16, 1, 1), 17: (32, 1, 1),
         32: (32, 1, 1), 33: (64, 1, 1), 64: (64, 1, 1), 65: (64, 1, 2), 129: (64, 1, 3), 130: (64, 1, 3)}


def widths(dtype):
    """[(p, mode)]: mode "ok" — operands that allow 16-byte lanes; "ld" — a leading dimension of p + 1 (a column slice of a wider
    buffer); "ptr" — a base pointer one element off 16 bytes.  p = 2 gives scalar lanes in two column lanes: on its own where 2 is no
    multiple of `wide`, through a leading dimension of 3 where it is."""
    w = WIDE[dtype]
    return [(w * k, "ok") for k in MULTIPLES] + [(p, "ok") for p in SCALARS] + [(2 * w, "ld"), (4 * w, "ptr"), (2, "ld" if w == 2 else "ok")]


def expected(kernel, dtype, p, mode, n=0, nnz=0, longest=0):
    """(vec, column_lanes, entry_lanes, column_tiles) the case is meant to hit."""
    w = WIDE[dtype]
    vec = w if mode == "ok" and p % w == 0 else 1
    cl, ep, tiles = LANES[-(-p // vec)]
    if kernel == COO:
        ep = 1
    if kernel == SPMM and vec > 1 and cl == 1 and n > 0 and nnz <= 16 * n and (longest == 0 or longest <= 4 * (nnz // n + 1) + 16):
        ep = 1      # one lane per row: 16-byte dense rows, short sparse rows, no row much longer than the mean
    return vec, cl, ep, tiles


def single_tile(dtype, p, mode):
    return expected(SDDMM, dtype, p, mode)[3] == 1


def query(kernel, dtype, p, mode="ok", col_strided=False):
    """`query(n_rows, nnz, max_row_nnz) -> Geom` for the builders: the library's answer.  A refusal raises — no case is skipped."""
    from torchsparsegradutils_amd import _backend

    def ask(n, nnz, longest):
        return cr.Geom(*_backend.csr_geometry(kernel, dtype, n, nnz, p, longest, mode == "ok", col_strided))

    return ask


N_CASES = 6 * len(cr.BUILDERS)


def case(kernel, dtype, i, only_single_tile=False):
    """Case i of a kernel: width i (mod the widths), builder i (mod the builders), int32 for even i and int64 for odd i.  21 (17 of
    one tile) widths and 13 builders have no common factor, so 78 cases are 78 different pairs: every builder with six widths, every
    width with three or four builders, each of them with both index types."""
    ws = [w for w in widths(dtype) if not only_single_tile or single_tile(dtype, *w)]
    p, mode = ws[i % len(ws)]
    name = cr.BUILDERS[i % len(cr.BUILDERS)]
    return p, mode, name, (torch.int32, torch.int64)[i % 2]


@functools.lru_cache(maxsize=None)
def pattern(kernel, dtype, i, only_single_tile=False):
    """(p, mode, index type, Pattern) of case i, its claim and its geometry asserted."""
    p, mode, name, itype = case(kernel, dtype, i, only_single_tile)
    pat = cr.build(name, query(kernel, dtype, p, mode), np.random.default_rng(1000 * kernel + i))
    cr.check_claim(pat, spmm_rules=kernel == SPMM)
    g = pat.geom
    longest = int(pat.lens.max()) if pat.honest else 0
    assert (g.vec, g.cl, g.ep, g.tiles) == expected(kernel, dtype, p, mode, pat.n, len(pat.col), longest), (KERNELS[kernel], p, mode, name, g)
    assert g.stage == STAGE[kernel] and (kernel == SPMM or g.runs == 1)
    return p, mode, itype, pat
