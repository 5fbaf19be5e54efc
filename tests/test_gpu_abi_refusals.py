"""Dtype refusals of the extern "C" entry points: the value / index type codes a kernel family is not compiled for.

The type dispatch sits behind `set_device`, so these calls need a device — but they launch nothing: every case is a code the
family refuses.  The operands are otherwise valid (the base calls of _abi_cases.Call: 8 rows, 8 entries, the family's smallest
width, plans that pass `fill`) and every device buffer is a zero-filled 4 KiB allocation: whatever a wrongly accepted call would
read them as, every index is 0 and in range.

The table holds the answers of the library before the entry points were rewritten on the shared dispatch helpers of
csrc/tsgu_common.h.  Per entry point, in the order of `_cases`: the status of every (vtype, itype) pair.
"""

import pytest
import torch

import _abi_cases as A

pytestmark = pytest.mark.gpu

F32, F64, BF16, NONE = 0, 1, 2, 7

# the real value-type codes a family has no kernels for (everything not listed is compiled for fp32, fp64 and bf16)
_ONLY_F32 = ("tsgu_csr_spmm_tile", "tsgu_csr_sddmm_tile")
_F32_BF16 = ("tsgu_csr_mm_backward", "tsgu_csr_spmm_rowpack", "tsgu_csr_mm_backward_rowpack", "tsgu_csr_sddmm_rowpack", "tsgu_csr_spmm_march",
             "tsgu_csr_sddmm_march")
_F32_F64 = ("tsgu_csr_sptrsm_lattice", "tsgu_coldot", "tsgu_cg_alpha", "tsgu_cg_update1", "tsgu_cg_update1_alpha", "tsgu_cg_beta",
            "tsgu_cg_beta_precond", "tsgu_cg_update2", "tsgu_cg2_residual", "tsgu_cg2_direction", "tsgu_bicg_scalar", "tsgu_bicg_vector",
            "tsgu_bicg_update_x_precond", "tsgu_minres_scalar", "tsgu_minres_vector", "tsgu_minres_scalar_ms", "tsgu_minres_vector_ms",
            "tsgu_diag_logsum", "tsgu_diag_logsum_backward", "tsgu_quadform", "tsgu_quadform_backward", "tsgu_csr_row_sumsq",
            "tsgu_csr_row_sumsq_backward")
TYPED = [n for n in A.LAUNCHERS if {"vtype", "itype"} & {p[0] for p in A.PARAMS[n]}]


def _refused_vtypes(name):
    if name in _ONLY_F32:
        return (F64, BF16, NONE)
    if name in _F32_BF16:
        return (F64, NONE)
    if name in _F32_F64:
        return (BF16, NONE)
    return (NONE,)


def _cases(name):
    """The refused (changes) of an entry point, in a fixed order."""
    names = [p[0] for p in A.PARAMS[name]]
    out = []
    if "vtype" in names:
        out += [dict(vtype=v) for v in _refused_vtypes(name)]
    if "itype" in names:
        out.append(dict(itype=NONE))
    if "vtype" in names and "itype" in names:
        out.append(dict(vtype=NONE, itype=NONE))
    if name in ("tsgu_csr_spmm", "tsgu_csr_spmm_lattice_dot"):        # the dot epilogue sums in the value type: fp32 and fp64
        out.append(dict(vtype=BF16, dot_partial="buffer", dot_w="buffer"))
    return out


EXPECTED = {
    "tsgu_bicg_scalar": [-1, -1],
    "tsgu_bicg_update_x_precond": [-1, -1],
    "tsgu_bicg_vector": [-1, -1],
    "tsgu_cg2_direction": [-1, -1],
    "tsgu_cg2_residual": [-1, -1],
    "tsgu_cg_alpha": [-1, -1],
    "tsgu_cg_beta": [-1, -1],
    "tsgu_cg_beta_precond": [-1, -1],
    "tsgu_cg_update1": [-1, -1],
    "tsgu_cg_update1_alpha": [-1, -1],
    "tsgu_cg_update2": [-1, -1],
    "tsgu_coldot": [-1, -1],
    "tsgu_coo_sddmm": [-1, -1, -1],
    "tsgu_csr_diag_positions": [-1],
    "tsgu_csr_mm_backward": [-1, -1, -1, -1],
    "tsgu_csr_mm_backward_rowpack": [-1, -1, -1, -1],
    "tsgu_csr_row_sumsq": [-1, -1, -1, -1],
    "tsgu_csr_row_sumsq_backward": [-1, -1, -1, -1],
    "tsgu_csr_sddmm": [-1, -1, -1],
    "tsgu_csr_sddmm_lattice": [-1],
    "tsgu_csr_sddmm_march": [-1, -1],
    "tsgu_csr_sddmm_rowpack": [-1, -1, -1, -1],
    "tsgu_csr_sddmm_tile": [-1, -1, -1],
    "tsgu_csr_spmm": [-1, -1, -1, -2],
    "tsgu_csr_spmm_lattice": [-1],
    "tsgu_csr_spmm_lattice_dot": [-1, -1],
    "tsgu_csr_spmm_march": [-1, -1],
    "tsgu_csr_spmm_rowpack": [-1, -1, -1, -1],
    "tsgu_csr_spmm_tile": [-1, -1, -1],
    "tsgu_csr_sptrsm": [-1, -1, -1],
    "tsgu_csr_sptrsm_lattice": [-1, -1],
    "tsgu_diag_logsum": [-1, -1, -1, -1],
    "tsgu_diag_logsum_backward": [-1, -1, -1, -1],
    "tsgu_index_fingerprint": [-1],
    "tsgu_index_fingerprint_match": [-1],
    "tsgu_lattice_row_codes": [-1],
    "tsgu_lattice_rows": [-1],
    "tsgu_minres_scalar": [-1, -1],
    "tsgu_minres_scalar_ms": [-1, -1],
    "tsgu_minres_vector": [-1, -1],
    "tsgu_minres_vector_ms": [-1, -1],
    "tsgu_quadform": [-1, -1],
    "tsgu_quadform_backward": [-1, -1],
    "tsgu_segment_logsumexp": [-1, -1, -1],
    "tsgu_segment_logsumexp_backward": [-1, -1, -1],
    "tsgu_segment_mm": [-1, -1, -1],
    "tsgu_segment_mm_grad_b": [-1, -1, -1],
}


@pytest.fixture(scope="module")
def buffers():
    held = []

    def pointer(name, i):
        held.append(torch.zeros(4096, dtype=torch.uint8, device="cuda"))
        return held[-1].data_ptr()

    yield pointer
    torch.cuda.synchronize()


def test_every_typed_entry_is_listed():
    assert sorted(EXPECTED) == TYPED


@pytest.mark.parametrize("name", TYPED)
def test_dtype_refusals_of(name, buffers):
    call = A.Call(name, buffers, torch.cuda.current_device())
    got = []
    for ch in _cases(name):
        ch = {k: (buffers(k, 0) if v == "buffer" else v) for k, v in ch.items()}
        got.append(call.run(**ch))
    print(name, got)
    assert got == EXPECTED[name], f"{name}: {list(zip(_cases(name), got, EXPECTED[name]))}"
