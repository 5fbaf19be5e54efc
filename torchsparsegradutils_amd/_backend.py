"""ctypes binding of ``libtsgu_hip.so`` (C ABI in ``include/tsgu_hip.h``).

PyTorch is used for device memory and streams only: every wrapper below takes
tensors, checks them, and hands raw device pointers + the current HIP stream to
the hand-written gfx950 kernels.  There is NO fallback: if the shared library is
missing, or a tensor does not live on a HIP device, the call raises.
"""

from __future__ import annotations

import ctypes
import functools
import os
import sys
import threading
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSGU_LIB_PATH") or os.path.join(_HERE, "csrc", "libtsgu_hip.so")  # env override: kernel A/B builds

TSGU_F32, TSGU_F64, TSGU_BF16 = 0, 1, 2
TSGU_I32, TSGU_I64 = 0, 1

_VTYPE = {torch.float32: TSGU_F32, torch.float64: TSGU_F64, torch.bfloat16: TSGU_BF16}
_ITYPE = {torch.int32: TSGU_I32, torch.int64: TSGU_I64}

_lib = None
_lib_lock = threading.Lock()

_i64 = ctypes.c_int64
_int = ctypes.c_int
_ptr = ctypes.c_void_p
_dbl = ctypes.c_double

# One table per header of include/: name -> (restype, argtypes) of every symbol the header declares.  `ABI` below them is the registry.
ABI_VERSION = 7          # TSGU_ABI_VERSION of include/tsgu_hip.h this binding was written against

SIGNATURES = {
    "tsgu_abi_version": (_int, []),
    "tsgu_status_string": (ctypes.c_char_p, [_int]),
    "tsgu_device_info": (_int, [_int, ctypes.c_char_p, _int, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_device_copy": (_int, [_ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_device_cu_count": (_int, [_int, ctypes.POINTER(_int)]),
    "tsgu_index_fingerprint": (_int, [_int, _i64, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_index_fingerprint_match": (_int, [_int, _i64, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_tile_geometry": (_int, [_int, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_spmm_tile": (_int, [_int, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _int, _ptr]),
    "tsgu_csr_sddmm_tile": (_int, [_int, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _dbl, _i64, _int, _ptr]),
    "tsgu_csr_spmm": (
        _int,
        [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _i64, _ptr, _i64, _i64, _i64, _i64, _i64, _i64,
         _ptr, _i64, _ptr, _int, _ptr],
    ),
    "tsgu_spmm_num_blocks": (_i64, [_int, _i64, _i64, _i64, _i64]),
    "tsgu_csr_geometry": (_int, [_int, _int, _i64, _i64, _i64, _i64, _int, _int, ctypes.POINTER(_int), ctypes.POINTER(_int),
                                 ctypes.POINTER(_int), ctypes.POINTER(_i64), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_sddmm": (
        _int,
        [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _dbl, _int, _i64, _i64,
         _int, _ptr],
    ),
    "tsgu_coo_sddmm": (_int, [_int, _int, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _dbl, _i64, _int, _ptr]),
    "tsgu_segment_logsumexp_workspace": (_int, [_int, _i64, ctypes.POINTER(_i64)]),
    "tsgu_segment_logsumexp": (
        _int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _int, _i64, _ptr, _i64, _i64, _ptr, _i64, _int, _ptr],
    ),
    "tsgu_segment_logsumexp_backward": (
        _int, [_int, _int, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr],
    ),
    "tsgu_segment_mm_tile_rows": (_int, []),
    "tsgu_segment_mm": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _ptr, _i64, _i64, _i64, _ptr, _i64, _int, _ptr],
    ),
    "tsgu_segment_mm_grad_b_workspace": (
        _int, [_int, _i64, _i64, _i64, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)],
    ),
    "tsgu_segment_mm_grad_b": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _i64,
               _int, _ptr],
    ),
    "tsgu_csr_mm_backward": (
        _int,
        [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _ptr, _i64,
         _i64, _i64, _i64, _int, _ptr],
    ),
    "tsgu_minres_scalar": (
        _int,
        [_int, _int, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _dbl, _dbl, _dbl, _i64, _int, _ptr],
    ),
    "tsgu_minres_vector": (
        _int,
        [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _int, _int, _ptr],
    ),
    "tsgu_minres_scalar_ms": (
        _int,
        [_int, _int, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _dbl, _dbl, _ptr, _int, _dbl, _i64, _int, _ptr],
    ),
    "tsgu_minres_vector_ms": (
        _int,
        [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _int, _int, _i64, _dbl, _int, _ptr],
    ),
    "tsgu_bicg_update_x_precond": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_rowpack_geometry": (
        _int,
        [_int, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
         ctypes.POINTER(_int)],
    ),
    "tsgu_csr_spmm_rowpack": (_int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _int, _ptr]),
    "tsgu_csr_mm_backward_rowpack": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _i64, _i64, _int, _ptr]),
    "tsgu_csr_sddmm_rowpack": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _dbl, _i64, _int, _ptr]),
    "tsgu_lattice_lds_bytes": (_int, [_int, _int, _i64, _int, _int, _int, _int, _int, _int, _int, _int, _int]),
    "tsgu_csr_spmm_lattice": (_int, [_int, _ptr, _i64, _i64, _ptr, _ptr, _i64, _ptr, _i64, _i64, _int, _ptr]),
    "tsgu_csr_spmm_lattice_dot": (_int, [_int, _ptr, _i64, _i64, _ptr, _ptr, _i64, _ptr, _i64, _i64, _ptr, _i64, _ptr, _ptr, _int, _ptr]),
    "tsgu_csr_sddmm_lattice": (_int, [_int, _ptr, _i64, _i64, _ptr, _i64, _ptr, _i64, _ptr, _dbl, _i64, _int, _ptr]),
    "tsgu_march_supported": (_int, [_int, _int, _int, _int]),
    "tsgu_march_lds_bytes": (_int, [_int, _int, _i64, _int, _int, _int, _int, _int, _int]),
    "tsgu_csr_spmm_march": (_int, [_int, _ptr, _int, _i64, _i64, _ptr, _ptr, _i64, _ptr, _i64, _i64, _int, _ptr]),
    "tsgu_csr_sddmm_march": (_int, [_int, _ptr, _i64, _i64, _ptr, _i64, _ptr, _i64, _ptr, _dbl, _int, _i64, _int, _ptr]),
    "tsgu_lattice_slots": (_int, []),
    "tsgu_lattice_rows": (_int, [_int, _i64, _ptr, _ptr, _int, _int, _int, _int, _ptr, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr,
                                 _int, _int, _int, _ptr]),
    "tsgu_lattice_row_codes": (_int, [_int, _i64, _ptr, _ptr, _int, _int, _int, _int, _ptr, _int, _ptr, _int, _ptr, _int, _ptr]),
    "tsgu_lattice_block_classes": (_int, [_i64, _ptr, _int, _int, _int, _int, _int, _int, _int, _ptr, _int, _ptr]),
    "tsgu_csr_sptrsm": (
        _int,
        [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _int, _int, _ptr],
    ),
    "tsgu_sptrsm_work_bytes": (_i64, [_i64, _i64]),
    "tsgu_csr_sptrsm_lattice": (_int, [_int, _ptr, _i64, _ptr, _int, _int, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _int, _int, _ptr]),
    "tsgu_cg_fold_rows": (_i64, []),
    "tsgu_cg_alpha": (_int, [_int, _ptr, _i64, _ptr, _ptr, _ptr, _dbl, _i64, _int, _ptr]),
    "tsgu_cg_update1": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_cg_num_blocks": (_i64, [_int, _i64, _i64]),
    "tsgu_cg_beta": (_int, [_int, _ptr, _i64, _ptr, _ptr, _dbl, _dbl, _dbl, _int, _int, _i64, _int, _ptr]),
    "tsgu_cg_beta_precond": (_int, [_int, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _dbl, _dbl, _dbl, _int, _int, _i64, _int, _ptr]),
    "tsgu_cg_update2": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_cg2_num_blocks": (_i64, [_int, _i64, _i64]),
    "tsgu_cg2_residual": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _int, _dbl, _ptr, _int, _ptr]),
    "tsgu_cg2_direction": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _int, _dbl, _dbl, _dbl, _int, _ptr, _int, _int, _ptr]),
    "tsgu_cg_update1_alpha": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _dbl, _ptr, _int, _ptr]),
    "tsgu_bicg_scalar": (_int, [_int, _int, _ptr, _i64, _i64, _ptr, _ptr, _ptr, _dbl, _dbl, _int, _int, _i64, _int, _ptr]),
    "tsgu_bicg_vector": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_coldot_max_blocks": (_i64, [_i64, _i64]),
    "tsgu_coldot": (_int, [_int, _i64, _i64, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _int, _ptr]),
    "tsgu_mvn_reduce_blocks": (_i64, [_i64]),
    "tsgu_csr_diag_positions": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_diag_logsum": (_int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_diag_logsum_backward": (_int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_quadform": (_int, [_int, _i64, _i64, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _int, _i64, _ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_quadform_backward": (
        _int, [_int, _i64, _i64, _ptr, _i64, _i64, _ptr, _i64, _i64, _ptr, _int, _i64, _ptr, _ptr, _i64, _i64, _ptr, _int, _ptr],
    ),
    "tsgu_csr_row_sumsq": (_int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_csr_row_sumsq_backward": (_int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_softmax.h (same library, same ABI version)
SIGNATURES_SOFTMAX = {
    "tsgu_segment_softmax_workspace": (_int, [_int, _i64, ctypes.POINTER(_i64)]),
    "tsgu_segment_softmax": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _int, _ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_segment_softmax_backward": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _ptr, _ptr, _i64, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_attention.h (same library, same ABI version)
SIGNATURES_ATTENTION = {
    "tsgu_csr_attention_supported": (_int, [_int, _int, _int]),
    "tsgu_csr_attention_geometry": (_int, [_int, _int, _int, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_attention": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _int, _int, _dbl, _ptr, _i64,
               _ptr, _int, _ptr]),
    "tsgu_csr_attention_backward_rows": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _int, _int,
               _dbl, _ptr, _i64, _ptr, _ptr, _int, _ptr]),
    "tsgu_csr_attention_backward_cols": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _int,
               _int, _dbl, _ptr, _i64, _ptr, _i64, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_mm_reduce.h (same library, same ABI version)
SIGNATURES_MM_REDUCE = {
    "tsgu_csr_spmm_reduce_geometry": (_int, [_int, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_spmm_reduce": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _int, _ptr, _i64, _ptr, _i64, _int, _ptr]),
    "tsgu_csr_spmm_reduce_backward_values": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _i64, _ptr, _int, _ptr]),
    "tsgu_csr_spmm_reduce_backward_dense": (
        _int, [_int, _int, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _ptr, _i64, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_spgemm.h (same library, same ABI version)
SIGNATURES_SPGEMM = {
    "tsgu_spgemm_bins": (_int, [ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_spgemm_row_bound": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_spgemm_symbolic": (
        _int, [_int, _int, _i64, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_spgemm_numeric": (
        _int, [_int, _int, _int, _i64, _ptr, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_spgemm_grad_a": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_spgemm_grad_b": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_bsr.h (same library, same ABI version)
SIGNATURES_BSR = {
    "tsgu_bsr_mm_geometry": (_int, [_int, _i64, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_bsr_spmm": (_int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _i64, _int, _ptr]),
    "tsgu_bsr_sddmm": (_int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _i64, _ptr, _int, _ptr]),
    "tsgu_bsr_spmm_t": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _i64, _ptr, _i64, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_bsr_attention.h (same library, same ABI version)
SIGNATURES_BSR_ATTENTION = {
    "tsgu_bsr_attention_supported": (_int, [_int, _int, _int, _i64, _i64]),
    "tsgu_bsr_attention_geometry": (_int, [_int, _int, _int, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_bsr_attention": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _int, _int, _dbl, _ptr,
               _i64, _ptr, _ptr, _int, _ptr]),
    "tsgu_bsr_attention_backward_rows": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64,
               _ptr, _int, _int, _dbl, _ptr, _i64, _ptr, _ptr, _int, _ptr]),
    "tsgu_bsr_attention_backward_cols": (
        _int, [_int, _int, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr,
               _ptr, _int, _int, _dbl, _ptr, _i64, _ptr, _i64, _int, _ptr]),
}

# the additive entries of include/tsgu_hip_factor.h (same library, same ABI version)
_FACTOR_ARGS = [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _dbl, _ptr, _ptr, _ptr, _int, _int, _ptr]
SIGNATURES_FACTOR = {
    "tsgu_csr_factor_work_bytes": (_i64, [_i64]),
    "tsgu_csr_factor_geometry": (_int, [_int, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_ilu0": (_int, list(_FACTOR_ARGS)),
    "tsgu_csr_ic0": (_int, list(_FACTOR_ARGS)),
}

# the additive entries of include/tsgu_hip_fsai.h (same library, same ABI version)
SIGNATURES_FSAI = {
    "tsgu_csr_fsai_geometry": (_int, [_int, ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_fsai": (_int, [_int, _int, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _int, _int, _ptr]),
}

# header of include/ -> its table: all that `load_library` binds (a header that is missing here would load with ctypes' default int
# signatures; tests/test_abi_conformance_cpu.py holds this mapping against the directory)
ABI = {
    "tsgu_hip.h": SIGNATURES,
    "tsgu_hip_softmax.h": SIGNATURES_SOFTMAX,
    "tsgu_hip_attention.h": SIGNATURES_ATTENTION,
    "tsgu_hip_mm_reduce.h": SIGNATURES_MM_REDUCE,
    "tsgu_hip_spgemm.h": SIGNATURES_SPGEMM,
    "tsgu_hip_bsr.h": SIGNATURES_BSR,
    "tsgu_hip_bsr_attention.h": SIGNATURES_BSR_ATTENTION,
    "tsgu_hip_factor.h": SIGNATURES_FACTOR,
    "tsgu_hip_fsai.h": SIGNATURES_FSAI,
}

# the additive entries of csrc/tsgu_hip_lobpcg.h (same library, same ABI version): a STAGED header, declared beside the sources
# until it moves to include/ ("Adding a header")
SIGNATURES_LOBPCG = {
    "tsgu_tall_geometry": (_int, [_int, _i64, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
                                  ctypes.POINTER(_i64)]),
    "tsgu_tall_gram": (_int, [_int, _i64, _i64, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _int, _int, _ptr]),
    "tsgu_tall_combine": (_int, [_int, _i64, _int, _ptr, _ptr, _ptr, _int, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_lobpcg_residual": (_int, [_int, _i64, _i64, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _i64, _int, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after `ABI` (tests/test_sparse_lobpcg_cpu.py holds it against the header)
STAGED = {"tsgu_hip_lobpcg.h": SIGNATURES_LOBPCG}

# the additive entries of csrc/tsgu_hip_amg.h (same library, same ABI version): the second STAGED header.  It has a registry of its
# own because tests pin `ABI` against include/ and `STAGED` to the LOBPCG table ("Adding a header")
SIGNATURES_AMG = {
    "tsgu_amg_geometry": (_int, [ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_csr_amg_hop": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_amg_mis2_update": (_int, [_int, _i64, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_csr_affine_spmm": (_int, [_int, _int, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _dbl,
                                    _ptr, _i64, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after `ABI` and `STAGED` (tests/test_sparse_amg_cpu.py holds it against the header)
STAGED_AMG = {"tsgu_hip_amg.h": SIGNATURES_AMG}

# the additive entries of csrc/tsgu_hip_gmres.h (same library, same ABI version): the third STAGED header, in a registry of its own
# for the same reason (tests pin `ABI`, `STAGED` and `STAGED_AMG`)
SIGNATURES_GMRES = {
    "tsgu_gmres_geometry": (_int, [_int, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_i64),
                                   ctypes.POINTER(_i64)]),
    "tsgu_gmres_project": (_int, [_int, _i64, _i64, _int, _ptr, _ptr, _i64, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_gmres_subtract": (_int, [_int, _i64, _i64, _int, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_gmres_scale": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_gmres_scalar": (_int, [_int, _int, _int, _int, _ptr, _i64, _ptr, _ptr, _ptr, _dbl, _dbl, _int, _i64, _int, _ptr]),
    "tsgu_gmres_update": (_int, [_int, _i64, _i64, _int, _ptr, _ptr, _i64, _ptr, _ptr, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after `ABI`, `STAGED` and `STAGED_AMG` (tests/test_gmres_cpu.py holds it
# against the header)
STAGED_GMRES = {"tsgu_hip_gmres.h": SIGNATURES_GMRES}

# the additive entries of csrc/tsgu_hip_color.h (same library, same ABI version): the fourth STAGED header, in a registry of its
# own for the same reason (tests pin `ABI`, `STAGED`, `STAGED_AMG` and `STAGED_GMRES`)
SIGNATURES_COLOR = {
    "tsgu_color_geometry": (_int, [ctypes.POINTER(_int)] * 6),
    "tsgu_csr_color_round": (_int, [_int, _i64, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _int, _ptr]),
    "tsgu_csr_color_check": (_int, [_int, _i64, _i64, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _i64, _ptr, _int, _int, _ptr]),
    "tsgu_csr_color_sweep": (_int, [_int, _int, _int, _i64, _i64, _i64, _i64, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64,
                                    _ptr, _ptr, _i64, _ptr, _i64, _ptr, _int, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_coloring_cpu.py holds it against
# the header)
STAGED_COLOR = {"tsgu_hip_color.h": SIGNATURES_COLOR}

# the additive entries of csrc/tsgu_hip_quadrature.h (same library, same ABI version): the fifth STAGED header, in a registry of its
# own for the same reason (tests pin `ABI` and the four registries above)
SIGNATURES_QUADRATURE = {
    "tsgu_quadrature_geometry": (_int, [ctypes.POINTER(_int), ctypes.POINTER(_i64)]),
    "tsgu_tridiag_quadrature": (_int, [_int, _int, _int, _int, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_rademacher_fill": (_int, [_int, _i64, _i64, _i64, _ptr, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_logdet_cpu.py holds it
# against the header)
STAGED_QUADRATURE = {"tsgu_hip_quadrature.h": SIGNATURES_QUADRATURE}

# the additive entries of csrc/tsgu_hip_ciq.h (same library, same ABI version): the sixth STAGED header, in a registry of its own
# for the same reason (tests pin `ABI` and the five registries above)
SIGNATURES_CIQ = {
    "tsgu_ciq_geometry": (_int, [_int, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_i64),
                                 ctypes.POINTER(_i64)]),
    "tsgu_ciq_update": (_int, [_int, _i64, _i64, _int, _ptr, _ptr, _ptr, _ptr, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_ciq_stop": (_int, [_int, _i64, _int, _ptr, _dbl, _ptr, _ptr, _ptr, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_sqrt_cpu.py holds it against
# the header)
STAGED_CIQ = {"tsgu_hip_ciq.h": SIGNATURES_CIQ}

# the additive entries of csrc/tsgu_hip_expm.h (same library, same ABI version): the seventh STAGED header, in a registry of its own
# for the same reason (tests pin `ABI` and the six registries above)
SIGNATURES_EXPM = {
    "tsgu_expm_geometry": (_int, [_int, _i64, _i64, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
                                  ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "tsgu_cheb_step": (_int, [_int, _i64, _i64, _ptr, _ptr, _ptr, _dbl, _dbl, _dbl, _ptr, _int, _int, _ptr, _int, _int, _ptr, _int, _ptr]),
    "tsgu_cheb_combine": (_int, [_int, _int, _int, _i64, _i64, _int, _int, _ptr, _ptr, _ptr, _i64, _ptr, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_expm_cpu.py holds it against
# the header)
STAGED_EXPM = {"tsgu_hip_expm.h": SIGNATURES_EXPM}

# the additive entries of csrc/tsgu_hip_topk.h (same library, same ABI version): the eighth STAGED header, in a registry of its own
# for the same reason (tests pin `ABI` and the seven registries above)
SIGNATURES_TOPK = {
    "tsgu_topk_geometry": (_int, [_int, _i64, _int, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
                                  ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "tsgu_topk_mm": (_int, [_int, _ptr, _ptr, _ptr, _i64, _i64, _i64, _int, _dbl, _int, _i64, _ptr, _ptr, _ptr, _int, _i64, _i64, _i64,
                            _i64, _i64, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_topk_cpu.py holds it against
# the header)
STAGED_TOPK = {"tsgu_hip_topk.h": SIGNATURES_TOPK}

# the additive entries of csrc/tsgu_hip_semi.h (same library, same ABI version): the ninth STAGED header, in a registry of its own
# for the same reason (tests pin `ABI` and the eight registries above)
SIGNATURES_SEMI = {
    "tsgu_semi_geometry": (_int, [_int, _i64, ctypes.POINTER(_i64), ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int),
                                  ctypes.POINTER(_int)]),
    "tsgu_semi_prune": (_int, [_int, _ptr, _i64, _i64, _i64, _ptr, _i64, _ptr, _i64, _int, _ptr]),
    "tsgu_semi_expand": (_int, [_int, _ptr, _i64, _ptr, _i64, _i64, _i64, _ptr, _i64, _int, _ptr]),
    "tsgu_semi_mm": (_int, [_int, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _ptr, _i64, _i64, _i64, _i64, _int, _int, _int, _ptr]),
    "tsgu_semi_mm_t": (_int, [_int, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr]),
    "tsgu_semi_sddmm": (_int, [_int, _ptr, _i64, _ptr, _i64, _ptr, _i64, _ptr, _i64, _i64, _i64, _i64, _int, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_semi_structured_cpu.py holds
# it against the header)
STAGED_SEMI = {"tsgu_hip_semi.h": SIGNATURES_SEMI}

# the additive entries of csrc/tsgu_hip_sinkhorn.h (same library, same ABI version): the tenth STAGED header, in a registry of its own
# for the same reason (tests pin `ABI` and the nine registries above)
SIGNATURES_SINKHORN = {
    "tsgu_sinkhorn_workspace": (_int, [_int, _i64, ctypes.POINTER(_i64)]),
    "tsgu_sinkhorn_half": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _int, _ptr]),
    "tsgu_sinkhorn_plan": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int, _ptr]),
    "tsgu_sinkhorn_half_backward": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _int,
                                           _ptr, _i64, _int, _ptr]),
    "tsgu_segment_sum": (_int, [_int, _int, _i64, _i64, _ptr, _ptr, _ptr, _ptr, _ptr, _ptr, _i64, _int, _ptr]),
}

# header of csrc/ -> its table: bound by `load_library` after the registries above (tests/test_sparse_sinkhorn_cpu.py holds it
# against the header)
STAGED_SINKHORN = {"tsgu_hip_sinkhorn.h": SIGNATURES_SINKHORN}


class HipExtensionMissing(RuntimeError):
    pass


def load_library():
    """Load (once) and return the ctypes handle; raises if the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise HipExtensionMissing(
                f"{LIB_PATH} not found: build the gfx950 extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C torchsparsegradutils_amd/csrc). "
                "torchsparsegradutils_amd has no CPU or eager fallback."
            )
        # torch has already loaded its libamdhip64.so (same SONAME), so the kernels register
        # with the runtime that owns torch's streams and allocations.
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for table in (*ABI.values(), *STAGED.values(), *STAGED_AMG.values(), *STAGED_GMRES.values(),
                      *STAGED_COLOR.values(), *STAGED_QUADRATURE.values(), *STAGED_CIQ.values(), *STAGED_EXPM.values(),
                      *STAGED_TOPK.values(), *STAGED_SEMI.values(), *STAGED_SINKHORN.values()):
            for name, (res, args) in table.items():
                fn = getattr(lib, name)  # AttributeError => header/library mismatch, fail loudly
                fn.restype = res
                fn.argtypes = args
        if lib.tsgu_abi_version() != ABI_VERSION:
            raise HipExtensionMissing("libtsgu_hip.so ABI version mismatch; rebuild the extension")
        _lib = lib
    return _lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load_library().tsgu_status_string(status).decode()
        raise RuntimeError(f"{what} failed: {msg} (tsgu status {status})")


def _query(name: str, *args):
    """A host-only query entry of the library: `name` called with `args` followed by one zeroed slot for each out-parameter its
    signature has left (`int*` / `int64_t*`).  Returns the slots' values as Python ints; raises through `check` under the name."""
    fn = getattr(load_library(), name)
    outs = [t._type_(0) for t in fn.argtypes[len(args):]]
    check(fn(*args, *map(ctypes.byref, outs)), name)
    return tuple(int(o.value) for o in outs)


def vtype_of(t: torch.Tensor) -> int:
    try:
        return _VTYPE[t.dtype]
    except KeyError:
        raise RuntimeError(f"torchsparsegradutils_amd: unsupported value dtype {t.dtype}") from None


def itype_of(t: torch.Tensor) -> int:
    try:
        return _ITYPE[t.dtype]
    except KeyError:
        raise RuntimeError(f"torchsparsegradutils_amd: unsupported index dtype {t.dtype}") from None


def operand_device(*tensors: torch.Tensor) -> torch.device:
    """The one device all operands of a call live on (CPU included: CPU operands are computed by the torch-op path, _cpu.py;
    the HIP bindings below still refuse them through `require_device`)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"all operands must be on the same device, got {dev} and {t.device}")
    return dev


def require_device(*tensors: torch.Tensor) -> torch.device:
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                f"the gfx950 kernels of torchsparsegradutils_amd were handed a tensor on '{t.device}': CPU operands are served by "
                "the torch-op path (_cpu.py) only when ALL operands of a call live on the CPU"
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"all operands must be on the same device, got {dev} and {t.device}")
    return dev


def _raw_stream(dev: torch.device) -> int:
    """Current HIP stream of `dev` as an integer handle (the accessor torch's own generated code uses: 0.1 us instead of 2)."""
    return torch._C._cuda_getCurrentRawStream(dev.index)


def launch(name: str, dev: torch.device, *args) -> None:
    """The one way a kernel launch crosses the C ABI: calls the library's `name` with `args` — tensors as their data pointers,
    None as NULL, everything else (sizes, flags, addresses that are already integers) as it is — followed by the device index
    and the current stream of `dev`, and raises through `check` under the name that was called.  The stream is read here, at
    call time: the same closure runs eagerly and under graph capture.  `dev` is made current only when it is not already
    (`torch.cuda.device` costs ~8 us per launch; the library sets the device itself, the context puts torch's back)."""
    fn = getattr(_lib or load_library(), name)
    argv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if torch.cuda.current_device() == dev.index:
        rc = fn(*argv, dev.index, _raw_stream(dev))
    else:
        with torch.cuda.device(dev):
            rc = fn(*argv, dev.index, _raw_stream(dev))
    if rc:
        check(rc, name)


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def is_transposed_view(t: torch.Tensor) -> bool:
    """2-D operand with unit ROW stride (``x.t()`` of a contiguous matrix — what ``bvec.t()`` in the reference's sparse
    multivariate normal hands over, distributions/sparse_multivariate_normal.py:96): consumed in place by K1 / K4."""
    return t.dim() == 2 and t.size(0) > 1 and t.size(1) > 1 and t.stride(0) == 1 and t.stride(1) >= t.size(0)


def strided2d(t: torch.Tensor):
    """(tensor, row stride, column stride) for a 2-D dense operand WITHOUT copying when it is row-major or a
    transposed view; anything else is made contiguous."""
    if is_transposed_view(t):
        return t, 1, t.stride(1)
    t = rowmajor(t)
    return t, _ld(t), 1


def rowmajor(t: torch.Tensor) -> torch.Tensor:
    """Return `t` (2-D or 3-D) with unit stride in the last dim and a sane leading dimension."""
    if t.is_contiguous():
        return t
    if t.stride(-1) != 1 and t.size(-1) != 1:
        return t.contiguous()
    if t.dim() >= 2 and t.size(-2) > 1 and t.stride(-2) < t.size(-1):
        return t.contiguous()
    if t.dim() == 3 and t.size(0) > 1 and t.stride(0) < t.size(1) * t.stride(1):
        return t.contiguous()
    if t.size(-1) == 1 and t.stride(-1) != 1:
        return t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return t.stride(-2) if t.size(-2) > 1 else max(t.size(-1), 1)


def _bs(t: torch.Tensor) -> int:
    return t.stride(0) if (t.dim() == 3 and t.size(0) > 1) else 0


def csr_spmm(crow, col, val, B, n_rows: int, n_cols: int, perm=None, out=None, dot_w=None, max_row_nnz: int = 0):
    """C = A·B for (batched) CSR arrays.  B: (m, p) or (b, m, p).  Returns C or (C, dot_partial).
    A 2-D B that is a transposed view is consumed in place and C comes back in the same (transposed) layout."""
    lib = load_library()
    dev = require_device(crow, col, val, B, perm, out, dot_w)
    if val.dtype != B.dtype:
        raise RuntimeError(f"expected A and B to have the same dtype, got {val.dtype} and {B.dtype}")
    batched = B.dim() == 3
    batch = B.size(0) if batched else 1
    p = B.size(-1)
    b_cs = 1
    if not batched and dot_w is None and out is None:
        B, ldb, b_cs = strided2d(B)
    else:
        B = rowmajor(B)
        ldb = _ld(B)
    nnz = col.size(-1)
    crow, col, val = crow.contiguous(), col.contiguous(), val.contiguous()
    if perm is not None:
        perm = perm.contiguous()
    shape = (batch, n_rows, p) if batched else (n_rows, p)
    c_cs = 1
    if out is None:
        if b_cs != 1:
            out = torch.empty((p, n_rows), dtype=B.dtype, device=dev).t()   # same layout as the operand: coalesced stores
            ldc, c_cs = 1, n_rows
        else:
            out = torch.empty(shape, dtype=B.dtype, device=dev)
            ldc = _ld(out)
    else:
        ldc = _ld(out)
    partial = None
    vt = vtype_of(val)
    if dot_w is not None:
        nblk = lib.tsgu_spmm_num_blocks(vt, n_rows, nnz, p, max_row_nnz)
        partial = torch.empty((batch * nblk, p), dtype=B.dtype, device=dev)
        dot_w = rowmajor(dot_w)
    launch("tsgu_csr_spmm", dev, vt, itype_of(crow), n_rows, n_cols, nnz, crow, col, val, perm, B, ldb, b_cs, _bs(B), out, ldc, c_cs,
           _bs(out), p, batch, max_row_nnz, dot_w, _ld(dot_w) if dot_w is not None else 0, partial)
    return out if dot_w is None else (out, partial)


def csr_sddmm(crow, col, G, B, n_rows: int, n_cols: int, alpha: float = 1.0, swap_roles: bool = False):
    """out[k] = alpha·<G[row k], B[col k]> (or roles swapped) for (batched) CSR patterns."""
    dev = require_device(crow, col, G, B)
    if G.dtype != B.dtype:
        raise RuntimeError(f"expected both dense operands to have the same dtype, got {G.dtype} and {B.dtype}")
    batched = G.dim() == 3
    batch = G.size(0) if batched else 1
    p = G.size(-1)
    G, B = rowmajor(G), rowmajor(B)
    crow, col = crow.contiguous(), col.contiguous()
    nnz = col.size(-1)
    out = torch.empty(col.shape, dtype=G.dtype, device=dev)
    launch("tsgu_csr_sddmm", dev, vtype_of(G), itype_of(crow), n_rows, n_cols, nnz, crow, col, G, _ld(G), _bs(G), B, _ld(B), _bs(B), out,
           float(alpha), int(bool(swap_roles)), p, batch)
    return out


def csr_mm_backward(tplan, val, G, B, n_rows: int, n_cols: int):
    """(gradA values in A's order, gradB) in one pass over the transposed plan `tplan` of A."""
    dev = require_device(tplan.crow, val, G, B)
    if not (val.dtype == G.dtype == B.dtype):
        raise RuntimeError("expected A, B and the upstream gradient to have the same dtype")
    batched = G.dim() == 3
    batch = G.size(0) if batched else 1
    p = G.size(-1)
    G, B = rowmajor(G), rowmajor(B)
    val = val.contiguous()
    gradA = torch.empty(val.shape, dtype=val.dtype, device=dev)
    gradB = torch.empty(B.shape, dtype=B.dtype, device=dev)
    launch("tsgu_csr_mm_backward", dev, vtype_of(val), itype_of(tplan.crow), n_rows, n_cols, tplan.col.size(-1), tplan.crow, tplan.col,
           tplan.perm, val, G, _ld(G), _bs(G), B, _ld(B), _bs(B), gradA, gradB, _ld(gradB), _bs(gradB), p, batch)
    return gradA, gradB


def fused_backward_supported(dtype: torch.dtype, p: int) -> bool:
    wide = {torch.float32: 4, torch.bfloat16: 8}.get(dtype)
    if wide is None or p <= 0:
        return False
    vec = wide if p % wide == 0 else 1
    return (p + vec - 1) // vec <= 64


CSR_SPMM, CSR_SDDMM, COO_SDDMM, CSR_MM_BACKWARD = 0, 1, 2, 3


def csr_geometry(kernel: int, dtype: torch.dtype, n_rows: int, nnz: int, p: int, max_row_nnz: int = 0, wide_ok: bool = True,
                 col_strided: bool = False):
    """(vec, column_lanes, entry_lanes, column_tiles, row_runs, stage_entries) of a plan-free kernel (`CSR_SPMM`, `CSR_SDDMM`,
    `COO_SDDMM`, `CSR_MM_BACKWARD`) for these sizes, answered on the host by the launchers' own rules; raises where they refuse."""
    return _query("tsgu_csr_geometry", int(kernel), _VTYPE[dtype], int(n_rows), int(nnz), int(p), int(max_row_nnz), int(bool(wide_ok)),
                  int(bool(col_strided)))


class _RowpackPlanStruct(ctypes.Structure):
    """``tsgu_rowpack_plan`` of include/tsgu_hip.h."""

    _fields_ = [("nblocks", _i64), ("ecap", ctypes.c_int32), ("ucap", ctypes.c_int32), ("nclasses", ctypes.c_int32),
                ("rows_per_group", ctypes.c_int32)] + [(k, _ptr) for k in ("uptr", "ucol", "upos", "sperm", "order", "vpair", "eptr",
                                                                     "wcls", "wbase", "cne", "srcstart")]


def _plan_struct(rp):
    """ctypes image of a _pattern.RowPackPlan (cached on the plan; the plan keeps the tensors alive)."""
    st = rp._cstruct
    if st is None:
        st = _RowpackPlanStruct(rp.nblocks, rp.ecap, rp.ucap, rp.nclasses, rp.group, _p(rp.uptr), _p(rp.ucol), _p(rp.upos), _p(rp.sperm),
                                _p(rp.order), _p(rp.vpair), _p(rp.eptr), _p(rp.wcls), _p(rp.wbase), _p(rp.cne), _p(rp.srcstart))
        rp._cstruct = st
    return ctypes.addressof(st)


@functools.lru_cache(maxsize=None)
def rowpack_geometry(dtype: torch.dtype, p: int):
    """(rows_per_block, (max_entries, max_union, lds_budget_bytes), entry_lanes) of the row-pair gather kernels, or None."""
    if dtype not in (torch.float32, torch.bfloat16) or p <= 0:
        return None
    lib = load_library()
    r, e, a, b, c = _int(0), _int(0), _int(0), _int(0), _int(0)
    if lib.tsgu_rowpack_geometry(_VTYPE[dtype], p, ctypes.byref(r), ctypes.byref(e), ctypes.byref(a), ctypes.byref(b),
                                 ctypes.byref(c)) != 0:
        return None
    return r.value, (a.value, b.value, c.value), e.value


def csr_spmm_rowpack(crow, val, rp, B, n_rows: int):
    """C = A·B through the row-pair union walk; `rp` is a _pattern.RowPackPlan of the walked pattern."""
    dev = require_device(crow, val, B)
    B = rowmajor(B)
    p = B.size(-1)
    out = torch.empty((n_rows, p), dtype=B.dtype, device=dev)
    launch("tsgu_csr_spmm_rowpack", dev, vtype_of(val), itype_of(crow), n_rows, B.size(0), rp.nnz, crow, _plan_struct(rp), val.contiguous(),
           B, _ld(B), out, _ld(out), p)
    return out


def csr_sddmm_rowpack(crow, rp, R, Cm, n_rows: int, alpha: float = 1.0):
    """out[k] = alpha·<R[row k], Cm[col k]> in stored order through the row-pair union walk (plan of a stored-order pattern)."""
    dev = require_device(crow, R, Cm)
    R, Cm = rowmajor(R), rowmajor(Cm)
    p = R.size(-1)
    out = torch.empty((rp.nnz,), dtype=R.dtype, device=dev)
    launch("tsgu_csr_sddmm_rowpack", dev, vtype_of(R), itype_of(crow), n_rows, Cm.size(0), rp.nnz, crow, _plan_struct(rp), R, _ld(R), Cm,
           _ld(Cm), out, float(alpha), p)
    return out


# ---- row-block tile kernels (csrc/tile_impl.h) --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tile_geometry(dtype: torch.dtype, p: int):
    """(rows_per_block, max_union, max_entries) of the tile kernels for (dtype, p), or None when they are not compiled for it."""
    if dtype != torch.float32 or p <= 0:
        return None
    lib = load_library()
    r, u, e = _int(0), _int(0), _int(0)
    if lib.tsgu_tile_geometry(_VTYPE[dtype], p, ctypes.byref(r), ctypes.byref(u), ctypes.byref(e)) != 0:
        return None
    return r.value, u.value, e.value


def _tile_struct(tp):
    st = tp._cstruct
    if st is None:
        from ._tile import TilePlanStruct

        st = TilePlanStruct(tp.n_rows, tp.n_cols, tp.nnz, tp.n_blocks, tp.rows_per_block, tp.max_union, tp.max_entries, 0, _p(tp.desc),
                            _p(tp.ucol), _p(tp.lidx), _p(tp.rptr), _p(tp.cpos), _p(tp.cslot), _p(tp.ent), _p(tp.xrow))
        tp._cstruct = st
    return ctypes.addressof(st)


def csr_spmm_tile(tp, val, B):
    """C = A·B (a plan with value chunks `cpos` / `cslot`: Aᵀ·G through A's own values) by the row-block tile walk."""
    dev = require_device(val, B)
    B = rowmajor(B)
    p = B.size(-1)
    out = torch.empty((tp.n_rows, p), dtype=B.dtype, device=dev)
    launch("tsgu_csr_spmm_tile", dev, vtype_of(val), _tile_struct(tp), val.contiguous(), B, _ld(B), out, _ld(out), p)
    return out


def csr_sddmm_tile(tp, R, Cm, alpha: float = 1.0):
    """out[k] = alpha·<R[row k], Cm[col k]> in stored order by the row-block tile walk (plan of a stored-order pattern)."""
    dev = require_device(R, Cm)
    R, Cm = rowmajor(R), rowmajor(Cm)
    p = R.size(-1)
    out = torch.empty((tp.nnz,), dtype=R.dtype, device=dev)
    launch("tsgu_csr_sddmm_tile", dev, vtype_of(R), _tile_struct(tp), R, _ld(R), Cm, _ld(Cm), out, float(alpha), p)
    return out


def csr_mm_backward_rowpack(tcrow, rp, val, G, B, n_rows_t: int):
    """(gradA values in A's order, gradB) in one pass over the transposed pattern's RowPackPlan."""
    dev = require_device(tcrow, val, G, B)
    G, B = rowmajor(G), rowmajor(B)
    p = G.size(-1)
    val = val.contiguous()
    grad_a = torch.empty_like(val)
    grad_b = torch.empty((n_rows_t, p), dtype=G.dtype, device=dev)
    launch("tsgu_csr_mm_backward_rowpack", dev, vtype_of(val), itype_of(tcrow), n_rows_t, G.size(0), rp.nnz, tcrow, _plan_struct(rp), val, G,
           _ld(G), B, _ld(B), grad_a, grad_b, _ld(grad_b), p)
    return grad_a, grad_b


# ---- lattice plane-sweep kernels (csrc/lattice_impl.h; plans from _lattice.py) -------------------------------
LAT_SPMM, LAT_SDDMM, LAT_SPMMT = 0, 1, 2


def lattice_lds_bytes(mode: int, vtype: int, p: int, ty: int, tz: int, ry: int, rz: int, nloc: int, recw: int, threads: int,
                      ring: int = 4, cpl: int = 1) -> int:
    """Dynamic LDS bytes of a lattice launch configuration, or a negative tsgu status when it does not fit."""
    return int(load_library().tsgu_lattice_lds_bytes(mode, vtype, p, ty, tz, ry, rz, nloc, recw, threads, ring, cpl))


_LATTICE_ELEMENT_BYTES = {torch.float32: 4, torch.bfloat16: 2, torch.float64: 8}


def lattice_rows_fit(mode: int, dtype: torch.dtype, p: int, stored_order: bool = True) -> bool:
    """Are the sweeps compiled for dense rows of p `dtype` values: whole 16-byte lanes, 1, 2, 4, 8 or 16 of them — one lane per row
    (4 fp32 columns) for the product in the stored order (`stored_order`: the walked plan is not the transposed one) only."""
    es = _LATTICE_ELEMENT_BYTES.get(dtype)
    if es is None or (p * es) % 16:
        return False
    lanes = (p * es) // 16
    return lanes in (2, 4, 8, 16) or (lanes == 1 and mode == LAT_SPMM and dtype == torch.float32 and stored_order)


def lattice_config(lp, mode: int, dtype: torch.dtype, p: int):
    """Launch configuration (tile, segments, record tables) of the _lattice.LatticePlan `lp` for these operands, or None."""
    from . import _lattice

    if not lattice_rows_fit(mode, dtype, p, lp.kind == 0):
        return None
    return _lattice.config_for(lp, mode, _VTYPE[dtype], p, _LATTICE_ELEMENT_BYTES[dtype], lattice_lds_bytes, be=sys.modules[__name__])


def lattice_tune(lp, mode: int, dtype: torch.dtype, p: int, time_ms):
    """Measured choice among the best-ranked launch configurations of `lp` for these operands (`_lattice.tune_config`)."""
    from . import _lattice

    return _lattice.tune_config(lp, mode, _VTYPE[dtype], p, _LATTICE_ELEMENT_BYTES[dtype], lattice_lds_bytes, sys.modules[__name__], time_ms)


def lattice_rows(crow, col, dims, status, slot, thash=None, trep=None, remap=None, ctable=None, lens=None, rcls=None, disp=None,
                 box_mask: int = 0, periodic: int = 0):
    """Row analysis kernels of csrc/lattice_plan.hip: pass 1 (hash -> slot table) when `ctable` is None, pass 2 (class
    assignment + exact check) otherwise; the rows of the transposed pattern when `disp` is given.  `box_mask` / `periodic`
    (pass 2 of the stored-order walk): also the plane-march condition, status[4]."""
    dev = require_device(crow, col, status)
    nb, nx, ny, nz = dims
    launch("tsgu_lattice_rows", dev, itype_of(crow), crow.numel() - 1, crow, col, nb, nx, ny, nz, disp, 0 if disp is None else disp.numel(),
           slot, thash, trep, remap, ctable, lens, rcls, status, int(box_mask), int(periodic))


def lattice_block_classes(rcls, n_rows, dims, ty, tz, nseg, mask):
    dev = require_device(rcls, mask)
    nb, nx, ny, nz = dims
    launch("tsgu_lattice_block_classes", dev, n_rows, rcls, nb, nx, ny, nz, ty, tz, nseg, mask)


def lattice_row_codes(crow, col, dims, rows, out, disp=None):
    dev = require_device(crow, col, rows, out)
    nb, nx, ny, nz = dims
    launch("tsgu_lattice_row_codes", dev, itype_of(crow), crow.numel() - 1, crow, col, nb, nx, ny, nz, disp, 0 if disp is None else disp.numel(),
           rows, rows.numel(), out)


def march_lds_bytes(mode: int, vtype: int, p: int, ty: int, tz: int, ry: int, rz: int, ncls: int, threads: int) -> int:
    """Dynamic LDS bytes of a plane-march launch configuration (csrc/march_impl.h), or a negative tsgu status."""
    return int(load_library().tsgu_march_lds_bytes(mode, vtype, p, ty, tz, ry, rz, ncls, threads))


def march_supported(mode: int, mask: int, uniform_len: int, threads: int) -> bool:
    """Is there a plane-march kernel for this product / displacement set / row form / workgroup size (csrc/march_sets.h)?"""
    return bool(load_library().tsgu_march_supported(mode, mask, uniform_len, threads))


def march_config(lp, mode: int, dtype: torch.dtype, p: int):
    """Launch configuration of the plane-march kernels for the stored-order _lattice.LatticePlan `lp`, or None when the pattern
    is not a full periodic box stencil / the operands are not covered (fp32, 32 or 64 columns)."""
    from . import _lattice

    if lp is None or lp.kind != 0:
        return None
    if dtype == torch.bfloat16:      # whole-line march (csrc/linemarch_impl.h): Aᵀ·G of a periodic 27-point stencil at 16 columns
        return _lattice.linemarch_config_for(lp, mode, _VTYPE[dtype], p, march_lds_bytes)
    if dtype != torch.float32:
        return None
    return _lattice.march_config_for(lp, mode, _VTYPE[dtype], p, march_lds_bytes, march_supported)


# Per-kernel timing hook (bench.py): a list to which the lattice launchers append (name, start event, end event) recorded on the
# launch stream around the C call.  None = off (the product never pays for it).
KERNEL_EVENTS = None


def _timed(name: str, dev: torch.device):
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record(torch.cuda.current_stream(dev))
    return name, ev


def _timed_end(tok, dev: torch.device) -> None:
    tok[1][1].record(torch.cuda.current_stream(dev))
    KERNEL_EVENTS.append((tok[0], tok[1][0], tok[1][1]))


def csr_spmm_lattice(lp, cfg, val, B, dot: bool = False, skip: int = 0, dot_w=None, out=None):
    """C = A·B (plan kind 0) or Aᵀ·B for the transposed plan (kind 1; `val` in A's own order) by the plane sweep / plane march.
    `dot` (plane sweep, fp32, stored order): also the per-workgroup partial sums of <C[row], B[row]> per column — returns
    (C, partial [workgroups][p]), the Krylov loops' fused dot epilogue; `skip` (with `dot`): address of a device int32 — the launch
    does nothing when it is non-zero (iterations queued past the end of a solve); `dot_w` (with `dot`): the partial sums are of
    <C[row], dot_w[row]> instead; `out` (with `dot`): a contiguous (n_rows, p) tensor that receives C."""
    dev = B.device
    if not B.is_cuda or val.device != dev:
        require_device(val, B)
        raise RuntimeError(f"all operands must be on the same device, got {val.device} and {dev}")
    if not B.is_contiguous():
        B = rowmajor(B)
    p = B.size(-1)
    n_rows = lp.n_rows
    if out is None or not dot:
        out = torch.empty((n_rows, p), dtype=B.dtype, device=dev)
    if not val.is_contiguous():
        val = val.contiguous()
    march = getattr(cfg, "march", False)
    transposed = cfg.mode == LAT_SPMMT if march else bool(lp.kind)
    if dot:
        if march or transposed or B.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("csr_spmm_lattice: the dot epilogue exists for the fp32 / fp64 stored-order plane sweep only")
        nwg = lp.nb * cfg.nseg * -(-lp.ny // cfg.ty) * -(-lp.nz // cfg.tz)
        partial = torch.empty((nwg, p), dtype=B.dtype, device=dev)
        launch("tsgu_csr_spmm_lattice_dot", dev, _VTYPE[val.dtype], cfg.struct_addr, n_rows, lp.nnz, val, B, _ld(B), out, p, p, partial, nwg,
               skip or None, dot_w)
        return out, partial
    tok = _timed("lattice_spmm_t" if transposed else "lattice_spmm", dev) if KERNEL_EVENTS is not None else None
    ldb = B.stride(0) if B.size(0) > 1 else max(p, 1)
    if march:
        ct = cfg.col_tile          # operands wider than 64 columns: one launch per tile of 64 columns
        vt, bp, op = _VTYPE[val.dtype], B.data_ptr(), out.data_ptr()
        for j in range(0, p, ct):
            launch("tsgu_csr_spmm_march", dev, vt, cfg.struct_addr, int(transposed), n_rows, lp.nnz, val, bp + j * 4, ldb, op + j * 4, p, ct)
    else:
        launch("tsgu_csr_spmm_lattice", dev, _VTYPE[val.dtype], cfg.struct_addr, n_rows, lp.nnz, val, B, ldb, out, p, p)
    if tok is not None:
        _timed_end(tok, dev)
    return out


def csr_sddmm_lattice(lp, cfg, R, Cm, alpha: float = 1.0):
    """out[k] = alpha·<R[row k], Cm[col k]> in stored order by the plane sweep (plan kind 0)."""
    dev = R.device
    if not R.is_cuda or Cm.device != dev:
        require_device(R, Cm)
        raise RuntimeError(f"all operands must be on the same device, got {Cm.device} and {dev}")
    if not R.is_contiguous():
        R = rowmajor(R)
    if not Cm.is_contiguous():
        Cm = rowmajor(Cm)
    p = R.size(-1)
    n_rows = lp.n_rows
    out = torch.empty((lp.nnz,), dtype=R.dtype, device=dev)
    tok = _timed("lattice_sddmm", dev) if KERNEL_EVENTS is not None else None
    ldr = R.stride(0) if R.size(0) > 1 else max(p, 1)
    ldc = Cm.stride(0) if Cm.size(0) > 1 else max(p, 1)
    if getattr(cfg, "march", False):
        ct = cfg.col_tile          # operands wider than 64 columns: the dots of the later column tiles are added to the first
        vt, rp, cp = _VTYPE[R.dtype], R.data_ptr(), Cm.data_ptr()
        for j in range(0, p, ct):
            launch("tsgu_csr_sddmm_march", dev, vt, cfg.struct_addr, n_rows, lp.nnz, rp + j * 4, ldr, cp + j * 4, ldc, out, float(alpha),
                   int(j > 0), ct)
    else:
        launch("tsgu_csr_sddmm_lattice", dev, _VTYPE[R.dtype], cfg.struct_addr, n_rows, lp.nnz, R, ldr, Cm, ldc, out, float(alpha), p)
    if tok is not None:
        _timed_end(tok, dev)
    return out


def _tiled_ok(*dense) -> bool:
    return all(t.dim() == 2 and t.data_ptr() % 16 == 0 and (_ld(t) * t.element_size()) % 16 == 0 for t in dense)


def coo_sddmm(row, col, G, B, alpha: float = 1.0):
    if not G.is_cuda and operand_device(row, col, G, B) is not None:
        from . import _cpu

        out = _cpu.coo_sddmm(row, col, G, B)
        return out if alpha == 1.0 else out.mul_(alpha)
    dev = require_device(row, col, G, B)
    if G.dtype != B.dtype:
        raise RuntimeError(f"expected both dense operands to have the same dtype, got {G.dtype} and {B.dtype}")
    G, B = rowmajor(G), rowmajor(B)
    row, col = row.contiguous(), col.contiguous()
    nnz = row.numel()
    out = torch.empty((nnz,), dtype=G.dtype, device=dev)
    launch("tsgu_coo_sddmm", dev, vtype_of(G), itype_of(row), nnz, row, col, G, _ld(G), B, _ld(B), out, float(alpha), G.size(-1))
    return out


def segment_logsumexp_workspace_bytes(dtype: torch.dtype, nnz: int) -> int:
    """Workspace bytes tsgu_segment_logsumexp needs for `nnz` entries of value type `dtype`."""
    return _query("tsgu_segment_logsumexp_workspace", _VTYPE[dtype], nnz)[0]


def segment_logsumexp(ptr, perm, val, out, n_groups: int, nnz: int, include_zeros: bool, axis_len: int,
                      groups_per_item: int, item_stride: int, workspace):
    """out[group] = log Σ exp over the segments [ptr[g], ptr[g+1]) of val (through perm when given), plus the absent entries of
    each group when include_zeros; group g lands at out[(g // groups_per_item) * item_stride + g % groups_per_item] and the
    padding of every item is set to -inf.  `out` may be a view into a larger buffer (only its data pointer is used)."""
    dev = require_device(ptr, perm, val, out, workspace)
    if perm is not None and perm.dtype != ptr.dtype:
        raise RuntimeError(f"index dtypes differ: {ptr.dtype} and {perm.dtype}")
    if out.dtype != val.dtype:
        raise RuntimeError(f"output dtype {out.dtype} differs from the values' {val.dtype}")
    launch("tsgu_segment_logsumexp", dev, vtype_of(val), itype_of(ptr), n_groups, nnz, ptr, perm, val, int(bool(include_zeros)), axis_len, out,
           groups_per_item, item_stride, workspace, workspace.numel() * workspace.element_size())


def segment_logsumexp_backward(val, ptr, g_grp, lse_grp, idx, g_idx, lse_idx, n_groups: int):
    """grad[k] = g_grp[grp(k)]·exp(val[k] − lse_grp[grp(k)]) + g_idx[idx[k]]·exp(val[k] − lse_idx[idx[k]]) in stored order
    (either direction may be None)."""
    dev = require_device(val, ptr, g_grp, lse_grp, idx, g_idx, lse_idx)
    itp = ptr if ptr is not None else idx
    if ptr is not None and idx is not None and ptr.dtype != idx.dtype:
        raise RuntimeError(f"index dtypes differ: {ptr.dtype} and {idx.dtype}")
    for t in (g_grp, lse_grp, g_idx, lse_idx):
        if t is not None and (t.dtype != val.dtype or not t.is_contiguous()):
            raise RuntimeError("group vectors must be contiguous and of the values' dtype")
    grad = torch.empty_like(val)
    launch("tsgu_segment_logsumexp_backward", dev, vtype_of(val), itype_of(itp), val.numel(), val, ptr, n_groups, g_grp, lse_grp, idx, g_idx,
           lse_idx, grad)
    return grad


SOFTMAX_STAGE_BYTES = 8192       # kLseStageBytes of csrc/logsumexp_impl.h: one wave's range is this many bytes of accumulators

# Launch notes of the segmented softmax (tests): a list to which every call appends (entry, kernels launched).  None = off.
SOFTMAX_LAUNCHES = None


def segment_softmax_range(dtype: torch.dtype) -> int:
    """Entries of one range of the segmented softmax kernels for value type `dtype` (bf16 accumulates in fp32)."""
    return SOFTMAX_STAGE_BYTES // (8 if dtype == torch.float64 else 4)


def segment_softmax_workspace_bytes(dtype: torch.dtype, nnz: int) -> int:
    """Workspace bytes the segmented softmax entries need for `nnz` entries of value type `dtype` when groups cross ranges."""
    return _query("tsgu_segment_softmax_workspace", _VTYPE[dtype], nnz)[0]


def _softmax_call(name: str, ptr, perm, operands, n_groups: int, log_form: bool, crossing: bool, out=None):
    """One segmented softmax entry: operands (one input, or two) -> `out` (a new value array when None).  `crossing`: some group
    crosses a range boundary of the kernels (known from the pattern) — only then the workspace and the merge / fix-up launches."""
    first = operands[0]
    if out is None:
        out = torch.empty_like(first)
    dev = require_device(ptr, perm, *operands, out)
    if perm is not None and perm.dtype != ptr.dtype:
        raise RuntimeError(f"index dtypes differ: {ptr.dtype} and {perm.dtype}")
    for t in (*operands, out):
        if t.dtype != first.dtype or t.shape != first.shape or not t.is_contiguous():
            raise RuntimeError("the value arrays must be contiguous, of one dtype and one shape")
    if not ptr.is_contiguous() or (perm is not None and not perm.is_contiguous()) or ptr.numel() != n_groups + 1:
        raise RuntimeError("ptr (n_groups + 1 entries) and perm must be contiguous")
    nnz = first.numel()
    ws = torch.empty(segment_softmax_workspace_bytes(first.dtype, nnz), dtype=torch.uint8, device=dev) if crossing and nnz else None
    launch(name, dev, vtype_of(first), itype_of(ptr), n_groups, nnz, ptr, perm, *operands, int(bool(log_form)), out, ws,
           0 if ws is None else ws.numel())
    if SOFTMAX_LAUNCHES is not None:
        SOFTMAX_LAUNCHES.append((name, ("main", "merge", "fix") if ws is not None else ("main",) if nnz and n_groups else ()))
    return out


def segment_softmax(ptr, perm, val, n_groups: int, log_form: bool, crossing: bool, out=None):
    """y[k'] = softmax (or log-softmax) of val over the segments [ptr[g], ptr[g+1]), k' = perm[k] when perm is given: the result
    is in val's own order."""
    return _softmax_call("tsgu_segment_softmax", ptr, perm, (val,), n_groups, log_form, crossing, out)


def segment_softmax_backward(ptr, perm, y, g, n_groups: int, log_form: bool, crossing: bool, out=None):
    """gin = y·(g − Σ_group g·y), or g − exp(y)·Σ_group g for the log form, in the values' own order."""
    return _softmax_call("tsgu_segment_softmax_backward", ptr, perm, (y, g), n_groups, log_form, crossing, out)


def sinkhorn_workspace_bytes(dtype: torch.dtype, nnz: int) -> int:
    """Workspace bytes the Sinkhorn entries need for `nnz` entries of value type `dtype` when groups cross ranges."""
    return _query("tsgu_sinkhorn_workspace", _VTYPE[dtype], nnz)[0]


def _acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float32 if dtype == torch.bfloat16 else dtype


def _sinkhorn_operands(what: str, dev, val, index, vectors, workspace):
    """The refusals the Sinkhorn wrappers share: `index` [(tensor, entries)] of one dtype, `vectors` [(tensor or None, entries)] of
    the values' accumulator type; everything contiguous.  Returns the workspace's bytes (0 without one)."""
    acc = _acc_dtype(val.dtype)
    if not val.is_contiguous():
        raise RuntimeError(f"{what}: the value array must be contiguous")
    idt = index[0][0].dtype
    for t, n in index:
        if t is not None and (t.dtype != idt or not t.is_contiguous() or t.numel() != n):
            raise RuntimeError(f"{what}: index arrays must be contiguous, of one dtype and of their pattern's sizes")
    for t, n in vectors:
        if t is not None and (t.dtype != acc or not t.is_contiguous() or t.numel() != n):
            raise RuntimeError(f"{what}: group vectors must be contiguous, of dtype {acc} and of their direction's length")
    if workspace is not None and workspace.numel() * workspace.element_size() < sinkhorn_workspace_bytes(val.dtype, val.numel()):
        raise RuntimeError(f"{what}: the workspace is too small")
    return 0 if workspace is None else workspace.numel() * workspace.element_size()


def sinkhorn_half(ptr, perm, idx, val, other, log_marg, out, workspace):
    """out[g] = log_marg[g] − log Σ_{k in group g} exp(val[perm[k]] + other[idx[k]]) over the segments of `ptr` (log_marg None: zeros).
    `out` may be a row of a larger buffer.  `workspace` None: the caller knows that no group crosses a range of the kernels."""
    dev = require_device(ptr, perm, idx, val, other, log_marg, out, workspace)
    n, nnz = ptr.numel() - 1, val.numel()
    wsb = _sinkhorn_operands("sinkhorn_half", dev, val, [(ptr, n + 1), (perm, nnz), (idx, nnz)],
                             [(log_marg, n), (out, n), (other, other.numel())], workspace)
    launch("tsgu_sinkhorn_half", dev, vtype_of(val), itype_of(ptr), n, nnz, ptr, perm, idx, val, other, log_marg, out, workspace, wsb)


def sinkhorn_plan(ptr, idx, val, pot_group, pot_other, out=None):
    """out[k] = val[k] + pot_group[group of k] + pot_other[idx[k]] in stored order, rounded once to the values' dtype."""
    if out is None:
        out = torch.empty_like(val)
    dev = require_device(ptr, idx, val, pot_group, pot_other, out)
    n, nnz = ptr.numel() - 1, val.numel()
    _sinkhorn_operands("sinkhorn_plan", dev, val, [(ptr, n + 1), (idx, nnz)], [(pot_group, n), (pot_other, pot_other.numel())], None)
    if out.dtype != val.dtype or out.shape != val.shape or not out.is_contiguous():
        raise RuntimeError("sinkhorn_plan: the output must be a contiguous array of the values' dtype and shape")
    launch("tsgu_sinkhorn_plan", dev, vtype_of(val), itype_of(ptr), n, nnz, ptr, idx, val, pot_group, pot_other, out)
    return out


def sinkhorn_half_backward(ptr, perm, idx, grp, val, pot_group, pot_other, log_marg_other, g_other, grad, g_out, accumulate: bool,
                           workspace):
    """The adjoint of the other direction's half step, walked over the segments of `ptr`: term = g_other[idx]·exp(val + pot_group +
    pot_other[idx] − log_marg_other[idx]); grad[perm[k]] −= term; g_out[g] = (accumulate ? g_out[g] : 0) − Σ_group term."""
    dev = require_device(ptr, perm, idx, grp, val, pot_group, pot_other, log_marg_other, g_other, grad, g_out, workspace)
    n, nnz, m = ptr.numel() - 1, val.numel(), g_other.numel()
    wsb = _sinkhorn_operands("sinkhorn_half_backward", dev, val, [(ptr, n + 1), (perm, nnz), (idx, nnz), (grp, nnz)],
                             [(pot_group, n), (g_out, n), (pot_other, m), (log_marg_other, m), (g_other, m), (grad, nnz)], workspace)
    launch("tsgu_sinkhorn_half_backward", dev, vtype_of(val), itype_of(ptr), n, nnz, ptr, perm, idx, grp, val, pot_group, pot_other,
           log_marg_other, g_other, grad, g_out, int(bool(accumulate)), workspace, wsb)


def segment_sum(ptr, perm, val, add, out, workspace):
    """out[g] = add[g] + Σ_{k in group g} val[perm[k]] (add None: zeros); val is an accumulator array (float32 / float64)."""
    dev = require_device(ptr, perm, val, add, out, workspace)
    n, nnz = ptr.numel() - 1, val.numel()
    if val.dtype not in (torch.float32, torch.float64):
        raise RuntimeError(f"segment_sum: values must be float32 or float64, got {val.dtype}")
    wsb = _sinkhorn_operands("segment_sum", dev, val, [(ptr, n + 1), (perm, nnz)], [(add, n), (out, n)], workspace)
    launch("tsgu_segment_sum", dev, vtype_of(val), itype_of(ptr), n, nnz, ptr, perm, val, add, out, workspace, wsb)


def attention_supported(dtype: torch.dtype, heads: int, d: int) -> bool:
    """Do the attention kernels take `heads` heads of width `d` in value type `dtype`?  Host only (no GPU needed)."""
    vt = _VTYPE.get(dtype)
    return vt is not None and bool(load_library().tsgu_csr_attention_supported(vt, int(heads), int(d)))


def attention_geometry(dtype: torch.dtype, heads: int, d: int):
    """(entry lanes of a row's lane group, rows per workgroup, entries of one staged slice) of the attention kernels for
    (dtype, heads, d): the sizes at which their walk changes path.  Host only."""
    return _query("tsgu_csr_attention_geometry", _VTYPE[dtype], int(heads), int(d))


def _aligned_rows(t: torch.Tensor) -> torch.Tensor:
    """A 2-D operand as the attention kernels read it: unit column stride, base and row stride multiples of 16 bytes."""
    ok = t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and \
        (t.size(0) <= 1 or (t.stride(0) >= t.size(1) and (t.stride(0) * t.element_size()) % 16 == 0))
    return t if ok else t.clone(memory_format=torch.contiguous_format)


def _one_dtype(what: str, arrays, one_d: bool = True):
    """Operand check of a group of index arrays, or of value arrays: contiguous, of one dtype and (`one_d`) 1-D.  Returns the first."""
    first = arrays[0]
    for t in arrays:
        if (one_d and t.dim() != 1) or t.dtype != first.dtype or not t.is_contiguous():
            raise RuntimeError(f"the {what} must be contiguous{' 1-D' if one_d else ''} arrays of one dtype")
    return first


def _one_width(what: str, dense, row_major: bool = True):
    """Operand check of a group of dense operands: 2-D, of one dtype and width and (`row_major`) with unit column stride and rows
    that do not overlap.  Returns the first."""
    ref = dense[0]
    for t in dense:
        if t.dim() != 2 or t.dtype != ref.dtype or t.size(1) != ref.size(1) or (row_major and (
                (t.stride(1) != 1 and t.size(1) > 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)))):
            raise RuntimeError(f"the {what} must be 2-D{' row-major' if row_major else ''} arrays of one dtype and width")
    return ref


def _attention_walk(walk, bias, *dense):
    ptr, idx, perm = walk
    dev = require_device(ptr, idx, perm, bias, *dense)
    _one_dtype("index arrays of a walk", (ptr, idx) if perm is None else (ptr, idx, perm), one_d=False)
    if bias is not None and (bias.dtype != dense[0].dtype or not bias.is_contiguous() or bias.numel() != idx.numel()):
        raise RuntimeError("the bias must be a contiguous value array of the pattern in the operands' dtype")
    _one_width("dense operands [rows, heads*d] of an attention", dense, row_major=False)
    return dev


def _acc_dtype(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype == torch.float64 else torch.float32


def csr_attention(walk, bias, Q, K, V, heads: int, d: int, scale: float):
    """(O [n, heads·d], lse [n, heads] in the accumulator type) of attention over the pattern walked by rows as
    ``walk = (ptr, idx, perm or None)``; bias: the pattern's value array (at perm[k] for entry k) or None."""
    dev = _attention_walk(walk, bias, Q, K, V)
    ptr, idx, perm = walk
    Q, K, V = _aligned_rows(Q), _aligned_rows(K), _aligned_rows(V)
    n, m = Q.size(0), K.size(0)
    O = torch.empty((n, heads * d), dtype=Q.dtype, device=dev)
    lse = torch.empty((n, heads), dtype=_acc_dtype(Q.dtype), device=dev)
    launch("tsgu_csr_attention", dev, vtype_of(Q), itype_of(ptr), n, m, idx.numel(), ptr, idx, perm, bias, Q, _ld(Q), K, _ld(K),
           V, _ld(V), heads, d, float(scale), O, _ld(O), lse)
    return O, lse


def csr_attention_backward(walk, twalk, bias, Q, K, V, dO, lse, heads: int, d: int, scale: float, want_dA: bool):
    """(dQ, dK, dV, dA or None) from the forward's lse: the row pass over `walk`, then the column pass over the transposed walk
    `twalk` on the same stream.  dA is in the accumulator type, in the order of the pattern's value array."""
    dev = _attention_walk(walk, bias, Q, K, V, dO)
    _attention_walk(twalk, bias, Q, K, V, dO)
    ptr, idx, perm = walk
    tptr, tidx, tperm = twalk
    Q, K, V, dO = _aligned_rows(Q), _aligned_rows(K), _aligned_rows(V), _aligned_rows(dO)
    n, m, nnz = Q.size(0), K.size(0), idx.numel()
    acc = _acc_dtype(Q.dtype)
    if lse.dtype != acc or lse.shape != (n, heads) or not lse.is_contiguous():
        raise RuntimeError("lse must be the forward's [n, heads] array in the accumulator type")
    dQ, dK, dV = torch.empty_like(Q, memory_format=torch.contiguous_format), torch.empty((m, heads * d), dtype=Q.dtype, device=dev), \
        torch.empty((m, heads * d), dtype=Q.dtype, device=dev)
    delta = torch.empty((n, heads), dtype=acc, device=dev)
    dA = torch.empty((nnz,), dtype=acc, device=dev) if want_dA else None
    vt, it = vtype_of(Q), itype_of(ptr)
    launch("tsgu_csr_attention_backward_rows", dev, vt, it, n, m, nnz, ptr, idx, perm, bias, Q, _ld(Q), K, _ld(K), V, _ld(V),
           dO, _ld(dO), lse, heads, d, float(scale), dQ, _ld(dQ), delta, dA)
    launch("tsgu_csr_attention_backward_cols", dev, vt, it, n, m, nnz, tptr, tidx, tperm, bias, Q, _ld(Q), K, _ld(K), V,
           _ld(V), dO, _ld(dO), lse, delta, heads, d, float(scale), dK, _ld(dK), dV, _ld(dV))
    return dQ, dK, dV, dA


MM_REDUCE_OPS = {"amax": 0, "amin": 1}


def spmm_reduce_geometry(dtype: torch.dtype, p: int):
    """(rows per workgroup, entries of one staging pass, columns per grid.z slice) of the max / min product kernels for `p` columns
    of value type `dtype` with 16-byte aligned operands: the sizes at which their walk changes path.  Host only."""
    return _query("tsgu_csr_spmm_reduce_geometry", _VTYPE[dtype], int(p))


def _reduce_operands(index_arrays, val, *dense):
    dev = require_device(*index_arrays, val, *dense)
    _one_dtype("index arrays of a max / min product", index_arrays)
    ref = _one_width("dense operands of a max / min product", dense)
    if val is not None and (val.dtype != ref.dtype or val.dim() != 1 or not val.is_contiguous()):
        raise RuntimeError(f"expected A and B to have the same dtype, got {val.dtype} and {ref.dtype}")
    return dev


def csr_spmm_reduce(crow, col, val, B, n_rows: int, n_cols: int, reduce: str):
    """(C [n_rows, p], arg [n_rows, p] int32) of the max / min product of the 2-D CSR arrays with B [n_cols, p]: arg is the
    winning entry's position in `val` (−1 for a row without entries)."""
    dev = _reduce_operands((crow, col), val, B)
    p = B.size(1)
    if p < 1:
        raise RuntimeError("the max / min product needs at least one column")
    C = torch.empty((n_rows, p), dtype=B.dtype, device=dev)
    arg = torch.empty((n_rows, p), dtype=torch.int32, device=dev)
    launch("tsgu_csr_spmm_reduce", dev, vtype_of(B), itype_of(crow), n_rows, n_cols, col.numel(), crow, col, val, B, _ld(B), p,
           MM_REDUCE_OPS[reduce], C, p, arg, p)
    return C, arg


def csr_spmm_reduce_backward_values(crow, col, arg, G, B, n_rows: int, n_cols: int):
    """dval[e] = Σ_{k: arg[i,k] = e} G[i,k]·B[col[e],k], in the order of the value array."""
    dev = _reduce_operands((crow, col), None, G, B)
    dval = torch.empty((col.numel(),), dtype=B.dtype, device=dev)
    launch("tsgu_csr_spmm_reduce_backward_values", dev, vtype_of(B), itype_of(crow), n_rows, n_cols, col.numel(), crow, col, arg,
           _ld(arg), G, _ld(G), B, _ld(B), G.size(1), dval)
    return dval


def csr_spmm_reduce_backward_dense(tptr, tidx, perm, val, arg, G, n_rows: int, n_cols: int):
    """dB[j,k] = Σ_{e in column j: arg[i,k] = e} val[e]·G[i,k] over the transposed walk (tptr, tidx, perm into val)."""
    dev = _reduce_operands((tptr, tidx, perm), val, G)
    p = G.size(1)
    dB = torch.empty((n_cols, p), dtype=G.dtype, device=dev)
    launch("tsgu_csr_spmm_reduce_backward_dense", dev, vtype_of(G), itype_of(tptr), n_rows, n_cols, tidx.numel(), tptr, tidx, perm,
           val, arg, _ld(arg), G, _ld(G), p, dB, p)
    return dB


def bsr_mm_geometry(dtype: torch.dtype, bh: int, bw: int, p: int):
    """(rows of the result per workgroup, columns of the p per workgroup, summed elements per LDS stage) of the block-sparse product
    kernels for blocks of bh × bw elements of `dtype` against `p` dense columns: the sizes at which their walk changes path.  Host only."""
    return _query("tsgu_bsr_mm_geometry", _VTYPE[dtype], int(bh), int(bw), int(p))


def _bsr_operands(index_arrays, val, *dense):
    dev = require_device(*index_arrays, val, *dense)
    _one_dtype("index arrays of a block-sparse product", index_arrays)
    ref = _one_width("dense operands of a block-sparse product", dense)
    if ref.size(1) < 1:
        raise RuntimeError("the block-sparse product needs at least one column")
    if val is not None and (val.dtype != ref.dtype or val.dim() != 3 or not val.is_contiguous()):
        raise RuntimeError(f"the blocks must be a contiguous (nnzb, bh, bw) array of the dense operands' dtype {ref.dtype}, "
                           f"got {tuple(val.shape)} of {val.dtype}")
    return dev


def bsr_spmm(crow, col, val, B, n_block_rows: int, n_block_cols: int):
    """C [n_block_rows·bh, p] = A·B for the 2-D BSR arrays (crow, col, val [nnzb, bh, bw]) and B [n_block_cols·bw, p]."""
    dev = _bsr_operands((crow, col), val, B)
    nnzb, bh, bw = val.shape
    p = B.size(1)
    C = torch.empty((n_block_rows * bh, p), dtype=B.dtype, device=dev)
    if C.numel():
        launch("tsgu_bsr_spmm", dev, vtype_of(B), itype_of(crow), n_block_rows, n_block_cols, nnzb, bh, bw, crow, col, val, B, _ld(B),
               p, C, p)
    return C


def bsr_sddmm(crow, col, G, B, n_block_rows: int, n_block_cols: int, bh: int, bw: int):
    """dval [nnzb, bh, bw]: dval[e] = G[I_e·bh : +bh] · B[col[e]·bw : +bw]ᵀ, in the order of the value array."""
    dev = _bsr_operands((crow, col), None, G, B)
    nnzb = col.numel()
    dval = torch.empty((nnzb, bh, bw), dtype=B.dtype, device=dev)
    if nnzb:
        launch("tsgu_bsr_sddmm", dev, vtype_of(B), itype_of(crow), n_block_rows, n_block_cols, nnzb, bh, bw, crow, col, G, _ld(G), B,
               _ld(B), G.size(1), dval)
    return dval


def bsr_spmm_t(tptr, tidx, perm, val, G, n_block_rows: int, n_block_cols: int):
    """dB [n_block_cols·bw, p] = Aᵀ·G over the transposed block walk (tptr, tidx, perm into val [nnzb, bh, bw])."""
    dev = _bsr_operands((tptr, tidx, perm), val, G)
    nnzb, bh, bw = val.shape
    p = G.size(1)
    dB = torch.empty((n_block_cols * bw, p), dtype=G.dtype, device=dev)
    if dB.numel():
        launch("tsgu_bsr_spmm_t", dev, vtype_of(G), itype_of(tptr), n_block_rows, n_block_cols, nnzb, bh, bw, tptr, tidx, perm, val, G,
               _ld(G), p, dB, p)
    return dB


BSR_ATTENTION_LIMITS = "block sides that are multiples of 16, d in {16, 32, 64, 128} and H >= 1"


def bsr_attention_supported(dtype: torch.dtype, heads: int, d: int, bh: int, bw: int) -> bool:
    """Do the block-sparse attention kernels take `heads` heads of width `d` over blocks of bh × bw in value type `dtype`?  Host only."""
    vt = _VTYPE.get(dtype)
    return vt is not None and bool(load_library().tsgu_bsr_attention_supported(vt, int(heads), int(d), int(bh), int(bw)))


def bsr_attention_geometry(dtype: torch.dtype, heads: int, d: int, bh: int, bw: int):
    """(rows one workgroup owns, keys of one LDS stage) of the block-sparse attention kernels: the sizes at which their walk
    changes path.  Host only."""
    return _query("tsgu_bsr_attention_geometry", _VTYPE[dtype], int(heads), int(d), int(bh), int(bw))


def _bsr_attention_operands(index_arrays, bias, bh: int, bw: int, *dense):
    dev = require_device(*index_arrays, bias, *dense)
    _one_dtype("index arrays of a block-sparse attention", index_arrays)
    ref = _one_width("dense operands [rows, heads*d] of a block-sparse attention", dense, row_major=False)
    if bias is not None and (bias.dtype != ref.dtype or bias.dim() != 3 or tuple(bias.shape[1:]) != (bh, bw) or not bias.is_contiguous()):
        raise RuntimeError(f"the bias must be a contiguous (nnzb, {bh}, {bw}) array of the dense operands' dtype {ref.dtype}")
    return dev


def bsr_attention(crow, col, bias, bh: int, bw: int, Q, K, V, heads: int, d: int, scale: float, want_acc: bool = True):
    """(O [n, heads·d], lse [n, heads] in the accumulator type, O before its rounding — O itself unless bfloat16) of attention over
    the 2-D block pattern (crow, col) of bh × bw blocks; bias: the stored blocks [nnzb, bh, bw] or None.  want_acc=False (no backward
    will follow) spares bfloat16 the second accumulator; the third result is then O."""
    dev = _bsr_attention_operands((crow, col), bias, bh, bw, Q, K, V)
    Q, K, V = _aligned_rows(Q), _aligned_rows(K), _aligned_rows(V)
    nrb, ncb = crow.numel() - 1, K.size(0) // bw
    O = torch.empty((nrb * bh, heads * d), dtype=Q.dtype, device=dev)
    lse = torch.empty((nrb * bh, heads), dtype=_acc_dtype(Q.dtype), device=dev)
    Oacc = torch.empty((nrb * bh, heads * d), dtype=lse.dtype, device=dev) if want_acc and O.dtype != lse.dtype else None
    if O.numel():
        launch("tsgu_bsr_attention", dev, vtype_of(Q), itype_of(crow), nrb, ncb, col.numel(), bh, bw, crow, col, bias, Q, _ld(Q), K,
               _ld(K), V, _ld(V), heads, d, float(scale), O, _ld(O), lse, Oacc)
    return O, lse, (O if Oacc is None else Oacc)


def bsr_attention_backward(crow, col, twalk, bias, bh: int, bw: int, Q, K, V, dO, O, lse, heads: int, d: int, scale: float,
                           want_dA: bool):
    """(dQ, dK, dV, dA or None) from the forward's O (in the accumulator type: its third result) and lse: the row pass over (crow, col), then the column pass over the transposed
    block walk `twalk` = (tptr, tidx, perm) on the same stream.  dA is [nnzb, bh, bw] in the accumulator type."""
    tptr, tidx, perm = twalk
    dev = _bsr_attention_operands((crow, col, tptr, tidx, perm), bias, bh, bw, Q, K, V, dO)
    require_device(O)
    Q, K, V, dO, O = (_aligned_rows(x) for x in (Q, K, V, dO, O))
    nrb, ncb, nnzb = crow.numel() - 1, tptr.numel() - 1, col.numel()
    n, m = nrb * bh, ncb * bw
    acc = _acc_dtype(Q.dtype)
    if lse.dtype != acc or lse.shape != (n, heads) or not lse.is_contiguous():
        raise RuntimeError("lse must be the forward's [n, heads] array in the accumulator type")
    if O.dtype != acc or O.shape != (n, heads * d):
        raise RuntimeError("O must be the forward's [n, heads*d] result in the accumulator type")
    dQ = torch.empty((n, heads * d), dtype=Q.dtype, device=dev)
    dK = torch.empty((m, heads * d), dtype=Q.dtype, device=dev)
    dV = torch.empty((m, heads * d), dtype=Q.dtype, device=dev)
    delta = torch.empty((n, heads), dtype=acc, device=dev)
    dA = torch.empty((nnzb, bh, bw), dtype=acc, device=dev) if want_dA else None
    vt, it = vtype_of(Q), itype_of(crow)
    if n:
        launch("tsgu_bsr_attention_backward_rows", dev, vt, it, nrb, ncb, nnzb, bh, bw, crow, col, bias, Q, _ld(Q), K, _ld(K), V,
               _ld(V), dO, _ld(dO), O, _ld(O), lse, heads, d, float(scale), dQ, _ld(dQ), delta, dA)
    if m:
        launch("tsgu_bsr_attention_backward_cols", dev, vt, it, nrb, ncb, nnzb, bh, bw, tptr, tidx, perm, bias, Q, _ld(Q), K, _ld(K),
               V, _ld(V), dO, _ld(dO), lse, delta, heads, d, float(scale), dK, _ld(dK), dV, _ld(dV))
    return dQ, dK, dV, dA


# kSpgemmLimit / kSpgemmGroup of csrc/spgemm_impl.h (tsgu_spgemm_bins reports them): the sparse × sparse kernels bin the rows of C by
# a per-row measure x — the upper bound Σ_k nnz(B[k,:]) in the symbolic phase, the row's length in the numeric one.  Bin b holds
# SPGEMM_BIN_LIMITS[b-1] < x <= SPGEMM_BIN_LIMITS[b] and keeps a row in LDS with SPGEMM_BIN_LANES[b] lanes; rows above the last
# limit work in global memory, one workgroup each.
SPGEMM_BIN_LIMITS = (32, 512, 4096)
SPGEMM_BIN_LANES = (8, 64, 256, 256)
SPGEMM_SCRATCH_MIN = 8192        # smallest sort buffer of the global bin: the power of two above the last limit


def spgemm_bins():
    """(limits, lanes per row) as the library reports them.  Host only."""
    limits, lanes = (_int * 3)(), (_int * 4)()
    check(load_library().tsgu_spgemm_bins(limits, lanes), "tsgu_spgemm_bins")
    return tuple(limits), tuple(lanes)


def _spgemm_indices(*arrays):
    return itype_of(_one_dtype("index arrays of a sparse × sparse product", arrays))


def _spgemm_values(*arrays):
    return vtype_of(_one_dtype("value arrays of a sparse × sparse product", arrays))


def spgemm_row_bound(a_crow, a_col, b_crow, n_rows: int, n_inner: int):
    """ub[i] = Σ_{k ∈ A[i,:]} nnz(B[k,:]) as int64."""
    dev = require_device(a_crow, a_col, b_crow)
    it = _spgemm_indices(a_crow, a_col, b_crow)
    ub = torch.zeros(n_rows, dtype=torch.int64, device=dev)
    launch("tsgu_spgemm_row_bound", dev, it, n_rows, n_inner, a_crow, a_col, b_crow, ub)
    return ub


def spgemm_symbolic(bin: int, rows, dims, a_crow, a_col, b_crow, b_col, scratch=None, sptr=None, cnt=None, c_crow=None, c_col=None):
    """One bin of the symbolic phase over the int32 row list `rows`: counts into `cnt` (int64, per row), or — with `c_crow` and
    `c_col` — writes the rows' ascending columns.  `scratch` / `sptr`: the sort buffers of the global bin."""
    dev = require_device(rows, a_crow, a_col, b_crow, b_col, scratch, sptr, cnt, c_crow, c_col)
    fill = c_col is not None
    it = _spgemm_indices(a_crow, a_col, b_crow, b_col, *((c_crow, c_col) if fill else ()))
    if rows.dtype != torch.int32 or not rows.is_contiguous() or (cnt is not None and cnt.dtype != torch.int64):
        raise RuntimeError("sparse × sparse product: row lists are contiguous int32 arrays, counts int64")
    if bin == len(SPGEMM_BIN_LIMITS) and (scratch is None or scratch.dtype != torch.int32 or sptr is None or sptr.dtype != torch.int64
                                          or sptr.numel() != rows.numel() + 1):
        raise RuntimeError("sparse × sparse product: the global bin sorts int32 scratch slices addressed by an int64 pointer array")
    n, k, m = dims
    launch("tsgu_spgemm_symbolic", dev, it, bin, rows.numel(), rows, n, k, m, a_crow, a_col, b_crow, b_col, scratch, sptr,
           int(fill), cnt, c_crow, c_col)


def spgemm_numeric(bin: int, rows, dims, a_crow, a_col, a_val, b_crow, b_col, b_val, c_crow, c_col, c_val, acc=None):
    """One bin of the numeric phase over the int32 row list `rows`: the rows' values go to `c_val`."""
    dev = require_device(rows, a_crow, a_col, a_val, b_crow, b_col, b_val, c_crow, c_col, c_val, acc)
    it = _spgemm_indices(a_crow, a_col, b_crow, b_col, c_crow, c_col)
    vt = _spgemm_values(a_val, b_val, c_val)
    if rows.dtype != torch.int32 or not rows.is_contiguous():
        raise RuntimeError("sparse × sparse product: row lists are contiguous int32 arrays")
    if c_col.numel() != c_val.numel() or a_col.numel() != a_val.numel() or b_col.numel() != b_val.numel():
        raise RuntimeError("sparse × sparse product: one value per stored entry")
    if bin == len(SPGEMM_BIN_LIMITS) and (acc is None or acc.dtype != _acc_dtype(c_val.dtype) or acc.numel() < c_val.numel()):
        raise RuntimeError("sparse × sparse product: the global bin accumulates in nnz(C) entries of the accumulator type")
    n, k, m = dims
    launch("tsgu_spgemm_numeric", dev, vt, it, bin, rows.numel(), rows, n, k, m, a_crow, a_col, a_val, b_crow, b_col, b_val, c_crow,
           c_col, acc, c_val)


def spgemm_grad_a(dims, a_row, a_col, b_crow, b_col, b_val, c_crow, c_col, g):
    """gradA at A's stored positions: Σ_{t ∈ B[k,:]} g[pos_C(i, col_t)]·b_t, in B's stored order."""
    dev = require_device(a_row, a_col, b_crow, b_col, b_val, c_crow, c_col, g)
    it = _spgemm_indices(a_row, a_col, b_crow, b_col, c_crow, c_col)
    vt = _spgemm_values(b_val, g)
    if g.numel() != c_col.numel() or b_val.numel() != b_col.numel() or a_row.numel() != a_col.numel():
        raise RuntimeError("sparse × sparse product: one value per stored entry")
    out = torch.empty(a_col.numel(), dtype=b_val.dtype, device=dev)
    n, k, m = dims
    launch("tsgu_spgemm_grad_a", dev, vt, it, n, k, m, a_col.numel(), a_row, a_col, b_crow, b_col, b_val, c_crow, c_col, g, out)
    return out


def spgemm_grad_b(dims, b_row, b_col, t_crow, t_idx, t_perm, a_val, c_crow, c_col, g):
    """gradB at B's stored positions: Σ_{i ∈ column k of A} a_ik·g[pos_C(i, j)], in the order of A's transposed pattern."""
    dev = require_device(b_row, b_col, t_crow, t_idx, t_perm, a_val, c_crow, c_col, g)
    it = _spgemm_indices(b_row, b_col, t_crow, t_idx, t_perm, c_crow, c_col)
    vt = _spgemm_values(a_val, g)
    if g.numel() != c_col.numel() or a_val.numel() != t_idx.numel() or t_perm.numel() != t_idx.numel() or b_row.numel() != b_col.numel():
        raise RuntimeError("sparse × sparse product: one value per stored entry")
    out = torch.empty(b_col.numel(), dtype=a_val.dtype, device=dev)
    n, k, m = dims
    launch("tsgu_spgemm_grad_b", dev, vt, it, n, k, m, b_col.numel(), b_row, b_col, t_crow, t_idx, t_perm, a_val, c_crow, c_col, g, out)
    return out


SEGMENT_MM_TILE_ROWS = 128      # kImmBM of csrc/indexed_mm_impl.h: the row tile of the plans' tile prefix


def segment_mm_grad_b_workspace(dtype: torch.dtype, n: int, n_seg: int, d1: int, d2: int):
    """(chunk rows, launch bound on chunks, workspace bytes) of tsgu_segment_mm_grad_b: functions of the shapes only."""
    return _query("tsgu_segment_mm_grad_b_workspace", _VTYPE[dtype], n, n_seg, d1, d2)


def _imm_geometry(plan, *tensors) -> torch.device:
    lib = load_library()
    if lib.tsgu_segment_mm_tile_rows() != SEGMENT_MM_TILE_ROWS:
        raise HipExtensionMissing("libtsgu_hip.so was built with another segment_mm row tile; rebuild the extension")
    dev = require_device(plan.offsets, plan.perm, *tensors)
    if plan.perm is not None and plan.perm.dtype != plan.offsets.dtype:
        raise RuntimeError(f"index dtypes differ: {plan.offsets.dtype} and {plan.perm.dtype}")
    return dev


def segment_mm(plan, a, b, out):
    """out[perm[i]] = a[perm[i]] @ b[r] for the rows i of plan segment r (zeros outside the real segments).  `a` and `out` are
    row-major 2-D (n, d1) / (n, d2); `b` (R, d1, d2) with unit stride on one of its two last axes (a transposed view is read
    in place).  The plan: indexed_matmul._Plan."""
    dev = _imm_geometry(plan, a, b, out)
    n, d1 = a.shape
    d2 = out.size(1)
    if a.dtype != b.dtype or out.dtype != a.dtype:
        raise RuntimeError(f"segment_mm: dtypes differ: {a.dtype}, {b.dtype}, {out.dtype}")
    if a.stride(1) != 1 or out.stride(1) != 1 or b.dim() != 3 or b.size(1) != d1 or b.size(2) != d2:
        raise RuntimeError("segment_mm: operands of unexpected layout")
    launch("tsgu_segment_mm", dev, vtype_of(a), itype_of(plan.offsets), n, d1, d2, plan.n_seg, plan.offsets, plan.tile_ptr, plan.max_tiles,
           plan.perm, a, max(a.stride(0), d1), b, b.stride(0), b.stride(1), b.stride(2), out, max(out.stride(0), d2))
    return out


def segment_mm_grad_b(plan, a, g, grad_b):
    """grad_b[r] = Σ over the rows i of plan segment r of a[perm[i]]ᵀ g[perm[i]]; `grad_b` (R, d1, d2) contiguous."""
    dev = _imm_geometry(plan, a, g, grad_b)
    n, d1 = a.shape
    d2 = g.size(1)
    if a.dtype != g.dtype or grad_b.dtype != a.dtype:
        raise RuntimeError(f"segment_mm_grad_b: dtypes differ: {a.dtype}, {g.dtype}, {grad_b.dtype}")
    if a.stride(1) != 1 or g.stride(1) != 1 or not grad_b.is_contiguous():
        raise RuntimeError("segment_mm_grad_b: operands of unexpected layout")
    chunk, max_chunks, nbytes = segment_mm_grad_b_workspace(a.dtype, n, plan.n_seg, d1, d2)
    chunk_ptr, part_ptr = plan.chunks(chunk)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    launch("tsgu_segment_mm_grad_b", dev, vtype_of(a), itype_of(plan.offsets), n, d1, d2, plan.n_seg, plan.offsets, chunk_ptr, part_ptr, chunk,
           max_chunks, plan.perm, a, max(a.stride(0), d1), g, max(g.stride(0), d2), grad_b, ws, nbytes)
    return grad_b


def csr_sptrsm(ptr, idx, val, B, n: int, lower: bool, unit: bool, perm=None, wg_per_cu: int = 1):
    """X = M^{-1} B for the row-gather structure (ptr, idx, [perm], val) of a triangular M.  `wg_per_cu`: persistent workgroups per
    compute unit (1 … 8; speed only, see include/tsgu_hip.h)."""
    lib = load_library()
    dev = require_device(ptr, idx, val, B, perm)
    if val.dtype != B.dtype:
        raise RuntimeError(f"expected A and B to have the same dtype, got {val.dtype} and {B.dtype}")
    if B.dim() != 2 or B.size(0) != n or ptr.numel() != n + 1:
        raise RuntimeError(f"tsgu_csr_sptrsm: a system of {n} rows needs a right-hand side of {n} rows and a row pointer of {n + 1} "
                           f"words, got {tuple(B.shape)} and {ptr.numel()}")
    B, ldb, b_cs = strided2d(B)
    p = B.size(-1)
    ptr, idx, val = ptr.contiguous(), idx.contiguous(), val.contiguous()
    if perm is not None:
        perm = perm.contiguous()
    X = torch.empty((n, p), dtype=B.dtype, device=dev)
    if n == 0 or p == 0:
        return X  # nothing to solve (the kernel would not even initialise its error word)
    work = torch.empty((lib.tsgu_sptrsm_work_bytes(n, p),), dtype=torch.uint8, device=dev)
    launch("tsgu_csr_sptrsm", dev, vtype_of(val), itype_of(ptr), n, idx.numel(), ptr, idx, perm, val, int(bool(lower)), int(bool(unit)), B, ldb,
           b_cs, X, _ld(X), p, work, int(wg_per_cu))
    # error word sits behind the 64 ticket counters (struct TrsmWork in csrc/sptrsm.hip).  It is only ever set by the
    # 4 s device-side wait bound (a dependency that never arrives).  Default: read back before X is handed out (one host
    # sync per solve); TSGU_SPTRSM_CHECK=lazy — and any solve inside a stream capture, where a host read is not allowed —
    # copies it asynchronously to pinned memory and examines it at the next solve / `poll_errors()`.
    _defer_error_check(work[512:516].view(torch.int32), dev)
    return X


def csr_sptrsm_lattice(tables, val, B, n: int, lower: bool, unit: bool, workgroups: int = 0):
    """X = M^{-1} B by the line sweep (csrc/sptrsm_lattice.hip) for the lattice factor described by `tables`
    (_lattice.trsm_tables of M's lattice plan for this sweep direction).  `workgroups`: persistent workgroups (0: the kernel's
    rule; speed only).  Allocation, error word and capture behaviour as `csr_sptrsm`."""
    lib = load_library()
    dev = require_device(tables.tab, val, B)
    if val.dtype != B.dtype:
        raise RuntimeError(f"expected A and B to have the same dtype, got {val.dtype} and {B.dtype}")
    if B.dim() != 2 or B.size(0) != n or tables.struct.nlines * tables.struct.nz != n or bool(tables.lower) != bool(lower):
        raise RuntimeError(f"tsgu_csr_sptrsm_lattice: a {'lower' if lower else 'upper'} sweep over {n} rows needs a right-hand side of "
                           f"{n} rows and the tables of that sweep, got {tuple(B.shape)} and tables of "
                           f"{tables.struct.nlines * tables.struct.nz} rows ({'lower' if tables.lower else 'upper'})")
    B, ldb, b_cs = strided2d(B)
    p = B.size(-1)
    val = val.contiguous()
    X = torch.empty((n, p), dtype=B.dtype, device=dev)
    if n == 0 or p == 0:
        return X
    work = torch.empty((lib.tsgu_sptrsm_work_bytes(n, p),), dtype=torch.uint8, device=dev)
    launch("tsgu_csr_sptrsm_lattice", dev, vtype_of(val), tables.struct_addr, val.numel(), val, int(bool(lower)), int(bool(unit)), B, ldb, b_cs,
           X, _ld(X), p, work, int(workgroups))
    _defer_error_check(work[512:516].view(torch.int32), dev, "tsgu_csr_sptrsm_lattice (dependency wait)")
    return X


FACTOR_DTYPES = (torch.float32, torch.float64)


def factor_geometry(dtype: torch.dtype):
    """(row_capacity, waves_per_block) of the incomplete factorisations for `dtype`: the entries of a row that are staged in LDS (a
    longer row is built in the output array itself) and the rows a workgroup has in flight."""
    return _query("tsgu_csr_factor_geometry", _VTYPE[dtype])


def csr_factor(kind: str, ptr, idx, diag_pos, val, n: int, shift: float = 0.0, wg_per_cu: int = 1, out=None):
    """The zero-fill incomplete factor of the CSR matrix (ptr, idx, val) on its own pattern (include/tsgu_hip_factor.h): `kind`
    "ilu0" (combined L \\ U array) or "ic0" (the arrays are those of tril(A)).  Columns ascending and unique per row, every diagonal
    stored, `diag_pos` its position per row — the caller's plan has checked that.  Returns (out, info): `info` a device int64, 0 or
    1 + the lowest row that broke down; nothing is read back here but the error word of the bounded waits, by the protocol of
    `csr_sptrsm`.  `out` may be `val` itself."""
    if kind not in ("ilu0", "ic0"):
        raise ValueError(f"csr_factor: unknown factorisation {kind!r}")
    if val.dtype not in FACTOR_DTYPES:
        raise TypeError(f"tsgu_csr_{kind}: float32 and float64 values only, got {val.dtype}")
    lib = load_library()
    dev = require_device(ptr, idx, diag_pos, val, out)
    if ptr.numel() != n + 1 or diag_pos.numel() != n or idx.numel() != val.numel() or not (ptr.dtype == idx.dtype == diag_pos.dtype):
        raise RuntimeError(f"tsgu_csr_{kind}: {n} rows need a row pointer of {n + 1} words, {n} diagonal positions and as many values as "
                           f"columns, all index arrays of one dtype; got {ptr.numel()}, {diag_pos.numel()}, {val.numel()} / {idx.numel()}")
    ptr, idx, diag_pos, val = ptr.contiguous(), idx.contiguous(), diag_pos.contiguous(), val.contiguous()
    if out is None:
        out = torch.empty_like(val)
    elif out.dtype != val.dtype or out.shape != val.shape or not out.is_contiguous():
        raise RuntimeError(f"tsgu_csr_{kind}: `out` must be a contiguous array like the values")
    info = torch.zeros((), dtype=torch.int64, device=dev)
    if n == 0:
        return out, info
    work = torch.empty((lib.tsgu_csr_factor_work_bytes(n),), dtype=torch.uint8, device=dev)
    launch(f"tsgu_csr_{kind}", dev, vtype_of(val), itype_of(ptr), n, idx.numel(), ptr, idx, diag_pos, val, float(shift), out, work, info,
           int(wg_per_cu))
    _defer_error_check(work[0:4].view(torch.int32), dev, f"tsgu_csr_{kind} (dependency wait)")
    return out, info


def fsai_geometry(dtype: torch.dtype):
    """(row_capacity, rows_per_block) of the FSAI build for `dtype`: the longest row of the pattern S (the largest local system)
    the kernel accepts, and the rows a workgroup takes at a time."""
    return _query("tsgu_csr_fsai_geometry", _VTYPE[dtype])


def csr_fsai(a_ptr, a_idx, a_val, s_ptr, s_idx, n: int, order=None, wg_per_cu: int = 8):
    """The values of the FSAI factor G on the lower pattern (s_ptr, s_idx) for the CSR (a_ptr, a_idx, a_val) of tril(A)
    (include/tsgu_hip_fsai.h).  Both patterns: columns ascending and unique per row, the diagonal last — the caller's plan has
    checked that, and that no row of S exceeds `fsai_geometry`'s capacity.  `order`: the rows in the order the waves take them
    (speed only).  Returns (out, info): `info` a device int64, 0 or 1 + the lowest row whose local matrix was not positive
    definite.  Nothing in the kernel waits, so there is no work buffer and nothing is read back here."""
    if a_val.dtype not in FACTOR_DTYPES:
        raise TypeError(f"tsgu_csr_fsai: float32 and float64 values only, got {a_val.dtype}")
    dev = require_device(a_ptr, a_idx, a_val, s_ptr, s_idx, order)
    index = [t for t in (a_ptr, a_idx, s_ptr, s_idx, order) if t is not None]
    if (a_ptr.numel() != n + 1 or s_ptr.numel() != n + 1 or a_idx.numel() != a_val.numel() or (order is not None and order.numel() != n)
            or any(t.dtype != a_ptr.dtype for t in index)):
        raise RuntimeError(f"tsgu_csr_fsai: {n} rows need two row pointers of {n + 1} words, as many values as columns of A, an "
                           f"`order` of {n} rows, and all index arrays of one dtype; got {a_ptr.numel()}, {s_ptr.numel()}, "
                           f"{a_val.numel()} / {a_idx.numel()}" + ("" if order is None else f", {order.numel()}"))
    a_ptr, a_idx, a_val, s_ptr, s_idx = (t.contiguous() for t in (a_ptr, a_idx, a_val, s_ptr, s_idx))
    order = None if order is None else order.contiguous()
    out = torch.empty(s_idx.numel(), dtype=a_val.dtype, device=dev)
    info = torch.zeros((), dtype=torch.int64, device=dev)
    if n == 0:
        return out, info
    launch("tsgu_csr_fsai", dev, vtype_of(a_val), itype_of(a_ptr), n, a_ptr, a_idx, a_val, s_ptr, s_idx, s_idx.numel(), order, out, info,
           int(wg_per_cu))
    return out, info


def tall_geometry(dtype: torch.dtype, n: int = 0, a: int = 0, b: int = 0):
    """(kmax, wmax, rows_per_workgroup, workspace_bytes) of the tall-skinny kernels (csrc/tsgu_hip_lobpcg.h): the widest block, the
    widest operand of the Gram kernel, the rows of a chunk, and the bytes `tall_gram` needs for `n` rows and an `a` x `b` result
    (`lobpcg_residual`: a = k, b = 1)."""
    return _query("tsgu_tall_geometry", _VTYPE[dtype], int(n), int(a), int(b))


def _tall_views(what: str, views):
    """Operand check of the dense views of a tall-skinny call: 2-D, one dtype and height, unit column stride, rows that do not overlap."""
    ref = views[0]
    if ref.dtype not in FACTOR_DTYPES:
        raise TypeError(f"{what}: float32 and float64 operands only, got {ref.dtype}")
    for t in views:
        if t.dim() != 2 or t.dtype != ref.dtype or t.size(0) != ref.size(0) or (t.stride(1) != 1 and t.size(1) > 1) or \
                (t.size(0) > 1 and t.stride(0) < t.size(1)):
            raise RuntimeError(f"the {what} must be 2-D row-major views of one dtype and height")
    return ref


def _tall_workspace(ref: torch.Tensor, a: int, b: int, workspace=None) -> torch.Tensor:
    need = tall_geometry(ref.dtype, ref.size(0), a, b)[3]
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(max(need // ref.element_size(), 1), dtype=ref.dtype, device=ref.device)
    return workspace


def tall_gram(Y, Z, out=None, workspace=None, workgroups: int = 0):
    """YᵀZ (a, b) for the row-major views Y (n, a) and Z (n, b), a, b <= wmax; `Y is Z` is read once.  Deterministic: the same bits
    for every `workgroups` (0: the library's choice).  `workspace`: scratch of `tall_geometry(...)[3]` bytes, allocated when missing."""
    ref = _tall_views("operands of tall_gram", (Y, Z))
    dev = require_device(Y, Z, out, workspace)
    a, b = Y.size(1), Z.size(1)
    if out is None:
        out = torch.empty((a, b), dtype=ref.dtype, device=dev)
    elif out.shape != (a, b) or out.dtype != ref.dtype or (b > 1 and out.stride(1) != 1):
        raise RuntimeError(f"tall_gram: out must be a row-major ({a}, {b}) array of {ref.dtype}")
    workspace = _tall_workspace(ref, a, b, workspace)
    launch("tsgu_tall_gram", dev, vtype_of(ref), ref.size(0), a, b, Y, _ld(Y), Z, _ld(Z), out, _ld(out), workspace,
           workspace.numel() * workspace.element_size(), int(workgroups))
    return out


def tall_combine(inputs, outputs, coefs, betas=None, workgroups: int = 0):
    """outputs[t] = betas[t]·outputs[t] + Σ_i inputs[i] @ coefs[t][i] in one pass over the rows: up to six (n, <= kmax) input views,
    up to four output views, `coefs[t][i]` a (width of input i, width of output t) matrix or None (the block does not
    contribute).  No output may share an element with an input or another output (views that interleave in one allocation do
    not); the library refuses anything else.  Returns `outputs`."""
    ref = _tall_views("operands of tall_combine", (*inputs, *outputs))
    dev = require_device(*inputs, *outputs, *(c for row in coefs for c in row))
    n_in, n_out = len(inputs), len(outputs)
    if len(coefs) != n_out or any(len(row) != n_in for row in coefs):
        raise RuntimeError(f"tall_combine: {n_out} outputs and {n_in} inputs need {n_out} rows of {n_in} coefficient matrices")
    flat = []
    for t, row in enumerate(coefs):
        for i, c in enumerate(row):
            if c is not None and (c.dtype != ref.dtype or tuple(c.shape) != (inputs[i].size(1), outputs[t].size(1))):
                raise RuntimeError(f"tall_combine: coefficient ({t}, {i}) must be a ({inputs[i].size(1)}, {outputs[t].size(1)}) "
                                   f"matrix of {ref.dtype}")
            if c is not None and ((c.size(1) > 1 and c.stride(1) != 1) or (c.size(0) > 1 and c.stride(0) < c.size(1))):
                c = c.contiguous()           # (a column-major result of torch.linalg: the kernel reads row-major matrices)
            flat.append(c)
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[_p(t) for t in ts])      # noqa: E731
    ints = lambda xs: (ctypes.c_int64 * len(xs))(*xs)                         # noqa: E731
    host = [ptrs(inputs), ints([t.size(1) for t in inputs]), ints([_ld(t) for t in inputs]),
            ptrs(outputs), ints([t.size(1) for t in outputs]), ints([_ld(t) for t in outputs]),
            (ctypes.c_double * n_out)(*([0.0] * n_out if betas is None else [float(x) for x in betas])),
            ptrs(flat), ints([0 if c is None else _ld(c) for c in flat])]
    addr = [ctypes.addressof(h) for h in host]
    launch("tsgu_tall_combine", dev, vtype_of(ref), ref.size(0), n_in, addr[0], addr[1], addr[2], n_out, addr[3], addr[4], addr[5],
           addr[6], addr[7], addr[8], int(workgroups))
    return outputs


def lobpcg_residual(AX, X, lam, out=None, workspace=None, workgroups: int = 0):
    """(R, sumsq): R = AX − X·diag(lam) for (n, k <= kmax) views and a device vector `lam` (k,), and the column sums of squares of R
    (k,) — deterministic, as `tall_gram`.  `out` receives R (it may share no element with AX or X)."""
    ref = _tall_views("operands of lobpcg_residual", (AX, X) if out is None else (AX, X, out))
    dev = require_device(AX, X, lam, out, workspace)
    k = AX.size(1)
    if X.size(1) != k or lam.shape != (k,) or lam.dtype != ref.dtype or not lam.is_contiguous() or (out is not None and out.size(1) != k):
        raise RuntimeError(f"lobpcg_residual: AX, X and R must be (n, {k}) views and lam a contiguous ({k},) vector of {ref.dtype}")
    if out is None:
        out = torch.empty((ref.size(0), k), dtype=ref.dtype, device=dev)
    sumsq = torch.empty(k, dtype=ref.dtype, device=dev)
    workspace = _tall_workspace(ref, k, 1, workspace)
    launch("tsgu_lobpcg_residual", dev, vtype_of(ref), ref.size(0), k, AX, _ld(AX), X, _ld(X), lam, out, _ld(out), sumsq, workspace,
           workspace.numel() * workspace.element_size(), int(workgroups))
    return out, sumsq


def amg_geometry():
    """(group widths the hop accepts — the powers of two between the library's limits —, column tile of the affine product)
    (csrc/tsgu_hip_amg.h).  Host only."""
    lo, hi, tile = _query("tsgu_amg_geometry")
    widths = []
    while lo <= hi:
        widths.append(lo)
        lo *= 2
    return tuple(widths), tile


def _amg_keys(what: str, n: int, *keys):
    for k in keys:
        if k is not None and (k.dtype != torch.int64 or k.shape != (n,) or not k.is_contiguous()):
            raise RuntimeError(f"{what}: keys are contiguous int64 vectors of {n} words (the bits of unsigned 64-bit keys)")


def amg_hop(ptr, idx, keys, n: int, group: int = 8, out=None):
    """out[i] = max(keys[i], max of keys[j] over the stored entries (i, j)) in UNSIGNED 64-bit order, on the CSR pattern (ptr, idx).
    Keys travel as int64 tensors holding the bits.  `group`: lanes per row, one of `amg_geometry()[0]` (speed only: the result
    does not depend on it).  `out` may not overlap `keys`."""
    dev = require_device(ptr, idx, keys, out)
    if ptr.numel() != n + 1 or ptr.dtype != idx.dtype:
        raise RuntimeError(f"tsgu_csr_amg_hop: {n} rows need a row pointer of {n + 1} words of the columns' dtype, got {ptr.numel()} "
                           f"({ptr.dtype} / {idx.dtype})")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    _amg_keys("tsgu_csr_amg_hop", n, keys, out)
    ptr, idx = ptr.contiguous(), idx.contiguous()
    launch("tsgu_csr_amg_hop", dev, itype_of(ptr), n, idx.numel(), ptr, idx if idx.numel() else None, keys, out, int(group))
    return out


AMG_INIT, AMG_ROUND, AMG_ROOTS = 0, 1, 2


def amg_mis2_update(mode: int, n: int, key=None, t=None, out=None, undecided=None, device=None):
    """One node-wise step of the MIS-2 aggregation (csrc/tsgu_hip_amg.h): AMG_INIT writes the initial keys, AMG_ROUND applies the
    state machine to (key, t = hop(hop(key))) and sets the device word `undecided` (zeroed by the caller) when a node stays
    undecided, AMG_ROOTS keeps the roots' keys and zeroes the rest.  Returns `out` (AMG_ROUND may write `key` in place)."""
    dev = require_device(key, t, out, undecided) or device
    if dev is None:
        raise RuntimeError("tsgu_amg_mis2_update: a device is required when no tensor names one")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=dev)
    _amg_keys("tsgu_amg_mis2_update", n, key, t, out)
    if undecided is not None and (undecided.dtype != torch.int64 or undecided.numel() != 1):
        raise RuntimeError("tsgu_amg_mis2_update: `undecided` is one int64 word")
    launch("tsgu_amg_mis2_update", dev, int(mode), n, key, t, out, undecided)
    return out


def csr_affine_spmm(ptr, idx, val, X, n_rows: int, n_cols: int, C=None, B=None, w=None, alpha: float = 1.0, out=None):
    """out = C + alpha·w∘(B − A·X) for the CSR matrix (ptr, idx, val) of shape (n_rows, n_cols) and row-major X (n_cols, p); C, B
    (n_rows, p) and w (n_rows,) are optional (None: 0, 0 and 1).  One launch (csrc/tsgu_hip_amg.h).  `out` may be C or B; it may
    not overlap X (the library refuses it).  float32 and float64."""
    if val.dtype not in FACTOR_DTYPES:
        raise TypeError(f"tsgu_csr_affine_spmm: float32 and float64 values only, got {val.dtype}")
    dev = require_device(ptr, idx, val, X, C, B, w, out)
    p = X.size(1) if X.dim() == 2 else -1
    dense = [t for t in (X, C, B, out) if t is not None]
    if (ptr.numel() != n_rows + 1 or ptr.dtype != idx.dtype or idx.numel() != val.numel() or X.dim() != 2 or X.size(0) != n_cols
            or any(t.dtype != val.dtype for t in dense) or (w is not None and (w.dtype != val.dtype or w.shape != (n_rows,)))
            or any(t.dim() != 2 or t.shape != (n_rows, p) for t in (C, B, out) if t is not None)
            or any((t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1)) for t in dense)):
        raise RuntimeError(f"tsgu_csr_affine_spmm: a ({n_rows}, {n_cols}) matrix needs a row pointer of {n_rows + 1} words of the "
                           f"columns' dtype, as many values as columns, a row-major X ({n_cols}, p) and row-major C, B, out "
                           f"({n_rows}, p) of the values' dtype, and w ({n_rows},)")
    if out is None:
        out = torch.empty((n_rows, p), dtype=val.dtype, device=dev)
    ptr, idx, val = ptr.contiguous(), idx.contiguous(), val.contiguous()
    w = None if w is None else w.contiguous()
    nnz = idx.numel()
    launch("tsgu_csr_affine_spmm", dev, vtype_of(val), itype_of(ptr), n_rows, n_cols, nnz, p, ptr, idx if nnz else None,
           val if nnz else None, X if X.numel() else None, _ld(X), C, 0 if C is None else _ld(C), B, 0 if B is None else _ld(B), w,
           float(alpha), out if out.numel() else None, _ld(out))
    return out


def color_geometry():
    """(group widths of the colouring round and check, colours per window, group widths of the sweep, column tile of the sweep)
    (csrc/tsgu_hip_color.h).  Host only."""
    lo, hi, window, slo, shi, tile = _query("tsgu_color_geometry")
    pows = lambda a, b: tuple(a << k for k in range(8) if (a << k) <= b)      # noqa: E731
    return pows(lo, hi), window, pows(slo, shi), tile


def _color_pattern(what: str, ptr, idx, tptr, tidx, n: int):
    """The contiguous index arrays of a colouring call and the size of the transposed list."""
    if ptr.numel() != n + 1 or ptr.dtype != idx.dtype or (tptr is None) != (tidx is None) or \
            (tptr is not None and (tptr.numel() != n + 1 or tptr.dtype != ptr.dtype or tidx.dtype != ptr.dtype)):
        raise RuntimeError(f"{what}: {n} rows need row pointers of {n + 1} words, all index arrays of one dtype")
    ptr, idx = ptr.contiguous(), idx.contiguous()
    if tptr is not None:
        tptr, tidx = tptr.contiguous(), tidx.contiguous()
    return ptr, idx, tptr, tidx, 0 if tidx is None else tidx.numel()


def _color_vector(what: str, n: int, *vectors):
    for c in vectors:
        if c is not None and (c.dtype != torch.int32 or c.shape != (n,) or not c.is_contiguous()):
            raise RuntimeError(f"{what}: colours are contiguous int32 vectors of {n} words")


def csr_color_round(ptr, idx, tptr, tidx, colors, n: int, out, undecided, group: int = 8):
    """One round of the greedy multicolouring on the pattern (ptr, idx) and its transpose (tptr, tidx; None when the pattern is
    structurally symmetric) (csrc/tsgu_hip_color.h): `out` receives the colours after the round, `undecided` (an int64 word the
    caller zeroed) becomes non-zero when a node stays uncoloured.  `group`: lanes per node, one of `color_geometry()[0]`."""
    dev = require_device(ptr, idx, tptr, tidx, colors, out, undecided)
    ptr, idx, tptr, tidx, nnz_t = _color_pattern("tsgu_csr_color_round", ptr, idx, tptr, tidx, n)
    _color_vector("tsgu_csr_color_round", n, colors, out)
    if undecided.dtype != torch.int64 or undecided.numel() != 1:
        raise RuntimeError("tsgu_csr_color_round: `undecided` is one int64 word")
    nnz = idx.numel()
    launch("tsgu_csr_color_round", dev, itype_of(ptr), n, nnz, ptr, idx if nnz else None, nnz_t, tptr, tidx if nnz_t else None,
           colors, out, undecided, int(group))
    return out


def csr_color_check(ptr, idx, tptr, tidx, colors, n: int, n_colors: int, group: int = 8):
    """A device int64: 0 when `colors` is a colouring of the pattern with `n_colors` colours, else 1 + the lowest row whose colour
    is outside [0, n_colors) or held by a neighbour (csrc/tsgu_hip_color.h).  Nothing is read back here."""
    dev = require_device(ptr, idx, tptr, tidx, colors)
    ptr, idx, tptr, tidx, nnz_t = _color_pattern("tsgu_csr_color_check", ptr, idx, tptr, tidx, n)
    _color_vector("tsgu_csr_color_check", n, colors)
    first = torch.zeros((), dtype=torch.int64, device=dev)
    nnz = idx.numel()
    launch("tsgu_csr_color_check", dev, itype_of(ptr), n, nnz, ptr, idx if nnz else None, nnz_t, tptr, tidx if nnz_t else None,
           colors if n else None, int(n_colors), first, int(group))
    return first


SWEEP_DIVIDE, SWEEP_UNIT, SWEEP_SCALED = 0, 1, 2


def csr_color_sweeps(mode: int, begin, end, idx, diag, val, B, X, classes, vmap=None, bmap=None, out=None, out_rows=None, group: int = 8):
    """One triangular sweep by colour classes, in place in the workspace X (n, p): one launch of `tsgu_csr_color_sweep`
    (csrc/tsgu_hip_color.h) per (row0, row1) of `classes`, in their order.  For the rows of a class,
    x[i] = (B[bmap(i)] − Σ_{e in [begin[i], end[i])} val[vmap(e)]·x[idx[e]]) / val[vmap(diag[i])] (SWEEP_DIVIDE), without the division
    (SWEEP_UNIT, diag None) or with the sum alone divided (SWEEP_SCALED); `out`, when given, also receives x[i] in row out_rows(i).
    The operands are checked once for all classes and nothing is copied: they are contiguous in the way the plan made them."""
    n, p = X.shape
    idt = begin.dtype
    if (begin.numel() != n or end.numel() != n or B.dim() != 2 or B.size(0) != n or B.size(1) != p or B.dtype != val.dtype
            or X.dtype != val.dtype or idx.dtype != idt or end.dtype != idt
            or any(t is not None and (t.numel() != n or t.dtype != idt) for t in (diag, bmap, out_rows))
            or (vmap is not None and (vmap.numel() != idx.numel() or vmap.dtype != idt))
            or (out is not None and (out.shape != X.shape or out.dtype != val.dtype))
            or any(t is not None and not (t.is_cuda and t.device == X.device)
                   for t in (begin, end, idx, diag, val, B, X, vmap, bmap, out, out_rows))
            or any(t is not None and not t.is_contiguous() for t in (begin, end, idx, diag, val, vmap, bmap, out_rows))
            or any(t is not None and ((t.size(1) > 1 and t.stride(1) != 1) or (t.size(0) > 1 and t.stride(0) < t.size(1))) for t in (B, X, out))):
        raise RuntimeError(f"tsgu_csr_color_sweep: {n} rows need contiguous begin, end, diag, bmap and out_rows of {n} words and a vmap of "
                           "as many words as columns, all of one index dtype, and row-major B, X and out of (n, p) elements of the "
                           "values' dtype, all on one GPU")
    dev = X.device
    fn = getattr(_lib or load_library(), "tsgu_csr_color_sweep")
    head = (_VTYPE.get(val.dtype, -1), itype_of(begin), int(mode), n, idx.numel(), val.numel())
    tail = (p, begin.data_ptr(), end.data_ptr(), idx.data_ptr() if idx.numel() else None, _p(diag), _p(vmap),
            val.data_ptr() if val.numel() else None, B.data_ptr(), _ld(B), _p(bmap), X.data_ptr(), _ld(X), _p(out),
            0 if out is None else _ld(out), _p(out_rows), int(group), dev.index)

    def run():
        stream = _raw_stream(dev)          # (read at call time: the same code runs eagerly and under graph capture)
        for row0, row1 in classes:
            rc = fn(*head, int(row0), int(row1), *tail, stream)
            if rc:
                check(rc, "tsgu_csr_color_sweep")

    if torch.cuda.current_device() == dev.index:
        run()
    else:
        with torch.cuda.device(dev):
            run()
    return X


def csr_color_sweep(mode: int, begin, end, idx, diag, val, B, X, row0: int, row1: int, vmap=None, bmap=None, out=None, out_rows=None,
                    group: int = 8):
    """The rows [row0, row1) of ONE colour class: `csr_color_sweeps` with a single class."""
    return csr_color_sweeps(mode, begin, end, idx, diag, val, B, X, ((row0, row1),), vmap=vmap, bmap=bmap, out=out, out_rows=out_rows,
                            group=group)


_PENDING = []            # (event or None, pinned / host int32 slot, what, tsgu status)
_PENDING_LOCK = threading.Lock()
# Default: the error word of a solve is read back before X is handed out (one host sync per solve; a C3-sized solve takes
# milliseconds).  TSGU_SPTRSM_CHECK=lazy defers the check (X is then UNVERIFIED until `poll_errors()` — exported by the
# package — has looked at it: the next solve, wait_for_plans() and interpreter exit call it).
_SYNC_CHECK = os.environ.get("TSGU_SPTRSM_CHECK", "sync") != "lazy"


def _defer_error_check(word: torch.Tensor, dev: torch.device, what: str = "tsgu_csr_sptrsm (dependency wait)",
                       status: int = -7) -> None:
    """Report a non-zero int32 error `word` as tsgu `status`: at once by default, at the next `poll_errors()` when lazy.  A word
    on the CPU (operands of the torch-op path) is already complete."""
    if not word.is_cuda:
        if _SYNC_CHECK:
            if int(word.item()) != 0:
                check(status, what)
            return
        with _PENDING_LOCK:
            _PENDING.append((None, word.reshape(1).to(torch.int32), what, status))
        return
    capturing = torch.cuda.is_current_stream_capturing()
    if _SYNC_CHECK and not capturing:
        if int(word.item()) != 0:
            check(status, what)
        return
    if capturing:
        return      # (a graph replay cannot report through the host; the 4 s device-side bound still ends the wait)
    poll_errors()
    host = torch.empty(1, dtype=torch.int32, pin_memory=True)
    host.copy_(word, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    with _PENDING_LOCK:
        _PENDING.append((ev, host, what, status))


def _poll_at_exit() -> None:
    try:
        poll_errors(block=True)
    except Exception as exc:  # noqa: BLE001
        import sys

        print(f"torchsparsegradutils_amd: {exc}", file=sys.stderr)


if not _SYNC_CHECK:
    import atexit

    atexit.register(_poll_at_exit)


def poll_errors(block: bool = False) -> None:
    """Raise if a device-side error word of an earlier launch is set.  Non-blocking by default (only completed
    launches are examined); ``block=True`` waits for all of them (tests, end of a run)."""
    with _PENDING_LOCK:
        items = list(_PENDING)
        _PENDING.clear()
    keep, failed = [], None
    for ev, host, what, status in items:
        if block and ev is not None:
            ev.synchronize()
        if ev is None or ev.query():
            if int(host.item()) != 0 and failed is None:
                failed = (status, what)
        else:
            keep.append((ev, host, what, status))
    if keep:
        with _PENDING_LOCK:
            _PENDING[:0] = keep
    if failed is not None:
        check(*failed)


def index_fingerprint(*tensors: torch.Tensor) -> torch.Tensor:
    """[len(tensors)][2] int64 device tensor: the 128-bit content fingerprint of each (contiguous) index tensor; queued on the
    current stream, nothing is read back here."""
    dev = require_device(*tensors)
    out = torch.zeros((len(tensors), 2), dtype=torch.int64, device=dev)      # (one fill for all the words; the launches accumulate)
    for i, t in enumerate(tensors):
        launch("tsgu_index_fingerprint", dev, itype_of(t), t.numel(), t.contiguous(), out[i], 1)
    return out


def index_fingerprint_match(tensors, refs=None, copy: bool = False, hash: bool = True):
    """One pass per index tensor (see tsgu_index_fingerprint_match): returns (words, copies) — `words` a [len(tensors)][3] int64
    device tensor {fingerprint word 0, word 1, non-zero iff the tensor differs from its `refs` entry}, `copies` fresh contiguous
    copies of the tensors (None unless `copy`).  `hash=False` (with `refs`, without `copy`): compare only — the fingerprint words stay 0
    (equal tensors have their reference's fingerprint).  Queued on the current stream, nothing is read back here."""
    dev = require_device(*tensors)
    out = torch.zeros((len(tensors), 3), dtype=torch.int64, device=dev)
    copies = [] if copy else None
    for i, t in enumerate(tensors):
        t = t.contiguous()
        r = None
        if refs is not None:
            r = refs[i]
            if r.dtype != t.dtype or r.numel() != t.numel() or r.device != t.device or not r.is_contiguous():
                raise ValueError("index_fingerprint_match: a reference tensor does not have the geometry of its index tensor")
        c = torch.empty_like(t) if copy else None
        launch("tsgu_index_fingerprint_match", dev, itype_of(t), t.numel(), t, r, c, out[i], 1 | (0 if hash or r is None or copy else 2))
        if copy:
            copies.append(c)
    return out, copies


KRYLOV_SLAB = 256      # columns one workgroup of the Krylov kernels covers with scalar lanes (kBlock in csrc/tsgu_common.h)


def krylov_width_rule(dtype: torch.dtype) -> str:
    """The column counts the fused step kernels (K5, K6, K7 of include/tsgu_hip.h) accept, in words."""
    wide = 16 // torch.empty((), dtype=dtype).element_size()
    return (f"any number up to {KRYLOV_SLAB}, and above that multiples of {wide} up to {KRYLOV_SLAB * wide} "
            f"(16-byte lanes of {wide} {dtype} columns)")


def krylov_num_blocks(who: str, t: torch.Tensor, n: int, p: int) -> int:
    """tsgu_cg_num_blocks for an (n, p) state of t's dtype; a width the step kernels do not take raises with the rule."""
    nb = load_library().tsgu_cg_num_blocks(vtype_of(t), n, p)
    if nb < 0:
        raise RuntimeError(f"{who}: {p} simultaneous right-hand sides are not supported by the fused kernels, which take "
                           f"{krylov_width_rule(t.dtype)}")
    return nb


def coldot(X, Y):
    """Column-wise dot products of two (n, p) arrays -> (p,) tensor (deterministic).  More than 256 columns are walked in
    slabs of 256 through the operands' leading dimensions (tsgu_coldot reads strided rows), one launch pair per slab."""
    if not X.is_cuda and not Y.is_cuda:
        from . import _cpu

        return _cpu.coldot(X, Y)
    lib = load_library()
    dev = require_device(X, Y)
    if X.dtype != Y.dtype:
        raise RuntimeError(f"tsgu_coldot: expected both operands to have the same dtype, got {X.dtype} and {Y.dtype}")
    X, Y = rowmajor(X), rowmajor(Y)
    n, p = X.shape
    vt, ldx, ldy = vtype_of(X), _ld(X), _ld(Y)
    out = torch.empty((p,), dtype=X.dtype, device=dev)
    if p == 0:
        return out
    partial = torch.empty((lib.tsgu_coldot_max_blocks(n, min(p, KRYLOV_SLAB)), min(p, KRYLOV_SLAB)), dtype=X.dtype, device=dev)
    for c0 in range(0, p, KRYLOV_SLAB):
        w = min(KRYLOV_SLAB, p - c0)
        launch("tsgu_coldot", dev, vt, n, w, X[:, c0:], ldx, Y[:, c0:], ldy, partial, out[c0:])
    return out


def gmres_geometry(dtype: torch.dtype, n: int, p: int):
    """(restart cap, basis group size, rows per workgroup, partial rows per launch) of the GMRES kernels for an (n, p) block
    (csrc/tsgu_hip_gmres.h).  Host only; a width the lane geometry does not cover raises with the rule."""
    fn = load_library().tsgu_gmres_geometry
    cap, group, rows, parts = _int(0), _int(0), _i64(0), _i64(0)
    rc = fn(_VTYPE[dtype], n, p, ctypes.byref(cap), ctypes.byref(group), ctypes.byref(rows), ctypes.byref(parts))
    if rc == -3:
        raise RuntimeError(f"gmres: {p} simultaneous right-hand sides are not supported by the fused kernels, which take "
                           f"{krylov_width_rule(dtype)}")
    check(rc, "tsgu_gmres_geometry")
    return cap.value, group.value, rows.value, parts.value


def gmres_state_rows(m: int) -> dict:
    """First row of every field of the GMRES `scal` state for restart length m, and the row count (csrc/tsgu_hip_gmres.h)."""
    return {"threshold": 0, "estimate": 1, "hnorm": 2, "g": 3, "cs": m + 4, "sn": 2 * m + 4, "y": 3 * m + 4, "h": 4 * m + 4,
            "coef": 5 * m + 4, "R": 6 * m + 4, "rows": m * m + 6 * m + 4}


GMRES_FLAG_WORDS = 4      # words in front of the per-column arrays of the GMRES `flags` (finished | cycle ended | steps | iterations)


def device_copy(src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst <- src by the library's own 16-bytes-per-lane streaming kernel (the measured HBM ceiling of bench.py)."""
    dev = require_device(src, dst)
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() != nbytes or not (src.is_contiguous() and dst.is_contiguous()):
        raise RuntimeError("device_copy: contiguous tensors of equal byte size expected")
    launch("tsgu_device_copy", dev, src, dst, nbytes)


def device_cu_count(index: int = 0) -> int:
    lib = load_library()
    n = _int(0)
    check(lib.tsgu_device_cu_count(index, ctypes.byref(n)), "tsgu_device_cu_count")
    return n.value


def device_info(index: int = 0):
    lib = load_library()
    name = ctypes.create_string_buffer(128)
    ncu, wave = _int(0), _int(0)
    check(lib.tsgu_device_info(index, name, 128, ctypes.byref(ncu), ctypes.byref(wave)), "tsgu_device_info")
    return name.value.decode(), ncu.value, wave.value


# ---- density reductions of the sparse multivariate normal (csrc/mvn.hip) ----------------------------------------------------------
MVN_DTYPES = (torch.float32, torch.float64)      # (fp32 sums in fp32, fp64 in fp64; bf16 is not offered)


def _mvn_partial(n_out: int, rows_per_item: int, dtype: torch.dtype, dev: torch.device):
    nb = load_library().tsgu_mvn_reduce_blocks(rows_per_item)
    return torch.empty(max(n_out * nb, 1), dtype=dtype, device=dev)


def _mvn_dtype(*tensors) -> None:
    for t in tensors:
        if t is not None and t.dtype not in MVN_DTYPES:
            raise TypeError(f"the density kernels take float32 and float64 operands, got {t.dtype}")
    kinds = {t.dtype for t in tensors if t is not None}
    if len(kinds) > 1:
        raise RuntimeError(f"expected all operands to have the same dtype, got {sorted(str(k) for k in kinds)}")


def csr_diag_positions(crow, col, perm, n_rows: int):
    """pos[i] = position in the owner's value array of row i's diagonal entry (-1: none stored), for a 2-D row-gather pattern."""
    dev = require_device(crow, col, perm)
    crow, col = crow.contiguous(), col.contiguous()
    perm = None if perm is None else perm.contiguous()
    if col.dtype != crow.dtype or (perm is not None and perm.dtype != crow.dtype):
        raise RuntimeError("index dtypes differ")
    if crow.numel() != n_rows + 1:
        raise RuntimeError(f"a pattern of {n_rows} rows needs a row pointer of {n_rows + 1} words, got {crow.numel()}")
    pos = torch.empty(n_rows, dtype=crow.dtype, device=dev)
    launch("tsgu_csr_diag_positions", dev, itype_of(crow), n_rows, col.numel(), crow, col, perm, pos)
    return pos


def diag_logsum(pos, val, n_rows: int, rows_per_item: int):
    """(items,) tensor of Σ_i log(val[pos[i]]) per item (pos None: Σ_i log(val[i]) of a dense vector of n_rows elements)."""
    _mvn_dtype(val)
    dev = require_device(pos, val)
    val = val.contiguous()
    if rows_per_item <= 0 or n_rows % rows_per_item or (pos is not None and pos.numel() != n_rows) or (pos is None and val.numel() != n_rows):
        raise RuntimeError("diag_logsum: operands of unexpected size")
    items = n_rows // rows_per_item
    out = torch.empty(items, dtype=val.dtype, device=dev)
    partial = _mvn_partial(items, rows_per_item, val.dtype, dev)
    launch("tsgu_diag_logsum", dev, vtype_of(val), itype_of(pos) if pos is not None else TSGU_I64, n_rows, rows_per_item, val.numel(), pos, val,
           out, partial, partial.numel())
    return out


def diag_logsum_backward(crow, perm, pos, val, g, n_rows: int, rows_per_item: int, grad=None):
    """Gradient of `diag_logsum` in the value array: written into a new array (zero off the diagonal), or added in place to the
    diagonal entries of `grad`."""
    _mvn_dtype(val, g, grad)
    dev = require_device(crow, perm, pos, val, g, grad)
    val, g = val.contiguous(), g.contiguous()
    if g.numel() * rows_per_item != n_rows or (pos is not None and pos.numel() != n_rows):
        raise RuntimeError("diag_logsum_backward: operands of unexpected size")
    fill = grad is None
    if fill:
        grad = torch.empty_like(val)
    elif not grad.is_contiguous() or grad.numel() != val.numel():
        raise RuntimeError("diag_logsum_backward: the gradient to update must be contiguous and of the values' size")
    if pos is not None:
        crow = crow.contiguous()
        perm = None if perm is None else perm.contiguous()
        if crow.numel() != n_rows + 1 or crow.dtype != pos.dtype or (perm is not None and perm.dtype != pos.dtype):
            raise RuntimeError("diag_logsum_backward: index arrays of unexpected size or dtype")
    launch("tsgu_diag_logsum_backward", dev, vtype_of(val), itype_of(pos) if pos is not None else TSGU_I64, n_rows, rows_per_item, val.numel(),
           crow if pos is not None else None, perm if pos is not None else None, pos, val, g, grad, int(fill))
    return grad


def _quad_operands(Y, E, w, rows_per_item: int):
    _mvn_dtype(Y, E, w)
    dev = require_device(Y, E, w)
    if Y.dim() != 2 or (E is not None and E.shape != Y.shape):
        raise RuntimeError("quadform: Y (and E) must be 2-D arrays of one shape")
    n, k = Y.shape
    if rows_per_item <= 0 or n % rows_per_item:
        raise RuntimeError("quadform: the rows are not a whole number of items")
    if w is not None:
        w = w.contiguous()
        if w.numel() != n:
            raise RuntimeError("quadform: one weight per row expected")
    return dev, n, k, w


def quadform(Y, E, w, w_mode: int, rows_per_item: int):
    """(items, k) tensor of Σ_i w_i^{±1} (Y[i,c] + E[i,c])² per item; Y and E are read through their strides."""
    dev, n, k, w = _quad_operands(Y, E, w, rows_per_item)
    items = n // rows_per_item
    out = torch.empty((items, k), dtype=Y.dtype, device=dev)
    partial = _mvn_partial(items * k, rows_per_item, Y.dtype, dev)
    launch("tsgu_quadform", dev, vtype_of(Y), n, k, Y, Y.stride(0), Y.stride(1), E, E.stride(0) if E is not None else 0,
           E.stride(1) if E is not None else 0, w, w_mode if w is not None else 0, rows_per_item, out, partial, partial.numel())
    return out


def quadform_backward(Y, E, w, w_mode: int, rows_per_item: int, g, want_w: bool):
    """(grad_Y in Y's layout, grad_w or None) of `quadform` for the upstream gradient g (items, k)."""
    dev, n, k, w = _quad_operands(Y, E, w, rows_per_item)
    _mvn_dtype(Y, g)
    g = g.contiguous()
    if g.numel() != (n // rows_per_item) * k or not g.is_cuda:
        raise RuntimeError("quadform_backward: upstream gradient of unexpected size or device")
    if k > 1 and Y.stride(0) == 1:
        gY = torch.empty((k, n), dtype=Y.dtype, device=dev).t()      # a transposed view in, the same layout out
    else:
        gY = torch.empty((n, k), dtype=Y.dtype, device=dev)
    gw = torch.empty(n, dtype=Y.dtype, device=dev) if (want_w and w is not None) else None
    launch("tsgu_quadform_backward", dev, vtype_of(Y), n, k, Y, Y.stride(0), Y.stride(1), E, E.stride(0) if E is not None else 0,
           E.stride(1) if E is not None else 0, w, w_mode if w is not None else 0, rows_per_item, g, gY, gY.stride(0), gY.stride(1), gw)
    return gY, gw


def _sumsq_operands(crow, col, perm, val, w, n_rows: int):
    _mvn_dtype(val, w)
    dev = require_device(crow, col, perm, val, w)
    crow, col, val = crow.contiguous(), col.contiguous(), val.contiguous()
    perm = None if perm is None else perm.contiguous()
    w = None if w is None else w.contiguous()
    if crow.numel() != n_rows + 1 or col.dtype != crow.dtype or (perm is not None and perm.dtype != crow.dtype) or col.numel() != val.numel():
        raise RuntimeError("row_sumsq: index arrays of unexpected size or dtype")
    return dev, crow, col, perm, val, w


def csr_row_sumsq(crow, col, perm, val, w, add, n_rows: int):
    """out[i] = add[i] + Σ_{k in row i} val[k]² w[col[k]]  (w, add optional)."""
    dev, crow, col, perm, val, w = _sumsq_operands(crow, col, perm, val, w, n_rows)
    _mvn_dtype(val, add)
    add = None if add is None else add.contiguous()
    if add is not None and (add.numel() != n_rows or not add.is_cuda):
        raise RuntimeError("row_sumsq: one addend per row expected")
    out = torch.empty(n_rows, dtype=val.dtype, device=dev)
    launch("tsgu_csr_row_sumsq", dev, vtype_of(val), itype_of(crow), n_rows, val.numel(), w.numel() if w is not None else 0, crow, col, perm, val,
           w, add, out)
    return out


def csr_row_sumsq_backward(crow, col, perm, val, w, g, n_rows: int):
    """grad_val[k] = 2 g[row(k)] val[k] w[col[k]] in the value array's order."""
    dev, crow, col, perm, val, w = _sumsq_operands(crow, col, perm, val, w, n_rows)
    _mvn_dtype(val, g)
    g = g.contiguous()
    if g.numel() != n_rows or not g.is_cuda:
        raise RuntimeError("row_sumsq_backward: one upstream value per row expected")
    grad = torch.empty_like(val) if n_rows else torch.zeros_like(val)
    launch("tsgu_csr_row_sumsq_backward", dev, vtype_of(val), itype_of(crow), n_rows, val.numel(), w.numel() if w is not None else 0, crow, col,
           perm, val, w, g, grad)
    return grad


# ---- Lanczos quadrature and Rademacher probes (csrc/tsgu_hip_quadrature.h; sparse_logdet.py) ------------------------------------
QUAD_CG, QUAD_ENTRIES = 0, 1                                   # `kind`: rows of CG coefficients | rows of (diagonal, off-diagonal)
QUAD_LOG, QUAD_RECIPROCAL, QUAD_IDENTITY, QUAD_ONE = 0, 1, 2, 3  # `fn`
QUAD_NO_WORK_ROWS = 64                                         # the header's promise: r up to here never reads `work`


@functools.lru_cache(maxsize=None)
def quadrature_geometry():
    """(steps_cap, work_bytes_per_column) of tsgu_tridiag_quadrature.  Host only."""
    return _query("tsgu_quadrature_geometry")


def tridiag_quadrature(coef, kind: int = QUAD_CG, fn: int = QUAD_LOG, scale=None, p: int = None):
    """(out, info) of tsgu_tridiag_quadrature for the first `p` columns (default: all) of the contiguous [r][2][width] array `coef`
    of float32 or float64: out[c] = scale[c]·Σ_j τ_j² f(λ_j) in coef's dtype, info[c] = ±r_c (int32).  One launch, no host read."""
    dev = require_device(coef, scale)
    if coef.dim() != 3 or coef.size(1) != 2 or not coef.is_contiguous():
        raise RuntimeError(f"tsgu_tridiag_quadrature: coef must be a contiguous [r][2][p] array, got {tuple(coef.shape)}")
    r, width = coef.size(0), coef.size(2)
    p = width if p is None else int(p)
    if not 0 < p <= width:
        raise RuntimeError(f"tsgu_tridiag_quadrature: {p} columns asked of an array of {width}")
    if p != width:
        # (the kernel takes a dense [r][2][p] array: the leading columns of a wider history are packed first)
        coef = coef[:, :, :p].contiguous()
    if scale is not None:
        scale = scale.contiguous()
        if scale.dtype != coef.dtype or scale.numel() != p:
            raise RuntimeError(f"tsgu_tridiag_quadrature: scale must hold {p} values of {coef.dtype}")
    out = torch.empty(p, dtype=coef.dtype, device=dev)
    info = torch.empty(p, dtype=torch.int32, device=dev)
    work = None
    if r > QUAD_NO_WORK_ROWS:
        work = torch.empty(p * quadrature_geometry()[1] // 8, dtype=torch.float64, device=dev)
    launch("tsgu_tridiag_quadrature", dev, vtype_of(coef), int(kind), int(fn), r, p, coef, scale, out, info, work)
    return out, info


def rademacher_fill(n: int, p: int, seed: int, dtype: torch.dtype, device) -> torch.Tensor:
    """The (n, p) block of ±1 of tsgu_rademacher_fill: a pure function of (seed, row, column), the same bits as `_cpu.rademacher_fill`."""
    device = torch.device(device)
    if device.type != "cuda":
        from . import _cpu

        return _cpu.rademacher_fill(n, p, seed, dtype)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((n, p), dtype=dtype, device=device)
    launch("tsgu_rademacher_fill", device, vtype_of(out), n, p, _i64(int(seed)).value, out)
    return out


# ---- contour-quadrature update (csrc/tsgu_hip_ciq.h; sparse_sqrt.py) ---------------------------------------------------------------
def ciq_geometry(dtype: torch.dtype, n: int, p: int):
    """(shift cap, plane alignment in elements, rows per workgroup, workgroups) of tsgu_ciq_update for an (n, p) block.  Host only;
    a width the lane geometry does not cover raises with the rule."""
    fn = load_library().tsgu_ciq_geometry
    cap, align, rows, groups = _int(0), _int(0), _i64(0), _i64(0)
    rc = fn(_VTYPE[dtype], n, p, ctypes.byref(cap), ctypes.byref(align), ctypes.byref(rows), ctypes.byref(groups))
    if rc == -3:
        raise RuntimeError(f"tsgu_ciq_geometry: {p} simultaneous right-hand sides are not supported by the fused kernels, which take "
                           f"{krylov_width_rule(dtype)}")
    check(rc, "tsgu_ciq_geometry")
    return cap.value, align.value, rows.value, groups.value


def ciq_update(zc, zp, wpp, wp, shift_stride: int, acc, keep, scal, omega, done, flags) -> None:
    """One tsgu_ciq_update launch on the (n, p) state `zc`: see csrc/tsgu_hip_ciq.h.  `keep` may be None."""
    dev = require_device(zc, zp, wpp, wp, acc, keep, scal, omega, done, flags)
    n, p = zc.shape
    launch("tsgu_ciq_update", dev, vtype_of(zc), n, p, omega.numel(), zc, zp, wpp, wp, int(shift_stride), acc, keep, scal, omega, done,
           flags)


def ciq_stop(scal, tol: float, est, done, flags) -> None:
    """One tsgu_ciq_stop launch on scal [S][12][p]: see csrc/tsgu_hip_ciq.h."""
    dev = require_device(scal, est, done, flags)
    launch("tsgu_ciq_stop", dev, vtype_of(scal), scal.size(2), scal.size(0), scal, float(tol), est, done, flags)


# ---- Chebyshev recurrence (csrc/tsgu_hip_expm.h; sparse_expm.py) --------------------------------------------------------------------
def expm_geometry(dtype: torch.dtype, n: int, p: int):
    """(time cap, chunk cap, plane alignment in elements, rows per workgroup, workgroups) of tsgu_cheb_step / tsgu_cheb_combine for an
    (n, p) block.  Host only; a width the lane geometry does not cover raises with the rule."""
    fn = load_library().tsgu_expm_geometry
    tcap, ccap, align, rows, groups = _int(0), _int(0), _int(0), _i64(0), _i64(0)
    rc = fn(_VTYPE[dtype], n, p, ctypes.byref(tcap), ctypes.byref(ccap), ctypes.byref(align), ctypes.byref(rows), ctypes.byref(groups))
    if rc == -3:
        raise RuntimeError(f"tsgu_expm_geometry: {p} simultaneous right-hand sides are not supported by the fused kernels, which take "
                           f"{krylov_width_rule(dtype)}")
    check(rc, "tsgu_expm_geometry")
    return tcap.value, ccap.value, align.value, rows.value, groups.value


def cheb_step(prod, x, prev, alpha: float, beta: float, gamma: float, flags, src=None, src_slot: int = 0, chunk=None, slot: int = 0) -> None:
    """One tsgu_cheb_step launch on the (n, p) state `prev`: see csrc/tsgu_hip_expm.h.  `prod`, `src` and `chunk` may be None; `src`
    and `chunk` are (n, slots, p)."""
    dev = require_device(prod, x, prev, src, chunk, flags)
    n, p = prev.shape
    launch("tsgu_cheb_step", dev, vtype_of(prev), n, p, prod, x, prev, float(alpha), float(beta), float(gamma), src,
           0 if src is None else src.size(1), int(src_slot), chunk, 0 if chunk is None else chunk.size(1), int(slot), flags)


def cheb_combine(mode: int, chunk, coef, planes, plane_stride: int, flags, accumulate: bool = False) -> None:
    """One tsgu_cheb_combine launch: `chunk` (n, m, p), `coef` (m, T, p), `planes` the T arrays (n, p) `plane_stride` elements apart
    (mode 0 writes them, mode 1 reads them): see csrc/tsgu_hip_expm.h."""
    dev = require_device(chunk, coef, planes, flags)
    n, m, p = chunk.shape
    launch("tsgu_cheb_combine", dev, vtype_of(chunk), int(mode), int(bool(accumulate)), n, p, m, coef.size(1), chunk, coef, planes,
           int(plane_stride), flags)


# ---- top-k of a dense product as CSR arrays (csrc/tsgu_hip_topk.h; sparse_topk.py) --------------------------------------------------
TOPK_CAUSAL, TOPK_EXCLUDE_SELF = 1, 2


def topk_geometry(dtype: torch.dtype, d: int = 1, k: int = 1):
    """(cap on k, rows per workgroup, keys per tile, columns per LDS stage, dynamic LDS bytes) of tsgu_topk_mm.  Host only; a k above
    the cap raises."""
    return _query("tsgu_topk_geometry", _VTYPE[dtype], int(d), int(k))


def topk_mm(Q, K, key_bias, k: int, scale: float, flags: int, causal_offset: int, crow, col, val) -> None:
    """One tsgu_topk_mm launch: Q (b, n, d), K (b, m, d) and key_bias (b, m) or None, contiguous; crow (n + 1,) shared by the batch
    items; col and val (b, nnz) are written.  See csrc/tsgu_hip_topk.h."""
    dev = require_device(Q, K, key_bias, crow, col, val)
    b, n, d = Q.shape
    m = K.size(1)
    launch("tsgu_topk_mm", dev, vtype_of(Q), Q, K, key_bias, n, m, d, int(k), float(scale), int(flags), int(causal_offset), crow, col, val,
           itype_of(crow), b, n * d, m * d, m, col.size(1))


# ---- 2:4 semi-structured operands (csrc/tsgu_hip_semi.h; sparse_semi_structured.py) --------------------------------------------------
# Every wrapper takes 2-D tensors with unit stride in the last dimension (`rowmajor`) and passes the row strides on: sliced views
# are consumed in place.  `meta` is the int32 (m, 4·ceil(k / 128)) position tensor of the header.
SEMI_DENSE_T, SEMI_OUT_T = 1, 2


def semi_geometry(dtype: torch.dtype, k: int = 0):
    """(meta words per row, tile rows, tile columns, dense columns per LDS stage, 1 if the sparse instruction serves the dtype) of
    tsgu_semi_mm.  Host only."""
    return _query("tsgu_semi_geometry", _VTYPE[dtype], int(k))


def semi_meta_words(k: int) -> int:
    return 4 * ((k + 127) // 128)


def semi_prune(W: torch.Tensor):
    """(values (m, k / 2), meta) of the dense (m, k) matrix W: one tsgu_semi_prune launch."""
    dev = require_device(W)
    W = rowmajor(W)
    m, k = W.shape
    val = torch.empty((m, k // 2), dtype=W.dtype, device=dev)
    meta = torch.empty((m, semi_meta_words(k)), dtype=torch.int32, device=dev)
    launch("tsgu_semi_prune", dev, vtype_of(W), W, _ld(W), m, k, val, max(k // 2, 1), meta, max(meta.size(1), 4))
    return val, meta


def semi_expand(val: torch.Tensor, meta: torch.Tensor, k: int) -> torch.Tensor:
    """The dense (m, k) matrix of (val, meta): one tsgu_semi_expand launch."""
    dev = require_device(val, meta)
    val = rowmajor(val)
    m = val.size(0)
    out = torch.empty((m, k), dtype=val.dtype, device=dev)
    launch("tsgu_semi_expand", dev, vtype_of(val), val, _ld(val), meta, max(meta.size(1), 4), m, k, out, max(k, 1))
    return out


def semi_mm(val, meta, k: int, Y, bias, linear: bool, smfmac: bool) -> torch.Tensor:
    """A·Y for Y (k, p) -> (m, p), or with `linear` Y·Aᵀ (+ bias) for Y (p, k) -> (p, m): one tsgu_semi_mm launch.  `smfmac` selects
    the sparse matrix instruction (bfloat16 only)."""
    dev = require_device(val, meta, Y, bias)
    val, Y = rowmajor(val), rowmajor(Y)
    m = val.size(0)
    p = Y.size(0) if linear else Y.size(1)
    out = torch.empty((p, m) if linear else (m, p), dtype=val.dtype, device=dev)
    launch("tsgu_semi_mm", dev, vtype_of(val), val, _ld(val), meta, max(meta.size(1), 4), Y, _ld(Y), bias, out, max(out.size(1), 1), m, k, p,
           SEMI_OUT_T if linear else SEMI_DENSE_T, int(bool(smfmac) and val.dtype == torch.bfloat16))
    return out


def semi_mm_t(val, meta, k: int, G, linear: bool) -> torch.Tensor:
    """Aᵀ·G for G (m, p) -> (k, p), or with `linear` G·A for G (p, m) -> (p, k): one tsgu_semi_mm_t launch."""
    dev = require_device(val, meta, G)
    val, G = rowmajor(val), rowmajor(G)
    m = val.size(0)
    p = G.size(0) if linear else G.size(1)
    out = torch.empty((p, k) if linear else (k, p), dtype=val.dtype, device=dev)
    launch("tsgu_semi_mm_t", dev, vtype_of(val), val, _ld(val), meta, max(meta.size(1), 4), G, _ld(G), out, max(out.size(1), 1), m, k, p,
           (SEMI_DENSE_T | SEMI_OUT_T) if linear else 0)
    return out


def semi_sddmm(meta, m: int, k: int, G, Y, linear: bool) -> torch.Tensor:
    """The gradient of the kept values, (m, k / 2): G (m, p) against Y (k, p), or with `linear` G (p, m) against Y (p, k): one
    tsgu_semi_sddmm launch."""
    dev = require_device(meta, G, Y)
    G, Y = rowmajor(G), rowmajor(Y)
    p = G.size(0) if linear else G.size(1)
    out = torch.empty((m, k // 2), dtype=G.dtype, device=dev)
    launch("tsgu_semi_sddmm", dev, vtype_of(G), G, _ld(G), Y, _ld(Y), meta, max(meta.size(1), 4), out, max(k // 2, 1), m, k, p,
           SEMI_DENSE_T if linear else 0)
    return out
