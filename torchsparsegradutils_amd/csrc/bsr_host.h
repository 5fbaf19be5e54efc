// What the entry points of the two BSR families share on the host (bsr.hip, bsr_attention.hip).
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int64_t kI31 = 0x7fffffffLL;

struct Dense { const void* ptr; int64_t ld; };

inline int elem_bytes(int vtype) { return vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 8 : vtype == TSGU_BF16 ? 2 : 0; }

// A workgroup owns T rows of the walked side: per_tile = T / oh whole block rows while the owned block height oh fits, else one of
// `pieces` pieces of one block row.  `tiles`: the workgroups that makes.
struct BsrSplit { int64_t per_tile, pieces, tiles; };
inline BsrSplit bsr_tile_split(int64_t oh, int64_t T, int64_t n_groups) {
    if (oh <= T) return {T / oh, 1, (n_groups + T / oh - 1) / (T / oh)};
    return {1, (oh + T - 1) / T, n_groups * ((oh + T - 1) / T)};
}

// The refusals every BSR entry point shares, in two pieces around the ones of its own (the order: include/tsgu_hip_bsr*.h).
// First the pointers and types.  `always`: pointers every call needs; `stored`: those only a pattern with blocks dereferences.
inline int bsr_check_args(int vtype, int itype, int64_t nnzb, std::initializer_list<const void*> always, std::initializer_list<const void*> stored) {
    for (const void* q : always)
        if (!q) return TSGU_ERR_BAD_ARG;
    for (const void* q : stored)
        if (!q && nnzb > 0) return TSGU_ERR_BAD_ARG;
    if (!elem_bytes(vtype) || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    return TSGU_OK;
}
// ... and last the sizes (bh, bw >= 1 and the counts >= 0 by then).  `null_ok`: a null dense operand is not looked at.
inline int bsr_check_sizes(int64_t nrb, int64_t ncb, int64_t nnzb, int64_t bh, int64_t bw, std::initializer_list<Dense> dense, bool null_ok) {
    for (const Dense& o : dense)
        if (!(null_ok && !o.ptr) && o.ld > 0xffffffffLL) return TSGU_ERR_TOO_LARGE;
    if (bh > kI31 || bw > kI31 || nnzb > kI31 / bh / bw || nrb > kI31 / bh || ncb > kI31 / bw) return TSGU_ERR_TOO_LARGE;
    return TSGU_OK;
}

}  // namespace tsgu
