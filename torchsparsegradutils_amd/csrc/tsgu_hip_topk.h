/*
 * tsgu_hip_topk.h — the k largest of scale·Q·Kᵀ + key_bias per row as CSR arrays (sparse_topk.py): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_TOPK`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation, no global atomics).  The entries are
 * additive, so TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * The score of (row i, column j) is  s = scale * <Q[i], K[j]> (+ key_bias[j]),  accumulated as the matrix-core tile layer does (fp32
 * for TSGU_F32 and TSGU_BF16, fp64 for TSGU_F64; `scale` cast to that type once; one rounding for the product with scale, one for
 * the bias).  The order of the scores is total: NaN above +inf, -0 equal to +0, and among equal scores the LOWER column first.  Row
 * i stores the best crow[i + 1] - crow[i] scores among its allowed columns, columns ascending, values rounded once to the value
 * type.  The scores are never written to global memory.
 */
#ifndef TSGU_HIP_TOPK_H
#define TSGU_HIP_TOPK_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSGU_TOPK_CAUSAL 1        /* flags: column j of row i is allowed only when j <= i + causal_offset */
#define TSGU_TOPK_EXCLUDE_SELF 2  /* flags: column i of row i is not allowed */

/* Host only.  k_cap: the largest k of tsgu_topk_mm (a compile-time constant, at least 128 for every value type);
 * rows_per_workgroup / keys_per_tile: the query rows a workgroup owns and the keys of one tile of its walk; stage_columns: the
 * columns of Q and K of one LDS stage (wider d is walked in stages); lds_bytes: the dynamic LDS of a launch with this k.
 * TSGU_ERR_BAD_ARG for d < 1 or k < 1, TSGU_ERR_TOO_LARGE (k_cap is still written) for k > k_cap. */
int tsgu_topk_geometry(int vtype, int64_t d, int k, int* k_cap, int* rows_per_workgroup, int* keys_per_tile, int* stage_columns,
                       int* lds_bytes);

/* One launch.
 *   Q         [batch][n][d], rows contiguous, `q_stride` elements between batch items
 *   K         [batch][m][d], `k_stride`
 *   key_bias  [batch][m], `bias_stride`, or NULL
 *   crow      [n + 1] of `itype`, an input shared by the batch items: crow[i + 1] - crow[i] = min(k, allowed columns of row i)
 *   col, val  [batch][crow[n]] outputs of `itype` and the value type, `out_stride` elements between batch items
 * Every row's crow[i + 1] - crow[i] entries are written, nothing else.  n = 0, m = 0 or batch = 0 launch nothing.
 * Refused on the host, before the launch: NULL Q, K, crow, col or val, negative sizes or strides, d < 1, k < 1, flags outside the
 * two bits, a non-finite scale, pointers not aligned to their element (TSGU_ERR_BAD_ARG); k > k_cap, n or m at or above 2^31 - 1,
 * more workgroups than a grid holds (TSGU_ERR_TOO_LARGE). */
int tsgu_topk_mm(int vtype, const void* Q, const void* K, const void* key_bias, int64_t n, int64_t m, int64_t d, int k, double scale,
                 int flags, int64_t causal_offset, const void* crow, void* col, void* val, int itype, int64_t batch, int64_t q_stride,
                 int64_t k_stride, int64_t bias_stride, int64_t out_stride, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_TOPK_H */
