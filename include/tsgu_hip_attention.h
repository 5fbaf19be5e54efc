/*
 * tsgu_hip_attention.h — attention over a sparse pattern: the fused SDDMM · softmax · SpMM entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, leading dimensions in elements, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 *   O[i,h,:] = sum_j P[i,j,h] * V[j,h,:],   P[i,.,h] = softmax over the stored j of row i of  scale * <Q[i,h,:], K[j,h,:]> + bias[i,j]
 *
 * The pattern is walked as groups (ptr[n_groups + 1], idx[nnz], perm): entry k of group g (ptr[g] <= k < ptr[g+1]) refers to the
 * dense row idx[k] of the other side, and its bias / dA value is at position perm[k] of the value array (perm = NULL: k).  The
 * row direction of a CSR matrix is (crow, col, NULL); of a CSC matrix its cached transpose (tptr, col, perm).  The column pass
 * takes the other one of the two.
 *
 * Dense operands are [rows, heads * d] with a row stride (ld*, in elements) >= heads * d; every base pointer and every row
 * stride must be a multiple of 16 bytes.  Supported: d in {8, 16, 32, 64, 128}, heads >= 1, heads * d <= 1024
 * (tsgu_csr_attention_supported); row counts and leading dimensions below 2^31.
 * `lse`, `delta` and `dA` are of the ACCUMULATOR type: float for TSGU_F32 and TSGU_BF16, double for TSGU_F64 (bf16 operands are
 * computed in fp32 and rounded once when O, dQ, dK, dV are stored; the caller rounds dA).
 *
 * Absent entries do not take part.  A row without entries gives O = 0, lse = -inf.  A row whose logits hold a NaN or a +inf, or
 * nothing but -inf, gives NaN (O and lse) for that head; -inf beside finite logits has weight 0 and gradient 0.
 * Deterministic: no float atomics, every sum in a fixed order that depends on the row's own entries only.  No nnz-sized
 * intermediate: the backward recomputes the probabilities from lse.  A row (or, in the column pass, a column) is walked by one
 * group of lanes however long it is.
 */
#ifndef TSGU_HIP_ATTENTION_H
#define TSGU_HIP_ATTENTION_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the kernels take (vtype, heads, d), else 0.  Host only. */
int tsgu_csr_attention_supported(int vtype, int heads, int d);

/* The launch geometry of (vtype, heads, d), for callers that size test cases or estimate occupancy.  Host only.
 *   entry_lanes      lanes of a row's group that take different entries of the row concurrently
 *   rows_per_block   rows (groups) one workgroup owns
 *   stage_entries    entries of one staged slice */
int tsgu_csr_attention_geometry(int vtype, int heads, int d, int* entry_lanes, int* rows_per_block, int* stage_entries);

/* Forward: writes O[n_rows, heads*d] and lse[n_rows, heads].  bias: value array of the pattern (vtype) or NULL (no bias). */
int tsgu_csr_attention(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                       const void* perm, const void* bias, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                       int64_t ldv, int heads, int d, double scale, void* O, int64_t ldo, void* lse, int device, void* stream);

/* Backward over the rows (the forward's walk): writes dQ[n_rows, heads*d], delta[n_rows, heads] (for the column pass) and, when
 * dA is not NULL, dA[perm ? perm[k] : k] = sum_h dS[k,h] for every entry. */
int tsgu_csr_attention_backward_rows(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                     const void* idx, const void* perm, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* lse, int heads, int d, double scale, void* dQ, int64_t lddq, void* delta,
                                     void* dA, int device, void* stream);

/* Backward over the columns: (tptr[n_cols + 1], tidx = row of every entry, tperm) is the transposed walk of the same pattern.
 * Reads the forward's lse and the row pass's delta, so it runs after the row pass on the same stream.  Writes dK and dV
 * [n_cols, heads*d]. */
int tsgu_csr_attention_backward_cols(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                     const void* tidx, const void* tperm, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* lse, const void* delta, int heads, int d, double scale, void* dK, int64_t lddk,
                                     void* dV, int64_t lddv, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_ATTENTION_H */
