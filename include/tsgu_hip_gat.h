/*
 * tsgu_hip_gat.h — fused graph-attention layers over a sparse pattern (sparse_gat.py): entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the conventions stated in tsgu_hip_semiring.h (device
 * pointers, leading dimensions in elements, `device` + `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no
 * allocation, no global atomics, graph-capturable).  The entries are additive, so TSGU_ABI_VERSION stays as it is.  The reference
 * has no counterpart.
 *
 *   kind 0 (GAT)    e[i,j,h] = lrelu(s_dst[i,h] + s_src[j,h]) + bias[i,j]                       O[i,h,:] = sum_j P[i,j,h] * X_src[j,h,:]
 *   kind 1 (GATv2)  e[i,j,h] = sum_k att[h,k] * lrelu(X_dst[i,h,k] + X_src[j,h,k]) + bias[i,j]   O[i,h,:] = sum_j P[i,j,h] * X_src[j,h,:]
 *
 * with P[i,.,h] the softmax of e over the stored j of row i and lrelu(z) = z > 0 ? z : slope * z (derivative `slope` at 0).  For
 * kind 0 `X_src` is the message matrix V and X_dst / att are not read; for kind 1 s_dst / s_src are not read.  Operands a kind does
 * not read may be NULL.
 *
 * (ptr, idx, perm) walks the pattern by rows: entry k of the walk has column idx[k] and its bias at bias[perm[k]] (perm NULL: k;
 * bias NULL: no bias).  The column pass takes the transposed walk of the same pattern (tptr over the columns, tidx = the row of
 * every entry, tperm = its position in the bias array).  int32 or int64 index arrays, all of one type.
 *
 * Dense rows are [*, heads * d] with a row stride >= heads * d, base pointers and row strides multiples of 16 bytes; s_dst, s_src,
 * ds_dst, ds_src are [*, heads] and att, datt are [heads * d], all without padding.  d is 8, 16, 32, 64 or 128 and heads * d <= 1024.
 * lse, delta ([n_rows, heads]), dA ([nnz]) and partials are in the ACCUMULATOR type (float for TSGU_F32 / TSGU_BF16, double for
 * TSGU_F64); a bf16 result is the float result rounded once.  Row counts below 2^31.
 *
 * Special values: a row without entries gives zeros and lse = -inf; a -inf logit beside finite ones has weight 0; a row with a
 * NaN, a +inf or only -inf logits is NaN for that head.  Deterministic: every sum in a fixed order that depends on the row's
 * (column's) own entries only; datt on the number of rows.
 */
#ifndef TSGU_HIP_GAT_H
#define TSGU_HIP_GAT_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch geometry of (vtype, kind, heads, d), for callers that size test cases and the partials buffer.  Host only.
 *   rows_per_block   rows (columns, for the column pass) one workgroup owns
 *   stage_entries    entries of the workgroup's (idx, bias) slice staged at a time by the FORWARD of this kind
 *   tile_width       elements of a dense row one pass of the row's lanes covers */
int tsgu_gat_geometry(int vtype, int kind, int heads, int d, int* rows_per_block, int* stage_entries, int* tile_width);

/* Forward: writes O[n_rows, heads * d] and lse[n_rows, heads]. */
int tsgu_csr_gat_forward(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                         const void* perm, const void* bias, const void* s_dst, const void* s_src, const void* X_dst, int64_t ldxd,
                         const void* X_src, int64_t ldxs, const void* att, int heads, int d, double slope, void* O, int64_t ldo,
                         void* lse, int device, void* stream);

/* Backward over the rows: writes delta[n_rows, heads], dA[nnz] when it is not NULL, and d_dst — kind 0: ds_dst[n_rows, heads]
 * (ldd is ignored); kind 1: dX_dst[n_rows, heads * d] with row stride ldd, and partials[n_partials, heads * d], the workgroups'
 * shares of datt, n_partials = ceil(n_rows / rows_per_block). */
int tsgu_csr_gat_backward_rows(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                               const void* idx, const void* perm, const void* bias, const void* s_dst, const void* s_src,
                               const void* X_dst, int64_t ldxd, const void* X_src, int64_t ldxs, const void* att, const void* dO,
                               int64_t lddo, const void* lse, int heads, int d, double slope, void* d_dst, int64_t ldd, void* delta,
                               void* dA, void* partials, int64_t n_partials, int device, void* stream);

/* Backward over the columns (the transposed walk): writes d_src[n_cols, heads * d] — kind 0: dV; kind 1: dX_src, both of its
 * terms — and for kind 0 ds_src[n_cols, heads]. */
int tsgu_csr_gat_backward_cols(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                               const void* tidx, const void* tperm, const void* bias, const void* s_dst, const void* s_src,
                               const void* X_dst, int64_t ldxd, const void* X_src, int64_t ldxs, const void* att, const void* dO,
                               int64_t lddo, const void* lse, const void* delta, int heads, int d, double slope, void* d_src,
                               int64_t ldds, void* ds_src, int device, void* stream);

/* datt[heads * d] (vtype) = the sum of partials[n_partials, heads * d] over the workgroups in a fixed order; n_partials = 0 gives
 * zeros. */
int tsgu_gat_fold(int vtype, const void* partials, int64_t n_partials, int heads, int d, void* datt, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_GAT_H */
