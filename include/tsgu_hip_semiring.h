/*
 * tsgu_hip_semiring.h — sparse × dense products in the log and tropical semirings (sparse_semiring.py): entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, leading
 * dimensions in elements, `device` + `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation, no
 * global atomics).  The entries are additive, so TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 *   semiring 0 (log)       C[i,c] = log sum_e exp(val[e] + B[idx[e], c])      e over the stored entries of row i
 *   semiring 1 (max_plus)  C[i,c] = max_e (val[e] + B[idx[e], c])
 *   semiring 2 (min_plus)  C[i,c] = min_e (val[e] + B[idx[e], c])
 *
 * The candidate t = val + B is ONE addition in the accumulator type (float for TSGU_F32 and TSGU_BF16, double for TSGU_F64); a
 * bf16 C is the float result rounded once.  Only stored entries are candidates.
 *
 * log: a candidate of -inf is an absent entry (weight 0, never NaN); +inf gives +inf; a NaN gives NaN; a row without candidates
 * gives -inf.  C_acc is C in the accumulator type: the backward entries read it (for TSGU_F32 / TSGU_F64 it may be C itself), the
 * forward writes it when it is not NULL.
 *
 * Tropical: the winner rule of tsgu_csr_spmm_reduce with the addition in place of the product — a candidate replaces the running
 * one on a strict compare only, of equal candidates (+0.0 and -0.0 are equal) the lowest stored position wins, a NaN wins over any
 * number and the first NaN stays.  arg[i,c] (int32) is the winner's position in the value array; a row without entries gives the
 * semiring's zero (-inf for max_plus, +inf for min_plus) and arg = -1.  nnz < 2^31.
 *
 * Gradients, with W[e,c] = exp(val[e] + B[idx[e],c] - C_acc[i,c]) (0 where the candidate is -inf) or [arg[i,c] == e]:
 *   dval[e] = sum_c G[i,c] * W[e,c]               dB[j,c] = sum_{e in column j, in the transposed pattern's order} G[i,c] * W[e,c]
 * Deterministic: every sum in a fixed order that depends on the row's (column's) own entries only.
 *
 * Dense operands are row-major with a row stride >= p, 1 <= p.  When p, every row stride and every base pointer of a call are
 * multiples of 16 bytes (arg and C_acc: p and the stride multiples of 16 / sizeof(value) entries) the rows are touched in 16-byte
 * lanes, else element by element.  Row counts below 2^31, strides below 2^32.
 */
#ifndef TSGU_HIP_SEMIRING_H
#define TSGU_HIP_SEMIRING_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch geometry of p columns of `vtype` with 16-byte aligned operands, for callers that size test cases.  Host only.
 *   rows_per_block   rows one workgroup owns
 *   stage_entries    entries of the workgroup's (idx, val) slice staged per pass
 *   cols_per_slice   columns one grid.z slice covers */
int tsgu_semiring_geometry(int vtype, int64_t p, int* rows_per_block, int* stage_entries, int* cols_per_slice);

/* Forward: writes C[n_rows, p]; log: also C_acc[n_rows, p] when it is not NULL (arg is ignored); tropical: arg[n_rows, p]. */
int tsgu_csr_semiring_mm(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                         const void* idx, const void* val, const void* B, int64_t ldb, int64_t p, void* C, int64_t ldc, void* C_acc,
                         int64_t ldacc, int* arg, int64_t ldarg, int device, void* stream);

/* Gradient of the values: writes all of dval[nnz] (vtype) in one pass over the rows.  log reads val, B and C_acc; tropical reads
 * arg only (val, B and C_acc may be NULL). */
int tsgu_csr_semiring_mm_bwd_values(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                    const void* idx, const void* val, const void* B, int64_t ldb, const void* C_acc, int64_t ldacc,
                                    const int* arg, int64_t ldarg, const void* G, int64_t ldg, int64_t p, void* dval, int device,
                                    void* stream);

/* Gradient of B: (tptr[n_cols + 1], tidx = row of every entry, perm = its position in val) is the transposed walk of the same
 * pattern.  Writes dB[n_cols, p].  log reads val, B and C_acc; tropical reads arg only. */
int tsgu_csr_semiring_mm_bwd_dense(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                   const void* tidx, const void* perm, const void* val, const void* B, int64_t ldb, const void* C_acc,
                                   int64_t ldacc, const int* arg, int64_t ldarg, const void* G, int64_t ldg, int64_t p, void* dB,
                                   int64_t lddb, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SEMIRING_H */
