/*
 * tsgu_hip_mm_reduce.h — sparse × dense products reduced with max / min instead of a sum: entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, leading dimensions in elements, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart; torch.sparse.mm(A, B, reduce) has these semantics for CSR
 * operands on the CPU only.
 *
 *   C[i,k] = max (op = 0) or min (op = 1) over the stored entries e of row i of  val[e] * B[idx[e], k]
 *
 * Only stored entries are candidates (an absent entry is not a zero).  The product is formed in the accumulator type (float for
 * TSGU_F32 and TSGU_BF16, double for TSGU_F64) and compared there; bf16 is rounded once when C is stored.  A candidate replaces
 * the running one on a strict > / < only: of equal candidates (+0.0 and -0.0 are equal) the one at the lowest stored position
 * wins.  A NaN candidate wins over any number, and the first NaN stays.  arg[i,k] (int32) is the winner's position in the value
 * array; a row without entries gives C = 0 and arg = -1.  Positions are int32: nnz < 2^31 (TSGU_ERR_TOO_LARGE beyond).
 *
 * Dense operands are row-major with a row stride (ld*, in elements) >= p, 1 <= p.  When p, every row stride and every base
 * pointer of a call are multiples of 16 bytes (arg: of 16 / sizeof(value) entries) the rows are touched in 16-byte lanes, else
 * element by element: alignment is never a reason for a refusal beyond whole elements.  Row counts below 2^31, strides below 2^32.
 *
 * The gradients flow through the winner only, from the forward's arg:
 *   dval[e] = sum_{k: arg[i,k] = e} G[i,k] * B[idx[e],k]           (row i of e; an entry that wins nothing gets exactly 0)
 *   dB[j,k] = sum_{e in column j: arg[i,k] = e} val[e] * G[i,k]    (over the transposed pattern, in its stored order)
 * Deterministic: no float atomics, every sum in a fixed order that depends on the row's (column's) own entries only.
 */
#ifndef TSGU_HIP_MM_REDUCE_H
#define TSGU_HIP_MM_REDUCE_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch geometry of p columns of `vtype` with 16-byte aligned operands, for callers that size test cases.  Host only.
 *   rows_per_block   rows one workgroup owns
 *   stage_entries    entries of the workgroup's (idx, val) slice staged per pass
 *   cols_per_slice   columns one grid.z slice covers */
int tsgu_csr_spmm_reduce_geometry(int vtype, int64_t p, int* rows_per_block, int* stage_entries, int* cols_per_slice);

/* Forward: writes C[n_rows, p] and arg[n_rows, p].  (ptr[n_rows + 1], idx[nnz], val[nnz]): the CSR arrays. */
int tsgu_csr_spmm_reduce(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                         const void* val, const void* B, int64_t ldb, int64_t p, int op, void* C, int64_t ldc, int* arg,
                         int64_t ldarg, int device, void* stream);

/* Gradient of the values: writes all of dval[nnz] (vtype) in one pass over the rows. */
int tsgu_csr_spmm_reduce_backward_values(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                         const void* idx, const int* arg, int64_t ldarg, const void* G, int64_t ldg, const void* B,
                                         int64_t ldb, int64_t p, void* dval, int device, void* stream);

/* Gradient of B: (tptr[n_cols + 1], tidx = row of every entry, perm = its position in val) is the transposed walk of the same
 * pattern.  Writes dB[n_cols, p]. */
int tsgu_csr_spmm_reduce_backward_dense(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                        const void* tidx, const void* perm, const void* val, const int* arg, int64_t ldarg,
                                        const void* G, int64_t ldg, int64_t p, void* dB, int64_t lddb, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_MM_REDUCE_H */
