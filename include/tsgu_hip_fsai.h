/*
 * tsgu_hip_fsai.h — the factorised sparse approximate inverse (FSAI, Kolotilina–Yeremin): an entry of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream` last, status codes,
 * tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it is.  The
 * reference has no counterpart.
 *
 * Operands: TSGU_F32 and TSGU_F64 with TSGU_I32 or TSGU_I64 indices (TSGU_BF16 is TSGU_ERR_BAD_DTYPE).
 *   (a_ptr[n + 1], a_idx, a_val)   the CSR of tril(A): columns ASCENDING and UNIQUE within every row, the diagonal last
 *   (s_ptr[n + 1], s_idx[s_nnz])   the CSR of the lower-triangular pattern S under the same conditions; every diagonal is stored
 * When S is tril(A)'s own pattern the same arrays are passed twice.  The entry does not check the conditions (the Python plan does,
 * once per pattern); whatever the arrays of S contain, only out[0 … s_nnz) is written.
 *
 * For row i let J = cols_S(i) (ascending, m entries, i last) and A[J,J] the m × m matrix gathered from tril(A): a position that A
 * does not store is zero, and A[j_a, j_b] with j_b <= j_a is taken from row j_a.  Then
 *     solve A[J,J]·y = e_m  (e_m the last unit vector),    g_i = y / sqrt(y_m)   written to row i of out on the pattern S,
 * so that diag(G·A·Gᵀ) = 1 and G·A·Gᵀ ≈ I: M⁻¹ = Gᵀ·G is symmetric positive definite and is applied with two sparse products.
 * The kernel computes the same row as the last row of the inverse Cholesky factor: A[J,J] = L·Lᵀ in place (each l_tk is
 * a_tk minus the products l_tc·l_kc summed in ascending c, divided by l_kk), then Lᵀ·g = e_m by back substitution (products summed
 * in descending row).  One IEEE operation per step in the value type, never contracted; the sums of a row depend on that row
 * alone, so two calls give the same bits whatever the grid, the `order` or the rows that share a wave.
 *
 * Rows are independent: there is no dependency chain, no wait and no work buffer.  A row whose local matrix is not positive
 * definite (a pivot that is not positive, NaN included) is finished with IEEE arithmetic; info[0] (device, int64) is 0 after a
 * clean build and 1 + (the lowest such row) otherwise.  A row of S longer than `row_capacity` is filled with NaN and counts as
 * such a row (the Python plan refuses it beforehand).
 *
 * order: null, or a permutation of 0 … n-1 (itype) in which the rows are dealt to the waves, `rows_per_block` at a time; a wave
 * works at the size class (8, 16, 32 or 64 lanes per row) of the longest row it holds, so a list sorted by row length keeps
 * short rows eight to a wave.  Speed only.  `workgroups_per_cu` (1 … 8): workgroups per compute unit; speed only.
 */
#ifndef TSGU_HIP_FSAI_H
#define TSGU_HIP_FSAI_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For callers that size test cases.  Host only.
 *   row_capacity     the longest row of S (the largest local system) the kernel accepts
 *   rows_per_block   consecutive entries of `order` (rows, when it is null) that one workgroup takes at a time */
int tsgu_csr_fsai_geometry(int vtype, int* row_capacity, int* rows_per_block);

int tsgu_csr_fsai(int vtype, int itype, int64_t n, const void* a_ptr, const void* a_idx, const void* a_val, const void* s_ptr,
                  const void* s_idx, int64_t s_nnz, const void* order, void* out, int64_t* info, int workgroups_per_cu, int device,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_FSAI_H */
