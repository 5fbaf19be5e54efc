/*
 * tsgu_hip_factor.h — zero-fill incomplete factorisations, ILU(0) and IC(0): entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream` last, status codes,
 * tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it is.  The
 * reference has no counterpart; the semantics are those of csrilu02 / csric02, MATLAB's ilu / ichol with no fill, scipy's spilu
 * restricted to the pattern.
 *
 * Operands: TSGU_F32 and TSGU_F64 with TSGU_I32 or TSGU_I64 indices (TSGU_BF16 is TSGU_ERR_BAD_DTYPE).  (ptr[n + 1], idx[nnz]) is
 * a CSR pattern whose columns are ASCENDING and UNIQUE within every row and which stores the diagonal of every row;
 * diag_pos[n] (itype) is the position of each row's diagonal in idx / val.  The entries do not check this (the Python plan
 * does, once per pattern); whatever the arrays contain, a row only ever waits on rows with a smaller index than its own, and every
 * wait is bounded (below).
 *
 * tsgu_csr_ilu0, the IKJ form: out[nnz] on the same pattern, the strict lower part L (unit diagonal implied), the diagonal and
 * the upper part U:
 *     for i = 0 … n-1:                        w = row i of A, its diagonal multiplied by (1 + shift)
 *       for k in cols(i), k < i, ascending:   w_k = w_k / out[k,k]
 *          for j in cols(k), j > k:           if (i,j) is stored: w_j = w_j - w_k * out[k,j]
 *       out[row i] = w
 * One IEEE division, multiplication and subtraction per update in the value type, never contracted, every w_j updated serially in
 * ascending k: the result is bit-identical to this sequential loop, whatever the grid.
 *
 * tsgu_csr_ic0: the same on the CSR of tril(A) (the diagonal is the last entry of every row; the upper triangle is never read,
 * symmetry is not checked):
 *     l_ik = (a_ik - sum_{j<k, j in cols(i) and cols(k)} l_ij * l_kj) / l_kk      for k in cols(i), k < i, ascending
 *     l_ii = sqrt(a_ii * (1 + shift) - sum_{j<i} l_ij^2)
 * The sums run in an order that depends on the two rows only (per lane in ascending order of row k's entries, then a fixed
 * butterfly over the 64 lanes): two calls give the same bits, whatever the grid.
 *
 * Breakdown — ILU: a row whose own pivot out[i,i] is zero; IC: a radicand that is not positive (NaN included) — never stops a
 * row: it is finished with IEEE arithmetic (inf / NaN) and handed on like any other.  info[0] (device, int64) is 0 after a clean
 * factorisation and 1 + (the lowest such row) otherwise.
 *
 * work: tsgu_csr_factor_work_bytes(n) bytes, 16-byte aligned, re-initialised by every call (one memset on the stream).  Its first
 * 32-bit word is the error word: a dependency that does not arrive within 4 s sets it, every wave then leaves, the call has
 * returned long before, and `out` is not valid — a caller that cannot rule that out reads the word after the stream has drained
 * (TSGU_ERR_TIMEOUT is its meaning).  `workgroups_per_cu` (1 … 8): persistent workgroups per compute unit; speed only.
 *
 * out == val is allowed (in-place factorisation): row i of val is read by the wave that owns row i only, before it writes row i.
 */
#ifndef TSGU_HIP_FACTOR_H
#define TSGU_HIP_FACTOR_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the work buffer of a factorisation of n rows.  Host only. */
int64_t tsgu_csr_factor_work_bytes(int64_t n);

/* For callers that size test cases.  Host only.
 *   row_capacity      entries of a row that are staged in LDS; a longer row is built in `out` itself
 *   waves_per_block   waves (= rows in flight) of a workgroup */
int tsgu_csr_factor_geometry(int vtype, int* row_capacity, int* waves_per_block);

int tsgu_csr_ilu0(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* diag_pos,
                  const void* val, double shift, void* out, void* work, int64_t* info, int workgroups_per_cu, int device,
                  void* stream);

int tsgu_csr_ic0(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* diag_pos,
                 const void* val, double shift, void* out, void* work, int64_t* info, int workgroups_per_cu, int device,
                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_FACTOR_H */
