/*
 * tsgu_hip_spgemm.h — sparse × sparse products C = A·B over CSR arrays: entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream` last, status codes,
 * tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it is.
 * The reference has no counterpart; torch.sparse.mm(S1, S2) has these semantics.
 *
 * A is [n_rows, n_inner], B is [n_inner, n_cols], C is [n_rows, n_cols]; (x_ptr[rows + 1], x_idx[nnz], x_val[nnz]) are CSR
 * arrays whose index type is `itype` for all three matrices.  n_cols < 2^31.  The columns of a row of B must be distinct (they
 * need not be sorted); the rows of A may be in any order.  C's pattern is the structural product: (i, j) is stored when some
 * A[i,k] and B[k,j] are both stored, whatever their values; its columns are ascending within every row.
 *
 * The work is launched per BIN of rows.  A caller sorts the rows by a per-row measure x into
 *     bin 0: 1 <= x <= limits[0]     bin 1: <= limits[1]     bin 2: <= limits[2]     bin 3: above
 * (rows with x = 0 belong to no bin) and hands every launch the int32 list of its rows.  For the symbolic launches x is the
 * upper bound ub[i] = sum over the stored A[i,k] of nnz(B[k,:]) (tsgu_spgemm_row_bound), for the numeric launch it is the
 * row's length in C.  Bins 0..2 keep the row in LDS; bin 3 works in global memory: the symbolic launches sort, for row g of the
 * list, the int32 slice scratch[sptr[g] .. sptr[g + 1]) whose length must be a power of two, at least ub and at least 8192;
 * the numeric launch accumulates in acc[nnz(C)] (accumulator type: float for TSGU_F32 and TSGU_BF16, double for TSGU_F64;
 * for TSGU_F32 / TSGU_F64 it may be c_val itself).
 *
 * Every output entry is summed in A's stored order, every gradient entry in the stored order of the side it walks, by plain
 * adds in the accumulator type (bf16 is rounded once): deterministic, no float atomics.  No workgroup waits on another.
 */
#ifndef TSGU_HIP_SPGEMM_H
#define TSGU_HIP_SPGEMM_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* limits[3]: the largest measure of the three LDS bins; lanes[4]: the lanes that own one row in each of the four bins.  Host only. */
int tsgu_spgemm_bins(int* limits, int* lanes);

/* ub[n_rows] (int64). */
int tsgu_spgemm_row_bound(int itype, int64_t n_rows, int64_t n_inner, const void* a_ptr, const void* a_idx, const void* b_ptr,
                          int64_t* ub, int device, void* stream);

/* One bin of the symbolic phase over rows[n_bin].  fill = 0: cnt[row] (int64) = distinct columns of the row.  fill = 1: with
 * c_ptr[n_rows + 1] known, the ascending columns go to c_idx[c_ptr[row] ..); nothing is written beyond the row's length. */
int tsgu_spgemm_symbolic(int itype, int bin, int64_t n_bin, const int* rows, int64_t n_rows, int64_t n_inner, int64_t n_cols,
                         const void* a_ptr, const void* a_idx, const void* b_ptr, const void* b_idx, int* scratch,
                         const int64_t* sptr, int fill, int64_t* cnt, const void* c_ptr, void* c_idx, int device, void* stream);

/* One bin of the numeric phase over rows[n_bin]: writes c_val at the rows' entries. */
int tsgu_spgemm_numeric(int vtype, int itype, int bin, int64_t n_bin, const int* rows, int64_t n_rows, int64_t n_inner,
                        int64_t n_cols, const void* a_ptr, const void* a_idx, const void* a_val, const void* b_ptr,
                        const void* b_idx, const void* b_val, const void* c_ptr, const void* c_idx, void* acc, void* c_val,
                        int device, void* stream);

/* grad_a[e] = sum over the entries t of row a_idx[e] of B of g[position in C of (a_row[e], b_idx[t])] * b_val[t], for the nnz_a
 * stored entries of A; g[nnz(C)] is the upstream gradient on C's pattern. */
int tsgu_spgemm_grad_a(int vtype, int itype, int64_t n_rows, int64_t n_inner, int64_t n_cols, int64_t nnz_a, const void* a_row,
                       const void* a_idx, const void* b_ptr, const void* b_idx, const void* b_val, const void* c_ptr,
                       const void* c_idx, const void* g, void* grad_a, int device, void* stream);

/* grad_b[t] = sum over the entries u of row b_row[t] of A's transposed pattern (t_ptr[n_inner + 1], t_idx = row in A, t_perm =
 * position in a_val) of a_val[t_perm[u]] * g[position in C of (t_idx[u], b_idx[t])], for the nnz_b stored entries of B. */
int tsgu_spgemm_grad_b(int vtype, int itype, int64_t n_rows, int64_t n_inner, int64_t n_cols, int64_t nnz_b, const void* b_row,
                       const void* b_idx, const void* t_ptr, const void* t_idx, const void* t_perm, const void* a_val,
                       const void* c_ptr, const void* c_idx, const void* g, void* grad_b, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SPGEMM_H */
