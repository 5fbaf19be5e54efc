/*
 * tsgu_hip_selinv.h — Takahashi selected inversion: the entries of (L·Lᵀ)⁻¹ or ((L+I)·D·(L+I)ᵀ)⁻¹ on the pattern of the lower
 * factor L (sparse_selinv.py): entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * L is given by its COLUMNS: `colptr` [n + 1], `rowidx` [nnz] ascending and unique within a column and never above the diagonal,
 * `perm` [nnz] the position of every CSC entry in the value array `val` (NULL: `val` is in CSC order), all of `itype`.  The caller's
 * plan has checked that; the kernel never reads through an entry outside [0, n) or a position outside [0, nnz) whatever the arrays hold.
 * The pattern must be closed under elimination (for every column, every pair of rows stored below the diagonal is a stored
 * position): a lookup that misses contributes a zero and is reported, nothing stalls.
 */
#ifndef TSGU_HIP_SELINV_H
#define TSGU_HIP_SELINV_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: bytes of the work buffer (16-byte aligned) for n columns and nnz entries of `vtype`; 0 for arguments out of range. */
int64_t tsgu_csc_selinv_work_bytes(int vtype, int64_t n, int64_t nnz);

/* Host only: the sub-diagonal entries of a column that are staged in LDS for `vtype` (a longer column is built in the work
 * buffer itself) and the columns a workgroup has in flight. */
int tsgu_csc_selinv_geometry(int vtype, int* column_capacity, int* waves_per_block);

/* One persistent launch (plus the memset of the work buffer's head and a one-thread kernel that writes `info`).
 *   D == NULL   Q = L·Lᵀ; `diag_pos` [n] is the CSC position of every column's diagonal (its first entry); diag_out is ignored.
 *   D != NULL   Q = (L+I)·D·(L+I)ᵀ with L stored strictly lower; `diag_pos` is ignored; `diag_out` [n] receives diag(Q⁻¹).
 * out[perm[p]] = Q⁻¹[rowidx[p], column of p] for every stored position, in the value type; `out` may not alias `val`.
 * info[0] = 1 + the lowest column whose pivot (L_ii or D_i) is zero or not finite, info[1] = 1 + the lowest column one of whose
 * lookups missed (the pattern is not closed); 0 for none.  Both are written behind the launch on `stream`.
 * The order of every sum depends on the pattern only: two calls, and calls with different `workgroups_per_cu` (1 … 8), give the
 * same bits.  Byte 0 of `work` is an int32 that is non-zero afterwards when a bounded dependency wait expired. */
int tsgu_csc_selinv(int vtype, int itype, int64_t n, int64_t nnz, const void* colptr, const void* rowidx, const void* perm,
                    const void* diag_pos, const void* val, const void* D, void* out, void* diag_out, void* work, int64_t* info,
                    int workgroups_per_cu, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SELINV_H */
