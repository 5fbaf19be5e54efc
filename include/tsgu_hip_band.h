/*
 * tsgu_hip_band.h — triangular solves with a BANDED factor in logarithmic depth (sparse_banded_solve.py): entries of
 * libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * A is given by its CSR arrays (`ptr` [n + 1], `idx` [nnz], both of `itype`; `val` [nnz]) with strictly ascending columns per row.
 * `lower` selects the triangle of A that is used (entries on the other side are ignored; with `unit` the stored diagonal too and
 * the diagonal is 1); `transpose` solves with op(A) = Aᵀ, read from the same arrays.  `w` is at least the largest |row − col| on
 * the selected side and at most 8; an entry further out is ignored, never read through.  The caller's plan has checked all that.
 */
#ifndef TSGU_HIP_BAND_H
#define TSGU_HIP_BAND_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only: the rows of a chunk, the summaries of a carry group and the longest chain one workgroup walks, for a system of n rows,
 * p columns and width w of `vtype`: pure functions of these four.  `chunk_rows` / `group_chunks`: 0, or a caller's override (tests). */
int tsgu_csr_band_geometry(int vtype, int64_t n, int64_t p, int w, int chunk_rows, int group_chunks, int* rows, int* group, int* top);

/* Host only: bytes of the work buffer of the solve below; 0 for arguments out of range.  Nothing in it needs initialising. */
int64_t tsgu_csr_band_sptrsm_work_bytes(int vtype, int64_t n, int64_t p, int w, int chunk_rows, int group_chunks);

/* X = op(A)⁻¹ B: B [n, p] with row stride ldb, X [n, p] with row stride ldx, both of `vtype` with unit column stride; X may not
 * alias B.  A handful of plain launches (chunk reduce, carry levels up and down, chunk apply) on `stream`: no waits between
 * workgroups, no error word, safe to capture.  Every sum is formed in an order fixed by (n, p, w, vtype) and the overrides: two
 * calls give the same bits.  A row without a diagonal gives inf / NaN in that row and the rows that depend on it. */
int tsgu_csr_band_sptrsm(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* val, int w, int lower,
                         int unit, int transpose, const void* B, int64_t ldb, void* X, int64_t ldx, int64_t p, void* work,
                         int chunk_rows, int group_chunks, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_BAND_H */
