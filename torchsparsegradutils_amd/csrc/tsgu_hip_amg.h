/*
 * tsgu_hip_amg.h — the kernels of the aggregation multigrid preconditioner (sparse_amg): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_AMG`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream`
 * last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION
 * stays as it is.  The reference has no counterpart.
 *
 * Patterns are CSR: a row pointer of n + 1 words and nnz column indices of one index type (TSGU_I32 or TSGU_I64).  Keys are
 * unsigned 64-bit words, `state << 62 | priority << 32 | index` with state 2 = root, 1 = undecided, 0 = removed.  Dense operands
 * of the product are TSGU_F32 or TSGU_F64 (TSGU_BF16 is TSGU_ERR_BAD_DTYPE), row-major [rows][p] with a leading dimension
 * ld >= p in elements.  Device pointers are aligned to their element.
 *
 * Determinism: no float atomics.  The hop is a max, exact in any order: its result does not depend on `group` or on the grid.  An
 * element of the product is summed in an order that depends on its row and on p alone: two runs give the same bits.
 *
 * Every launcher refuses on the host, before any launch: NULL or misaligned pointers and negative sizes (TSGU_ERR_BAD_ARG),
 * unknown types (TSGU_ERR_BAD_DTYPE), ld < p (TSGU_ERR_BAD_ARG), more than 2^31 - 1 nodes or 65535 column tiles
 * (TSGU_ERR_TOO_LARGE).  No kernel depends on values to stay in bounds: row extents are clamped to nnz and an entry whose column
 * is outside the matrix is skipped.
 */
#ifndef TSGU_HIP_AMG_H
#define TSGU_HIP_AMG_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  The lane groups tsgu_csr_amg_hop accepts are the powers of two min_group … max_group; column_tile is the number of
 * columns one workgroup of tsgu_csr_affine_spmm covers (speed only: any p is accepted). */
int tsgu_amg_geometry(int* min_group, int* max_group, int* column_tile);

/* out[i] = max(in[i], max over the stored entries (i, j) of in[j]) for i < n.  `group` lanes own a row (speed only).  `in` and
 * `out` may not overlap (TSGU_ERR_BAD_ARG).  idx may be NULL when nnz = 0. */
int tsgu_csr_amg_hop(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* in, void* out, int group,
                     int device, void* stream);

/* One node-wise step of the MIS-2 aggregation on n keys.
 *   mode 0   out[i] = the initial key of node i: undecided, priority lowbias32(i) >> 2 (key, t and undecided are not read)
 *   mode 1   with t = hop(hop(key)): an undecided node whose t carries its own index becomes a root, otherwise an undecided node
 *            whose t has state 2 is removed; out[i] = the next key.  *undecided (a device word the caller zeroed) is set to a
 *            non-zero value when a node is still undecided afterwards.  out may be key.
 *   mode 2   out[i] = key[i] for roots, 0 otherwise (t and undecided are not read). */
int tsgu_amg_mis2_update(int mode, int64_t n, const void* key, const void* t, void* out, void* undecided, int device, void* stream);

/* out[n_rows][p] = c + alpha · w ∘ (b − A·x) for the CSR matrix A (n_rows x n_cols; ptr, idx, val) and x [n_cols][p].  c, b
 * ([n_rows][p]) and w ([n_rows], one weight per row) are optional: NULL stands for 0, 0 and 1.  The epilogue is row-local: out
 * may be c or b (the same pointer and leading dimension); any other overlap of out with c or b, and any overlap of out with x,
 * is TSGU_ERR_BAD_ARG, decided by address ranges.  idx and val may be NULL when nnz = 0. */
int tsgu_csr_affine_spmm(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t p, const void* ptr, const void* idx,
                         const void* val, const void* x, int64_t ldx, const void* c, int64_t ldc, const void* b, int64_t ldb,
                         const void* w, double alpha, void* out, int64_t ldo, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_AMG_H */
