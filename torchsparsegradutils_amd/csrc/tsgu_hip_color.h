/*
 * tsgu_hip_color.h — the kernels of the multicolour ordering (sparse_coloring, and the coloured forms of sparse_ilu0, sparse_ic0 and
 * sparse_sgs): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_COLOR`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream`
 * last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION
 * stays as it is.  The reference has no counterpart.
 *
 * Patterns are CSR: a row pointer of n + 1 words and nnz column indices of one index type (TSGU_I32 or TSGU_I64).  The transposed
 * pattern (tptr, tidx; nnz_t entries) is that of Aᵀ; both pointers NULL stand for a structurally symmetric pattern.  The
 * neighbours of node i are the j != i with (i, j) or (j, i) stored.  Colours are 32-bit signed integers, -1 = uncoloured.  Dense
 * operands of the sweep are TSGU_F32 or TSGU_F64 (TSGU_BF16 is TSGU_ERR_BAD_DTYPE), row-major [rows][p] with a leading dimension
 * ld >= p in elements.  Device pointers are aligned to their element.
 *
 * Determinism: the colouring is a pure function of the pattern — node i has the key (lowbias32(i), i), the nodes are visited in
 * descending key and each takes the smallest colour no coloured neighbour holds; the rounds below reach exactly that result for
 * every `group` and every grid.  An element of the sweep is summed in an order that depends on its row and on p alone: two runs,
 * and every accepted `group`, give the same bits.  No float atomics.
 *
 * Every launcher refuses on the host, before any launch: NULL or misaligned pointers and negative sizes (TSGU_ERR_BAD_ARG),
 * unknown types (TSGU_ERR_BAD_DTYPE), ld < p (TSGU_ERR_BAD_ARG), more than 2^31 - 1 nodes or 65535 column tiles
 * (TSGU_ERR_TOO_LARGE).  No kernel depends on values to stay in bounds: row extents are clamped to nnz, an entry whose column is
 * outside the matrix is skipped, and a row whose mapped indices are outside their arrays is not written.
 */
#ifndef TSGU_HIP_COLOR_H
#define TSGU_HIP_COLOR_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  The lane groups of tsgu_csr_color_round / tsgu_csr_color_check are the powers of two min_group … max_group, those of
 * tsgu_csr_color_sweep the powers of two sweep_min_group … sweep_max_group; `window` is the number of colours one pass over a row
 * examines, column_tile the columns a group of sweep_min_group lanes covers (speed only: any p is accepted). */
int tsgu_color_geometry(int* min_group, int* max_group, int* window, int* sweep_min_group, int* sweep_max_group, int* column_tile);

/* One round of the colouring: out[i] = in[i] for a coloured node; an uncoloured node with no uncoloured neighbour of greater key
 * takes the smallest colour none of its neighbours holds in `in`, every other uncoloured node stays -1 and sets *undecided (a
 * device word of 64 bits the caller zeroed) to a non-zero value.  `in` and `out` (n colours each) may not overlap.  Starting from
 * all -1, at most n rounds colour every node.  idx may be NULL when nnz = 0, tidx when nnz_t = 0. */
int tsgu_csr_color_round(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, int64_t nnz_t, const void* tptr,
                         const void* tidx, const void* in, void* out, void* undecided, int group, int device, void* stream);

/* *first (a device word of 64 bits, written by the call) = 0 when `colors` is a colouring with n_colors colours, else 1 + the lowest
 * row whose colour is outside [0, n_colors) or is held by one of its neighbours. */
int tsgu_csr_color_check(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, int64_t nnz_t, const void* tptr,
                         const void* tidx, const void* colors, int64_t n_colors, void* first, int group, int device, void* stream);

/* The rows [row0, row1) of one colour class of a triangular sweep over a matrix of n rows, p right-hand sides, in ONE launch:
 *
 *     s = b[bmap(i)] − Σ_{e in [begin[i], end[i])} val[vmap(e)] · x[idx[e]]
 *     mode 0   x[i] = s / val[vmap(diag[i])]
 *     mode 1   x[i] = s                                        (unit diagonal: diag is not read and may be NULL)
 *     mode 2   x[i] = b[bmap(i)] − Σ / val[vmap(diag[i])]      (the right-hand side is scaled by the diagonal)
 *     and, when out is given, also out[out_rows(i)] = x[i]
 *
 * begin, end and diag are arrays of n positions into idx (nnz entries); vmap (nnz words), bmap and out_rows (n words) are
 * optional, NULL is the identity.  val has n_val elements; b, x and out have n rows.  The caller guarantees that no entry of the
 * class refers to a row of the class: x is updated in place.  b may be x itself (the same pointer and leading dimension, bmap
 * NULL); any other overlap of x with b or out is TSGU_ERR_BAD_ARG, decided by address ranges.  `group` lanes own a row (speed only).
 * idx and val may be NULL when nnz = 0. */
int tsgu_csr_color_sweep(int vtype, int itype, int mode, int64_t n, int64_t nnz, int64_t n_val, int64_t row0, int64_t row1, int64_t p,
                         const void* begin, const void* end, const void* idx, const void* diag, const void* vmap, const void* val,
                         const void* b, int64_t ldb, const void* bmap, void* x, int64_t ldx, void* out, int64_t ldo,
                         const void* out_rows, int group, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_COLOR_H */
