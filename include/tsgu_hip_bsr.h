/*
 * tsgu_hip_bsr.h — block-sparse (BSR) × dense products on the matrix cores: entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, leading dimensions in elements, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * A is n_block_rows × n_block_cols blocks of bh × bw elements; (ptr[n_block_rows + 1], idx[nnzb]) is the CSR pattern of the block
 * matrix and val holds the stored blocks in that order, each packed row-major (bh·bw elements).  Every stored block is a term: the
 * blocks of a block row are summed in stored order, column indices need not be sorted, a repeated (I, J) is two terms, a stored
 * zero block stays a term and a block row without blocks gives zeros.
 *
 *   tsgu_bsr_spmm     C[I·bh + r, :]  = sum_{e in block row I}    val[e][r, :] · B[idx[e]·bw : +bw, :]
 *   tsgu_bsr_sddmm    dval[e]         = G[I_e·bh : +bh, :] · B[idx[e]·bw : +bw, :]ᵀ                       (K = p)
 *   tsgu_bsr_spmm_t   dB[J·bw + c, :] = sum_{e in block column J} val[perm[e]][:, c]ᵀ · G[tidx[e]·bh : +bh, :]
 *
 * The products run on MFMA tiles of 16 × 16 with zero padding inside the tiles, so every bh, bw >= 1 is served; blocks whose sides
 * are multiples of 16 waste none of it.  Accumulation is in float for TSGU_F32 and TSGU_BF16 (bf16 products are exact, the result is
 * rounded once when stored) and in double for TSGU_F64.  Deterministic: no float atomics, and the summation order of an output
 * element depends on its own block row (block column) only.
 *
 * Dense operands are row-major with a row stride (ld*, in elements) >= p, 1 <= p.  16-byte accesses are used where an address
 * allows them and single elements elsewhere: alignment is never a reason for a refusal beyond whole elements.  nnzb·bh·bw,
 * n_block_rows·bh and n_block_cols·bw stay below 2^31, strides below 2^32 (TSGU_ERR_TOO_LARGE beyond).
 *
 * Host-side refusals, in this order, before any HIP call: null pointers (idx, val and the gathered dense operand may be null when
 * nnzb == 0), the value / index type, p < 1, bh < 1, bw < 1 or a negative count, a leading dimension below p or a dense pointer
 * that is not a whole number of elements, the size limits.  A call with nothing to compute returns TSGU_OK without touching a device.
 */
#ifndef TSGU_HIP_BSR_H
#define TSGU_HIP_BSR_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch geometry of blocks of bh × bw elements of `vtype` against p dense columns, for callers that size test cases.  Host only.
 *   tile_rows   rows of the result one workgroup computes: whole block rows while bh <= tile_rows (tile_rows / bh of them), else a
 *               piece of tile_rows rows of one block row
 *   tile_cols   columns of the p one workgroup computes
 *   k_stage     elements along the summed dimension per LDS stage: a block row's blocks are concatenated until a stage is full */
int tsgu_bsr_mm_geometry(int vtype, int64_t bh, int64_t bw, int64_t p, int* tile_rows, int* tile_cols, int* k_stage);

/* Forward: writes C[n_block_rows·bh, p]. */
int tsgu_bsr_spmm(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                  const void* ptr, const void* idx, const void* val, const void* B, int64_t ldb, int64_t p, void* C, int64_t ldc,
                  int device, void* stream);

/* Gradient of the values: writes all of dval[nnzb·bh·bw] from G[n_block_rows·bh, p] and B[n_block_cols·bw, p]. */
int tsgu_bsr_sddmm(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                   const void* ptr, const void* idx, const void* G, int64_t ldg, const void* B, int64_t ldb, int64_t p, void* dval,
                   int device, void* stream);

/* Gradient of B: (tptr[n_block_cols + 1], tidx = block row of every block, perm = its position in val) is the transposed walk of
 * the same block pattern.  Writes dB[n_block_cols·bw, p]. */
int tsgu_bsr_spmm_t(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                    const void* tptr, const void* tidx, const void* perm, const void* val, const void* G, int64_t ldg, int64_t p,
                    void* dB, int64_t lddb, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_BSR_H */
