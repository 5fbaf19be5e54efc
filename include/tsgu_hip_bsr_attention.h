/*
 * tsgu_hip_bsr_attention.h — block-sparse attention on the matrix cores: entries of libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, leading dimensions in elements, `device` +
 * `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no allocation).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 *   O[i,h,:] = sum_j P[i,j,h] * V[j,h,:],   P[i,.,h] = softmax over the j that row i's stored blocks cover of
 *                                                      scale * <Q[i,h,:], K[j,h,:]> + bias[i,j]
 *
 * The mask is the BSR pattern of tsgu_hip_bsr.h: n_block_rows × n_block_cols blocks of bh × bw elements, (ptr[n_block_rows + 1],
 * idx[nnzb]) the CSR pattern of the block matrix, bias (NULL: none) the stored blocks in that order, each packed row-major.  Block
 * columns need not be sorted, a stored zero block stays stored, a repeated (I, J) is two sets of entries (its keys appear twice in
 * the row's softmax, and each block has its own dA) and a block row without blocks gives O = 0, lse = -inf and zero gradients.  A
 * row whose logits hold a NaN or a +inf, or nothing but -inf, gives NaN (O and lse) for that head; -inf beside finite logits has
 * weight 0 and gradient 0.
 *
 * Dense operands are [rows, heads * d] with a row stride (ld*, in elements) >= heads * d; every base pointer and every row stride
 * is a multiple of 16 bytes.  Supported (tsgu_bsr_attention_supported): bh and bw multiples of 16, d in {16, 32, 64, 128},
 * heads >= 1.  n_block_rows·bh, n_block_cols·bw and nnzb·bh·bw stay below 2^31, strides below 2^32 (TSGU_ERR_TOO_LARGE beyond).
 * `lse`, `delta`, `dA` and `O_acc` are of the ACCUMULATOR type: float for TSGU_F32 and TSGU_BF16, double for TSGU_F64.  `O_acc` is
 * the forward's result as the row pass reads it for delta = <dO, O>: O itself for TSGU_F32 and TSGU_F64, the copy the forward
 * writes before rounding for TSGU_BF16.  TSGU_F32 and TSGU_F64 multiply and accumulate in their own type.  TSGU_BF16 runs all five
 * products on the bf16 MFMA with float accumulation: P enters P·V and Pᵀ·dO as two bf16 terms (its rounded value and the rounded
 * remainder), dS is rounded to bf16 for dS·K and dSᵀ·Q (unlike tsgu_hip_attention.h, whose bf16 is the float path rounded once);
 * results are rounded once when stored and the caller rounds dA.
 *
 * Deterministic: no float atomics, no nnz·heads-sized intermediate (the backward recomputes the probabilities from lse), every sum
 * in an order that depends on the element's own block row (block column) only, and no workgroup waits for another.
 *
 * Host-side refusals, in this order, before any HIP call: null pointers (idx and the gathered dense operands may be null when
 * nnzb == 0; bias and dA may always be), the value / index type, a negative count or a geometry that is not supported, a leading
 * dimension below heads * d or a dense pointer / row stride that is not a multiple of 16 bytes, the size limits.  A call with
 * nothing to compute returns TSGU_OK without touching a device.
 */
#ifndef TSGU_HIP_BSR_ATTENTION_H
#define TSGU_HIP_BSR_ATTENTION_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the kernels take (vtype, heads, d) over blocks of bh × bw elements, else 0.  Host only. */
int tsgu_bsr_attention_supported(int vtype, int heads, int d, int64_t bh, int64_t bw);

/* The launch geometry of (vtype, heads, d, bh, bw), for callers that size test cases.  Host only.
 *   tile_rows    rows (column pass: keys) one workgroup owns: whole block rows while bh <= tile_rows (tile_rows / bh of them), else
 *                a piece of tile_rows rows of one block row
 *   stage_keys   keys (column pass: rows) per LDS stage: a block row's blocks are concatenated until a stage is full */
int tsgu_bsr_attention_geometry(int vtype, int heads, int d, int64_t bh, int64_t bw, int* tile_rows, int* stage_keys);

/* Forward: writes O[n_block_rows·bh, heads*d], lse[n_block_rows·bh, heads] and, when O_acc is not NULL, the result before it is
 * rounded to vtype: O_acc[n_block_rows·bh, heads*d] packed, in the accumulator type (what the row pass takes for TSGU_BF16). */
int tsgu_bsr_attention(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                       const void* ptr, const void* idx, const void* bias, const void* Q, int64_t ldq, const void* K, int64_t ldk,
                       const void* V, int64_t ldv, int heads, int d, double scale, void* O, int64_t ldo, void* lse, void* O_acc,
                       int device, void* stream);

/* Backward over the block rows (the forward's walk): writes dQ, delta[n_block_rows·bh, heads] = <dO, O> (for the column pass) and,
 * when dA is not NULL, dA[nnzb·bh·bw] = sum_h dS for every stored element. */
int tsgu_bsr_attention_backward_rows(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh,
                                     int64_t bw, const void* ptr, const void* idx, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* O_acc, int64_t ldo, const void* lse, int heads, int d, double scale, void* dQ,
                                     int64_t lddq, void* delta, void* dA, int device, void* stream);

/* Backward over the block columns: (tptr[n_block_cols + 1], tidx = block row of every block, perm = its position in bias) is the
 * transposed walk of the same block pattern.  Reads the forward's lse and the row pass's delta, so it runs after the row pass on
 * the same stream.  Writes dK and dV [n_block_cols·bw, heads*d]. */
int tsgu_bsr_attention_backward_cols(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh,
                                     int64_t bw, const void* tptr, const void* tidx, const void* perm, const void* bias,
                                     const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                     const void* dO, int64_t lddo, const void* lse, const void* delta, int heads, int d,
                                     double scale, void* dK, int64_t lddk, void* dV, int64_t lddv, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_BSR_ATTENTION_H */
