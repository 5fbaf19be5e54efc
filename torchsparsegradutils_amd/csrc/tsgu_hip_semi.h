/*
 * tsgu_hip_semi.h — 2:4 semi-structured operands (sparse_semi_structured.py): prune, expand, A·Yᵀ, Aᵀ·G and the SDDMM on the kept
 * positions; entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_SEMI`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype, no synchronisation, no allocation, no global atomics).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart.
 *
 * THE OPERAND.  A is (m, k), k % 4 == 0, and keeps two of every four consecutive entries of a row (an aligned group):
 *   val   (m, k / 2) of the value type, row stride `ldv` elements: the kept entries of a row in column order (stored zeros fill a
 *         group with fewer than two non-zeros)
 *   meta  (m, ldm) of uint32, ldm >= 4 * ceil(k / 128), ldm % 4 == 0, 16-byte aligned: one nibble p0 | p1 << 2 per group with
 *         0 <= p0 < p1 <= 3, the kept positions inside the group.  Group g of a row (dense columns 4 g .. 4 g + 3) is found with
 *             stage = g / 32,  s = (g % 32) / 8,  q = (g % 8) / 2,  h = g % 2:   bits [8 s + 4 h, 8 s + 4 h + 4) of word 4 stage + q.
 *         (The 128 dense columns of one bf16 stage own four words; word q is the position register of the lanes of quarter q of
 *         v_smfmac_f32_16x16x32_bf16, byte s what `abid = s` selects in the s-th instruction of the stage.)  The groups past k
 *         hold the nibble 0x4.
 * Values are accumulated as the matrix-core tile layer does (fp32 for TSGU_F32 and TSGU_BF16, fp64 for TSGU_F64), in ascending
 * order of the summation index, and rounded once to the value type.  Dropped positions are not stored: a non-finite entry of a dense
 * operand that faces one is multiplied by zero on the expanding paths and never read by the sparse instruction.
 *
 * Every launcher refuses on the host, before the launch: NULL pointers, negative sizes, k % 4 != 0, a row stride below the row
 * length, pointers not aligned to their element, a `meta` that is not 16-byte aligned or whose ldm is no multiple of 4, flags
 * outside the entry's bits (TSGU_ERR_BAD_ARG); a value type other than the three (TSGU_ERR_BAD_DTYPE); a size at or above 2^31 - 1
 * or more workgroups than a grid holds (TSGU_ERR_TOO_LARGE).  A size of zero launches nothing unless a result has to be zeroed.
 */
#ifndef TSGU_HIP_SEMI_H
#define TSGU_HIP_SEMI_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TSGU_SEMI_DENSE_T 1   /* flags: the dense operand(s) are given transposed (see each entry) */
#define TSGU_SEMI_OUT_T 2     /* flags: the result is stored transposed */

/* Host only.  meta_words: 4 * ceil(k / 128), the least ldm; tile_rows / tile_cols: the result tile of a workgroup of tsgu_semi_mm;
 * stage_columns: the dense columns of one LDS stage of the value type; sparse_instruction: 1 when tsgu_semi_mm has the sparse
 * matrix instruction for the value type (TSGU_BF16).  TSGU_ERR_BAD_ARG for k < 0 or k % 4 != 0. */
int tsgu_semi_geometry(int vtype, int64_t k, int64_t* meta_words, int* tile_rows, int* tile_cols, int* stage_columns,
                       int* sparse_instruction);

/* val, meta = the 2:4 operand of W (m, k), row stride ldw: per group the two entries that rank first by (|w| descending, column
 * ascending); NaN ranks above inf, -0 equals +0.  The values are copied bit for bit.  Writes the first 4 * ceil(k / 128) words of
 * every row of meta. */
int tsgu_semi_prune(int vtype, const void* W, int64_t ldw, int64_t m, int64_t k, void* val, int64_t ldv, void* meta, int64_t ldm,
                    int device, void* stream);

/* out (m, k), row stride ldo = the dense matrix of the operand: the kept values at their positions, +0 elsewhere. */
int tsgu_semi_expand(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, int64_t m, int64_t k, void* out,
                     int64_t ldo, int device, void* stream);

/* C[i][n] = sum_c A[i][c] * Y[n][c] (+ bias[i]).  Y is (p, k), row stride ldy; with TSGU_SEMI_DENSE_T it is given as (k, p).  bias
 * is [m] or NULL, added in the accumulation type before the one rounding.  C is (m, p), row stride ldc; with TSGU_SEMI_OUT_T it is
 * stored as (p, m).  path = 1: the sparse matrix instruction (TSGU_BF16 only, else
 * TSGU_ERR_BAD_ARG); path = 0: A is expanded into a dense LDS image and multiplied by the dense instruction of the value type.
 * A·B for B (k, p): TSGU_SEMI_DENSE_T.  X·Aᵀ for X (p, k): TSGU_SEMI_OUT_T. */
int tsgu_semi_mm(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, const void* Y, int64_t ldy, const void* bias,
                 void* C, int64_t ldc, int64_t m, int64_t k, int64_t p, int flags, int path, int device, void* stream);

/* D[c][n] = sum_i A[i][c] * G[i][n].  G is (m, p), row stride ldg; with TSGU_SEMI_DENSE_T it is given as (p, m).  D is (k, p), row
 * stride ldd; with TSGU_SEMI_OUT_T it is stored as (p, k).  Reads the compressed bytes of A only. */
int tsgu_semi_mm_t(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, const void* G, int64_t ldg, void* D,
                   int64_t ldd, int64_t m, int64_t k, int64_t p, int flags, int device, void* stream);

/* out[i][s] = sum_n G[i][n] * Y[col(i, s)][n] for the kept positions only: out is (m, k / 2), row stride ldo.  G is (m, p) and Y
 * (k, p); with TSGU_SEMI_DENSE_T they are given as (p, m) and (p, k). */
int tsgu_semi_sddmm(int vtype, const void* G, int64_t ldg, const void* Y, int64_t ldy, const void* meta, int64_t ldm, void* out,
                    int64_t ldo, int64_t m, int64_t k, int64_t p, int flags, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_SEMI_H */
