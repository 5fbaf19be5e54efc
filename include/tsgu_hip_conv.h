/*
 * tsgu_hip_conv.h — neighbor_mm, sparse convolution as an implicit GEMM on the matrix cores (sparse_conv.py): entries of
 * libtsgu_hip.so.
 *
 * An addition to the C ABI of tsgu_hip.h with the conventions stated in tsgu_hip_semiring.h (device
 * pointers, leading dimensions in elements, `device` + `stream` last, status codes, tsgu_vtype / tsgu_itype, no synchronisation, no
 * allocation, no global atomics, graph-capturable).  The entries are additive, so TSGU_ABI_VERSION stays as it is.  The reference
 * has no counterpart.
 *
 *   out[i][:] = bias[:] + sum_k x[nbr[i][k]][:] @ w[k][:][:]            i < n_out, k < K
 *
 * `nbr` is an (n_out, K) row-major table of int32 or int64; an entry outside [0, n_in) is an absent neighbour and adds nothing (the
 * kernels never read x through it).  x is (n_in, d1) with row stride ldx, out (n_out, d2) with row stride ldo, w (K, d1, d2) read
 * through its three strides, of which w_stride1 or w_stride2 is 1.  TSGU_F32, TSGU_F64 and TSGU_BF16; bf16 accumulates in float
 * and is rounded once.  16-byte loads are used where addresses allow; nothing has to be aligned.  Deterministic: every sum has one
 * fixed order, which depends on the shapes only.
 */
#ifndef TSGU_HIP_CONV_H
#define TSGU_HIP_CONV_H

#include "tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch geometry of (vtype, n_out, k, d1, d2), for callers that size the workspace and test cases.  Host only.
 *   tile_rows        rows of `out` one forward workgroup owns
 *   chunk_rows       rows one grad_w workgroup sums
 *   chunks           ceil(n_out / chunk_rows), at least 1: the partial sums folded into every element of grad_w
 *   workspace_bytes  bytes of the grad_w workspace (chunks * k * d1 * d2 accumulator elements when chunks > 1; never below 16) */
int tsgu_neighbor_mm_geometry(int vtype, int64_t n_out, int64_t k, int64_t d1, int64_t d2, int64_t* tile_rows, int64_t* chunk_rows,
                              int64_t* chunks, int64_t* workspace_bytes);

/* Forward: writes out[n_out, d2].  bias[d2] may be NULL.  n_out = 0 or d2 = 0: nothing to do; k = 0, d1 = 0 or n_in = 0 (a
 * bias-only result) is the caller's to write and is refused.  The gradient of x is this entry on the inverse table with w's
 * transposed view (w_stride1 and w_stride2 exchanged). */
int tsgu_neighbor_mm(int vtype, int itype, int64_t n_in, int64_t n_out, int64_t k, int64_t d1, int64_t d2, const void* nbr,
                     const void* x, int64_t ldx, const void* w, int64_t w_stride0, int64_t w_stride1, int64_t w_stride2,
                     const void* bias, void* out, int64_t ldo, int device, void* stream);

/* grad_w[k][c1][c2] = sum_i x[nbr[i][k]][c1] * g[i][c2], contiguous (k, d1, d2); g is (n_out, d2) with row stride ldg.  The
 * workspace (workspace_bytes from tsgu_neighbor_mm_geometry) is read and written when chunks > 1 only. */
int tsgu_neighbor_mm_grad_w(int vtype, int itype, int64_t n_in, int64_t n_out, int64_t k, int64_t d1, int64_t d2, const void* nbr,
                            const void* x, int64_t ldx, const void* g, int64_t ldg, void* grad_w, void* workspace,
                            int64_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_CONV_H */
