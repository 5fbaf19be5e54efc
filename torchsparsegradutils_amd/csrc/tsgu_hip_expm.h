/*
 * tsgu_hip_expm.h — the Chebyshev recurrence of sparse_expm_mm (sparse_expm.py): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_EXPM`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype, no synchronisation, no allocation, no atomics, no reductions).  The entries are
 * additive, so TSGU_ABI_VERSION stays as it is.  The reference has no counterpart: it has no matrix exponential.
 *
 * The method.  For a symmetric A with spectrum in [lo, hi], rho = (hi - lo) / 2, mid = (hi + lo) / 2, Ahat = a A + b I with
 * a = 1 / rho, b = -mid / rho:  exp(t A) B = sum_k c_k w_k,  w_0 = B,  w_1 = Ahat w_0,  w_{k+1} = 2 Ahat w_k - w_{k-1}, with
 * coefficients c_k the host computes from scaled modified Bessel functions.  One step is
 *   SpMM (the caller's, into `prod`) -> tsgu_cheb_step
 * and once per chunk of m steps tsgu_cheb_combine adds the chunk's terms to the T results (one per time).  The adjoint
 * recurrence mu_k = c_k G + f_k Ahat mu_{k+1} - mu_{k+2} runs on the same two entries: tsgu_cheb_combine (mode 1) writes the source
 * terms sum_j c_{k,j} G_j of m steps at once, tsgu_cheb_step adds them through `src`.
 *
 * Every launcher refuses on the host, before any launch: NULL pointers (except the optional ones named below), operands that are
 * not aligned (16 bytes for every value array but `coef`, the element size for `coef`, 4 for `flags`), n <= 0, p <= 0, slot counts below 1, a slot outside its array, a
 * `plane_stride` below n * p or not a multiple of 16 bytes, a mode or an `accumulate` outside {0, 1}, `accumulate` with mode 1,
 * a NULL `prod` with alpha != 0 (TSGU_ERR_BAD_ARG); value types other than TSGU_F32 and TSGU_F64 (TSGU_ERR_BAD_DTYPE; TSGU_BF16
 * included); slot counts above the chunk cap, T above the time cap and widths the lane geometry does not cover
 * (TSGU_ERR_TOO_LARGE): any p <= 256, wider in multiples of the 16-byte lane (4 float32 / 2 float64 columns) up to 256 lanes.
 */
#ifndef TSGU_HIP_EXPM_H
#define TSGU_HIP_EXPM_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  time_cap: the largest T of tsgu_cheb_combine; chunk_cap: the largest slot count of a chunk (both compile-time
 * constants, at least 8 and 16); plane_align: elements a `plane_stride` must be a multiple of (16 bytes of the value type);
 * rows_per_workgroup / workgroups: the walk of both launchers over an [n][p] array (nothing has to be sized by them). */
int tsgu_expm_geometry(int vtype, int64_t n, int64_t p, int* time_cap, int* chunk_cap, int* plane_align, int64_t* rows_per_workgroup,
                       int64_t* workgroups);

/* One step of a three-term recurrence, every row walked once.  Per element, in the value type, with alpha, beta and gamma cast
 * to it once:
 *   t0  = gamma * prev[i][c]                       (taken as 0, and prev is not read, when gamma == 0)
 *   t1  = fma(beta, x[i][c], -t0)
 *   t2  = fma(alpha, prod[i][c], t1)               (t2 = t1 when prod is NULL; alpha must then be 0)
 *   new = t2 + src[i][src_slot][c]                 (new = t2 when src is NULL)
 *   prev[i][c] = new;   chunk[i][slot][c] = new    when `chunk` is given
 * At most 3 roundings, 4 with src (2 and 3 without prod).
 *   prod, x, prev   [n][p] contiguous, 16-byte aligned; x and prod are inputs and may not overlap prev
 *   src             [n][src_slots][p] or NULL;  chunk  [n][chunk_slots][p] or NULL (row-major [n][slots * p]: an SDDMM operand);
 *                   src and chunk may be the same array and the same slot (an element is read before it is written)
 *   flags           int32: nothing at all is written when flags[0] != 0
 * w_0 enters a chunk as (prod NULL, alpha 0, beta 1, x = B, gamma 0); the last adjoint vector as (prod NULL, alpha 0, beta 0,
 * gamma 0, src).  A step with prod and a chunk moves five planes. */
int tsgu_cheb_step(int vtype, int64_t n, int64_t p, const void* prod, const void* x, void* prev, double alpha, double beta, double gamma,
                   const void* src, int src_slots, int src_slot, void* chunk, int chunk_slots, int slot, const int* flags, int device,
                   void* stream);

/* One chunk of m slots against T planes, every row walked once.
 *   chunk    [n][m][p];   coef  [m][T][p] in the value type;   planes  T arrays [n][p], `plane_stride` elements apart
 * mode 0 (emit), per time j:  t = coef[0][j][c] * chunk[i][0][c];  t = fma(coef[s][j][c], chunk[i][s][c], t) for s = 1 ... m - 1 in
 *   this order;  planes[j][i][c] = accumulate ? planes[j][i][c] + t : t.  m roundings, one more with accumulate.  The T sums stay in
 *   registers while the m slots are read once; chunk is an input.
 * mode 1 (spread), per slot s:  t = coef[s][0][c] * planes[0][i][c];  t = fma(coef[s][j][c], planes[j][i][c], t) for j = 1 ... T - 1
 *   in this order;  chunk[i][s][c] = t.  T roundings.  The T planes are read once; planes is an input; accumulate must be 0.
 *   flags    int32: nothing at all is written when flags[0] != 0
 * No partial sums, no reduction: the same bits on every run. */
int tsgu_cheb_combine(int vtype, int mode, int accumulate, int64_t n, int64_t p, int m, int T, void* chunk, const void* coef,
                      void* planes, int64_t plane_stride, const int* flags, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_EXPM_H */
