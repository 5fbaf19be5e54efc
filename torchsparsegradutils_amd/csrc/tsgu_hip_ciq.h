/*
 * tsgu_hip_ciq.h — the contour-quadrature update of sparse_inv_sqrt_mm / sparse_sqrt_mm (sparse_sqrt.py): entries of
 * libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_CIQ`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype, no synchronisation, no allocation, no atomics on values).  The entries are additive, so
 * TSGU_ABI_VERSION stays as it is.  The reference has no counterpart: it copied multi-shift MINRES and dropped the caller.
 *
 * The method.  A^(-1/2) B ~ sum_q omega_q (A + sigma_q I)^(-1) B over S shifts (Hale, Higham, Trefethen 2008, method 3): multi-shift
 * MINRES on shared Lanczos vectors, of which only the weighted sum of the S solutions is wanted.  One iteration is
 *   SpMM (+ <z, A z> partials) -> tsgu_minres_scalar_ms(phase 0) -> tsgu_minres_vector_ms(which = 0) -> tsgu_minres_scalar_ms(phase 1)
 *   -> tsgu_ciq_update -> tsgu_ciq_stop
 * with the scal [S][12][p] layout of tsgu_minres_scalar_ms (include/tsgu_hip.h): row 1 beta_c, row 6 scale_c (after phase 1:
 * MINRES's estimate of |r_q| for the normalised right-hand side, up to sign), rows 7 ... 10 sub, subsub, diag and the scale of
 * this update.  The two entries below replace tsgu_minres_vector_ms(which = 1) and tsgu_minres_scalar_ms(phase 2).
 *
 * Every launcher refuses on the host, before any launch: NULL pointers (except `keep`), operands that are not aligned (16 bytes for
 * the [n][p] arrays and `keep`, the element size for the others), n <= 0, p <= 0, n_shift < 1, a `shift_stride` below n * p or not
 * a multiple of 16 bytes (TSGU_ERR_BAD_ARG); value types other than TSGU_F32 and TSGU_F64 (TSGU_ERR_BAD_DTYPE; TSGU_BF16 included);
 * n_shift above the cap and widths the lane geometry does not cover (TSGU_ERR_TOO_LARGE): any p <= 256, wider in multiples of the
 * 16-byte lane (4 float32 / 2 float64 columns) up to 256 lanes.
 */
#ifndef TSGU_HIP_CIQ_H
#define TSGU_HIP_CIQ_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  shift_cap: the largest n_shift of the two launchers (a compile-time constant, at least 32); plane_align: elements a
 * `shift_stride` must be a multiple of (16 bytes of the value type); rows_per_workgroup / workgroups: the walk of tsgu_ciq_update
 * over an [n][p] array (nothing has to be sized by them: the update writes no partial sums). */
int tsgu_ciq_geometry(int vtype, int64_t n, int64_t p, int* shift_cap, int* plane_align, int64_t* rows_per_workgroup,
                      int64_t* workgroups);

/* One update of the weighted sum, every row walked once.  With beta_c = scal[0][1][c] and, per shift q, sub, subsub, diag, scale =
 * scal[q][7 ... 10][c]:
 *   zc[i][c] /= beta_c                                    (in place, every column)
 *   for q = 0 ... n_shift - 1, in this order:
 *     w_c = ((zp[i][c] - sub * wp[q][i][c]) - subsub * wpp[q][i][c]) / diag      written over wpp[q][i][c]
 *     up  = w_c * scale;     t = fma(omega[q], up, t)     (t starts at 0);     keep[i][q][c] += up   when `keep` is given
 *   acc[i][c] += t
 *   zc, zp, acc   [n][p] contiguous, 16-byte aligned; zp is z one step back (q_prev of MINRES without a preconditioner)
 *   wpp, wp       n_shift planes [n][p], `shift_stride` elements apart
 *   keep          [n][n_shift][p] (row-major [n][n_shift * p]: the per-shift solutions, as an SDDMM operand) or NULL
 *   omega         [n_shift] in the value type
 *   done          [p] int32: a column with done[c] != 0 keeps every bit of acc, keep and wpp (its zc is still normalised)
 *   flags         int32: nothing at all is written when flags[0] != 0
 * No partial sums, no reduction: the same bits on every run. */
int tsgu_ciq_update(int vtype, int64_t n, int64_t p, int n_shift, void* zc, const void* zp, void* wpp, const void* wp,
                    int64_t shift_stride, void* acc, void* keep, const void* scal, const void* omega, const int* done, const int* flags,
                    int device, void* stream);

/* The stop rule on MINRES's own residual estimates, one workgroup, after tsgu_minres_scalar_ms(phase 1):
 *   est[c]  = max over q of |scal[q][6][c]|   (NaN when one of them is NaN)
 *   done[c] = done[c] != 0 or est[c] <= tol   (sticky; NaN compares false)
 *   flags[0] = 1 when every column is done
 * Nothing is written when flags[0] != 0 on entry.  est [p] in the value type, done [p] int32. */
int tsgu_ciq_stop(int vtype, int64_t p, int n_shift, const void* scal, double tol, void* est, int* done, int* flags, int device,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_CIQ_H */
