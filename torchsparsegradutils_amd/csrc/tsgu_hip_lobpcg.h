/*
 * tsgu_hip_lobpcg.h — the tall-skinny dense kernels of the LOBPCG eigensolver: entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream`
 * last, status codes, tsgu_vtype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it
 * is.  The reference has no counterpart.
 *
 * Operands: TSGU_F32 and TSGU_F64 (TSGU_BF16 is TSGU_ERR_BAD_DTYPE).  Every dense operand is a row-major view [n][width] with a
 * leading dimension ld >= width, in elements; several views may interleave in one allocation (the blocks X, W, P of a basis
 * [n][3k] are three views with ld = 3k).  Device pointers are aligned to the element (4 or 8 bytes).  Widths: 1 … wmax (96) for the operands of the
 * Gram kernel, 1 … kmax (32) for the blocks of the other two.
 *
 * Determinism: the rows are cut into chunks of `rows_per_workgroup` consecutive rows, a property of n alone.  A sum over the rows
 * is formed per chunk in ascending row order, written to the workspace, and the chunks are added in ascending order by a fold
 * whose grouping depends on the chunk count alone: no float atomics, and the same inputs give the same bits for every
 * `workgroups` (0: the library's choice; speed only).  The workspace is scratch: nothing is kept in it between calls.
 *
 * Every launcher refuses on the host, before any launch: NULL or misaligned pointers and n <= 0 (TSGU_ERR_BAD_ARG), widths of 0
 * (TSGU_ERR_BAD_ARG) or above the limit (TSGU_ERR_TOO_LARGE), ld < width (TSGU_ERR_BAD_ARG), an unknown value type
 * (TSGU_ERR_BAD_DTYPE), a workspace that is too small (TSGU_ERR_BAD_ARG).  No kernel depends on values to stay in bounds.
 */
#ifndef TSGU_HIP_LOBPCG_H
#define TSGU_HIP_LOBPCG_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For callers that size operands and workspaces.  Host only.
 *   kmax                 the widest block (X, W, P) of the combine and residual kernels
 *   wmax                 the widest operand of the Gram kernel
 *   rows_per_workgroup   rows of a chunk
 *   workspace_bytes      what tsgu_tall_gram needs for n rows and an a x b result (tsgu_lobpcg_residual: a = k, b = 1) */
int tsgu_tall_geometry(int vtype, int64_t n, int64_t a, int64_t b, int* kmax, int* wmax, int* rows_per_workgroup,
                       int64_t* workspace_bytes);

/* c[a][b] (leading dimension ldc) = yᵀ·z for y [n][a] and z [n][b]; y and z may be the same view.  Each element is within
 * gamma_n·(|y|ᵀ|z|) of the exact value. */
int tsgu_tall_gram(int vtype, int64_t n, int64_t a, int64_t b, const void* y, int64_t ldy, const void* z, int64_t ldz, void* c,
                   int64_t ldc, void* workspace, int64_t workspace_bytes, int workgroups, int device, void* stream);

/* out_t[n][out_width[t]] = beta[t]·out_t + Σ_i s_i[n][s_width[i]] · coef[t·n_in + i]   for t < n_out <= 4, i < n_in <= 6.
 * The arrays s, s_width, s_ld, out, out_width, out_ld, beta, coef and coef_ld are HOST arrays (of device pointers, of int64_t, of
 * double); coef and coef_ld have n_out·n_in entries, coef[t·n_in + i] a row-major [s_width[i]][out_width[t]] matrix with leading
 * dimension coef_ld[t·n_in + i], or NULL: the block does not contribute.  beta may be NULL (all zero); out_t is read only where
 * beta[t] != 0.  Matrices passed more than once (same pointer and leading dimension) are held once; at most 6 distinct ones
 * (TSGU_ERR_TOO_LARGE).  An output may share no element with an input or with another output (TSGU_ERR_BAD_ARG): views that
 * interleave in one allocation (equal ld, disjoint column windows) share none, any other overlap of the address ranges counts. */
int tsgu_tall_combine(int vtype, int64_t n, int n_in, const void* const* s, const int64_t* s_width, const int64_t* s_ld, int n_out,
                      void* const* out, const int64_t* out_width, const int64_t* out_ld, const double* beta, const void* const* coef,
                      const int64_t* coef_ld, int workgroups, int device, void* stream);

/* r[n][k] = ax − x·diag(lam) with lam[k] read from device memory (a product and a difference: two roundings per element), and
 * sumsq[k] = the column sums of squares of r.  r may not share an element with ax or x. */
int tsgu_lobpcg_residual(int vtype, int64_t n, int64_t k, const void* ax, int64_t ldax, const void* x, int64_t ldx, const void* lam,
                         void* r, int64_t ldr, void* sumsq, void* workspace, int64_t workspace_bytes, int workgroups, int device,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_LOBPCG_H */
