/*
 * tsgu_hip_quadrature.h — Gauss quadrature of Lanczos tridiagonal matrices and the Rademacher probe block of sparse_logdet
 * (sparse_logdet.py): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_QUADRATURE`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` +
 * `stream` last, status codes, tsgu_vtype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays
 * as it is.  The reference has no counterpart: its linear_cg returns the tridiagonal matrices and stops there.
 *
 * Quadrature.  For a symmetric tridiagonal r_c x r_c matrix T with eigenvalues lambda_j and first eigenvector components tau_j,
 * sum_j tau_j^2 f(lambda_j) = e_1' f(T) e_1.  With T the Lanczos matrix of (A, z / |z|) this is the Gauss rule for
 * z' f(A) z / |z|^2; conjugate gradients on A x = z / |z| produce T's entries from their coefficients (alpha_k, beta_k).
 *
 * Column length.  `coef` holds r rows; each column c has its own length r_c <= r, found by the kernel:
 *   kind 0   the matrix ends BEFORE the first row whose alpha is not a positive finite number (a zero row of a history CG never
 *            reached, a column CG froze), and AFTER the first row whose beta is not a positive finite number (the Krylov space is
 *            exhausted: the rule is exact there);
 *   kind 1   the matrix ends AFTER the first row whose off-diagonal is zero or not finite, and after row r - 1 at the latest.
 * No row count is passed in, and no column looks at another.
 *
 * Arithmetic: float64 whatever the value type.  The eigenvalues and first components come from the implicit QL iteration with
 * Wilkinson shifts, rotating only the first row of the eigenvector matrix (Golub-Welsch) — not from the three-term recurrence at
 * each eigenvalue, which loses the weights once the Krylov space is nearly exhausted.  A launch gives the same bits every time.
 *
 * Every launcher refuses on the host, before any launch: NULL pointers, r <= 0, p <= 0, n <= 0, unknown `kind` / `fn`
 * (TSGU_ERR_BAD_ARG), r above the cap or a block the grid cannot cover (TSGU_ERR_TOO_LARGE), value types other than TSGU_F32 and
 * TSGU_F64 (TSGU_ERR_BAD_DTYPE; TSGU_BF16 included).
 */
#ifndef TSGU_HIP_QUADRATURE_H
#define TSGU_HIP_QUADRATURE_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  steps_cap: the largest r of tsgu_tridiag_quadrature (a compile-time constant, at least 128);
 * work_bytes_per_column: bytes of `work` per column that a launch with r > 64 needs (r <= 64 never reads `work`). */
int tsgu_quadrature_geometry(int* steps_cap, int64_t* work_bytes_per_column);

/* out[c] = scale[c] * sum_j tau_j^2 f(lambda_j) over column c's r_c x r_c tridiagonal matrix, c < p.
 *   coef   [r][2][p] in the value type.  kind 0: row k holds the CG coefficients (alpha_k, beta_k) — the `hist` array
 *          tsgu_cg2_direction writes — and T[k][k] = 1 / alpha_k + beta_{k-1} / alpha_{k-1}, T[k][k+1] = sqrt(beta_k) / alpha_k.
 *          kind 1: row k holds (T[k][k], T[k][k+1]); the off-diagonal of the last row is ignored.
 *   fn     0: log, 1: reciprocal, 2: lambda (the sum is T[0][0]), 3: one (the sum is 1).
 *   scale  [p] in the value type, or NULL for 1.
 *   out    [p] in the value type; 0 for r_c = 0.
 *   info   [p] int32: r_c, or -r_c when fn is 0 or 1 and a lambda_j <= 0 was met; out[c] is NaN then.
 *   work   float64 scratch of p * work_bytes_per_column bytes, 8-byte aligned; may be NULL when r <= 64 (TSGU_ERR_BAD_ARG when it
 *          is NULL and the launch needs it).  Up to 100 rows a lane's three arrays live in LDS, [row][lane]; above, in `work`,
 *          [array][row][column]. */
int tsgu_tridiag_quadrature(int vtype, int kind, int fn, int r, int64_t p, const void* coef, const void* scale, void* out, int* info,
                            void* work, int device, void* stream);

/* out[i][c] = +1 or -1 for i < n, c < p ([n][p] in the value type, n < 2^32), a pure function of (seed, i, c):
 *   lowbias32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (32-bit words)
 *   s = lowbias32(lo32(seed) ^ lowbias32(hi32(seed)))
 *   h = lowbias32(c + lowbias32(i + s))          (sums modulo 2^32)
 *   out[i][c] = -1 if h >> 31 else +1
 * `_cpu.rademacher_fill` is the same expression in torch ops: CPU and GPU operands get the same probes bit for bit. */
int tsgu_rademacher_fill(int vtype, int64_t n, int64_t p, int64_t seed, void* out, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_QUADRATURE_H */
