/*
 * tsgu_hip_gmres.h — the Arnoldi kernels of restarted GMRES (utils/gmres.py): entries of libtsgu_hip.so.
 *
 * STAGED: this header lives beside the sources and not under include/ ("Adding a header"); its entries are bound
 * from `_backend.STAGED_GMRES`.  An addition to the C ABI of tsgu_hip.h with the same conventions (device pointers, `device` + `stream`
 * last, status codes, tsgu_vtype, no synchronisation, no allocation).  The entries are additive, so TSGU_ABI_VERSION stays as it
 * is.  The reference has no counterpart.
 *
 * Operands.  Values are TSGU_F32 or TSGU_F64 (TSGU_BF16 is TSGU_ERR_BAD_DTYPE).  A block is a contiguous row-major [n][p] array,
 * 16-byte aligned: the p columns are independent problems that advance in lock-step.  A basis is `k` such blocks, block i at
 * `basis + i * slab` elements with slab >= n * p a multiple of 4 (every block starts on a 16-byte boundary; anything else is
 * TSGU_ERR_BAD_ARG): column c of block i is basis vector i of problem c.  The lane geometry is that
 * of the Krylov step kernels of tsgu_hip.h: any p up to 256, above that multiples of the 16-byte lane width (4 fp32 / 2 fp64
 * columns) up to 256 lanes; every other p is TSGU_ERR_TOO_LARGE.  A workgroup owns `rows_per_workgroup` consecutive rows, workgroup
 * b the rows from b * rows_per_workgroup on; a launch writes `partial_rows` = ceil(n / rows_per_workgroup) partial rows
 * (tsgu_gmres_geometry).
 *
 * State of a solve with restart length m (1 <= m <= restart cap), kept by tsgu_gmres_scalar:
 *   scal   value type, rows of p values, m * m + 6 m + 4 rows:
 *          row 0 threshold | 1 estimate (the true residual norm at a cycle start, |g_{j+1}| after inner step j) | 2 hnorm
 *          (what tsgu_gmres_scale divides by: beta at a cycle start, h_{j+1,j} after inner step j) | 3 ... m + 3: g (m + 1 rows) |
 *          m + 4: cs (m) | 2 m + 4: sn (m) | 3 m + 4: y (m) | 4 m + 4: h, the Hessenberg column being built (m) |
 *          5 m + 4: coef, what the next subtraction takes away (m) | 6 m + 4: R, the rotated Hessenberg matrix, upper
 *          triangular, entry (i, j) in row 6 m + 4 + i * m + j
 *   flags  int32, 4 + 4 p words: [0] stop: every column is finished | [1] every column's cycle has ended | [2] cycles started |
 *          [3] inner steps run | [4, 4 + p) finished | [4 + p, 4 + 2 p) cycle ended | [4 + 2 p, 4 + 3 p) steps_c, inner steps of
 *          this cycle | [4 + 3 p, 4 + 4 p) iters_c, inner steps of the column since the solve began
 * The caller zeroes both before the first call.  Every launcher returns at once, writing nothing, when flags[0] != 0; with
 * `inner` != 0 also when flags[1] != 0 (the step of a cycle that no column still runs).
 *
 * Determinism: no atomics on values.  A partial row sums a workgroup's rows in an order that depends on (n, p, k) alone, and
 * tsgu_gmres_scalar sums partial rows in an order that depends on their count and p alone: two runs give the same bits.  Every
 * product that enters a sum is formed inside a fused multiply-add.
 *
 * Every launcher refuses on the host, before any launch: NULL pointers, n <= 0, p <= 0, k outside [1, restart cap + 1], operands
 * that are not 16-byte aligned (TSGU_ERR_BAD_ARG), unknown value types (TSGU_ERR_BAD_DTYPE), a p the lane geometry does not cover
 * (TSGU_ERR_TOO_LARGE).
 */
#ifndef TSGU_HIP_GMRES_H
#define TSGU_HIP_GMRES_H

#include "../../include/tsgu_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only.  restart_cap: the largest restart length (a compile-time constant, at least 64); group: basis vectors a workgroup
 * walks together (speed only); rows_per_workgroup and partial_rows for an [n][p] block of `vtype` as above.  TSGU_ERR_TOO_LARGE
 * for a p the lane geometry does not cover. */
int tsgu_gmres_geometry(int vtype, int64_t n, int64_t p, int* restart_cap, int* group, int64_t* rows_per_workgroup,
                        int64_t* partial_rows);

/* partial[b][i][c] = sum over the rows r of workgroup b of basis_i[r][c] * w[r][c] for i < k, and partial[b][k][c] = the sum of
 * w[r][c]^2: partial_rows * (k + 1) * p values.  Each sum is over at most rows_per_workgroup fused multiply-adds. */
int tsgu_gmres_project(int vtype, int64_t n, int64_t p, int k, const void* w, const void* basis, int64_t slab, void* partial,
                       const int* flags, int inner, int device, void* stream);

/* out[r][c] = w[r][c] - sum_{i<k} coef[i][c] * basis_i[r][c], one fused multiply-add per basis vector in the order i = 0 ... k - 1
 * (t <- fma(-coef[i][c], basis_i[r][c], t) from t = w[r][c]), and partial[b][c] = the sum of out[r][c]^2 over the rows of
 * workgroup b: partial_rows * p values.  coef: [k][p].  Every column is computed (the caller's scale discards the columns whose
 * cycle has ended).  out may be w; it may not overlap the basis.  With k = 1, basis = A x and coef = 1 this is the residual
 * b - A x of a cycle start and its norm. */
int tsgu_gmres_subtract(int vtype, int64_t n, int64_t p, int k, const void* w, const void* basis, int64_t slab, const void* coef,
                        void* out, void* partial, const int* flags, int inner, int device, void* stream);

/* out[r][c] = w[r][c] * (1 / hnorm[c]) — one division per column, one multiplication per element — and 0 for a column whose
 * "cycle ended" flag is set (hnorm is not read for it).  hnorm: [p], row 2 of scal.  out may be w.  With `inner` != 0 and
 * flags[1] set the launch writes nothing, as every launcher: the zero block of an ended column is written only while another
 * column's cycle still runs.  Once every cycle has ended `out` keeps what it held, which nothing reads before the next cycle
 * start: tsgu_gmres_update is bounded by steps_c and the cycle start rewrites block 0. */
int tsgu_gmres_scale(int vtype, int64_t n, int64_t p, const void* w, const void* hnorm, void* out, const int* flags, int inner,
                     int device, void* stream);

/* One phase of the per-column state on one workgroup.  m: the restart length (TSGU_ERR_BAD_ARG outside [1, restart cap]); j: the
 * inner step, 0 <= j < m (phases 1 to 3).  partial: `n_partial` rows (>= 1) as the phase's producer wrote them; more than 1024 of
 * them are first summed to 256 rows in `fold` (256 * (m + 1) * p values; may be NULL: no folding).  Not read in phase 4.
 *   phase 0, cycle start   partial [n_partial][p] of tsgu_gmres_subtract: beta = sqrt(sum).  On the first call (flags[2] = 0) for
 *            every column threshold = max(abstol, reltol * beta), finished = 0, iters_c = 0.  Then for a column that is not
 *            finished: estimate = hnorm = g_0 = beta, and it becomes finished when beta <= threshold or iters_c >= maxiter.
 *            Every column: cycle ended = finished, steps_c = 0.  flags[2] += 1; flags[0] = flags[1] = all finished.
 *   phase 1, after the first projection     partial [n_partial][j + 2][p] of tsgu_gmres_project with k = j + 1: for a column whose
 *            cycle has not ended h_i = coef_i = the sum, i <= j.
 *   phase 2, after the second projection    the same partial: coef_i = the sum, h_i = h_i + coef_i.
 *   phase 3, after the norm   partial [n_partial][p] of the second tsgu_gmres_subtract: hn = sqrt(sum).  For a column whose cycle has
 *            not ended: for i < j (h_i, h_{i+1}) <- (cs_i h_i + sn_i h_{i+1}, cs_i h_{i+1} - sn_i h_i); d = sqrt(h_j^2 + hn^2);
 *            (cs_j, sn_j) = (h_j / d, hn / d), or (1, 0) when d = 0; h_j <- cs_j h_j + sn_j hn; R(i, j) = h_i for i <= j;
 *            g_{j+1} = -(sn_j g_j), g_j <- cs_j g_j; estimate = |g_{j+1}|; hnorm = hn; steps_c = j + 1; iters_c += 1; its cycle
 *            ends when estimate <= threshold, hn = 0 (a lucky breakdown) or iters_c >= maxiter.  flags[3] += 1; flags[1] = every
 *            cycle has ended.  A column whose cycle has ended is untouched.
 *   phase 4, cycle end     per column with s = steps_c (0 for a finished column): y_i = (g_i - sum_{i<l<s} R(i, l) y_l) / R(i, i)
 *            for i = s - 1 ... 0, each term rounded and subtracted in the order l = i + 1 ... s - 1, 0 where R(i, i) = 0;
 *            y_i = 0 for s <= i < m. */
int tsgu_gmres_scalar(int vtype, int phase, int j, int m, const void* partial, int64_t n_partial, void* fold, void* scal, int* flags,
                      double abstol, double reltol, int maxiter, int64_t p, int device, void* stream);

/* x[r][c] += sum over i < min(k, steps_c[c]) of y[i][c] * basis_i[r][c], one fused multiply-add per basis vector in the order
 * i = 0, 1, ...; a column with steps_c = 0 keeps its bits.  y: [k][p] (row 3 m + 4 of scal).  x may not overlap the basis. */
int tsgu_gmres_update(int vtype, int64_t n, int64_t p, int k, void* x, const void* basis, int64_t slab, const void* y,
                      const int* flags, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TSGU_HIP_GMRES_H */
