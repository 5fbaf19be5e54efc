// K11: the contour-quadrature update of sparse_inv_sqrt_mm (sparse_sqrt.py): A^(-1/2) B ~ sum_q omega_q (A + sigma_q I)^(-1) B by
// multi-shift MINRES whose S solutions are never stored.  The Lanczos step and the Givens phase are those of minres.hip
// (tsgu_minres_vector_ms which = 0, tsgu_minres_scalar_ms phases 0 and 1); the two kernels here read their scal [S][12][p]:
//   1 beta_c | 6 scale_c (= -scale_prev s_c: MINRES's residual estimate after this step) | 7 sub | 8 subsub | 9 diag | 10 scale
//
// ciq_update_kernel walks the rows ONCE with the shifts innermost per row: the thread's q values (z one step back) and its weighted
// sum t = sum_q omega_q w_q scale_q stay in registers over the whole shift loop, so one iteration moves 3 S + 5 planes (w_prev2 and
// w_prev read, w_c written per shift; z_c read + written, q read, acc read + written) instead of the 6 S + 2 of minres_update_kernel
// followed by a weighted sum, and 5 S + 5 with `keep`.  The 4 S p per-shift scalars are NOT staged in LDS: at the widest block
// (1024 fp32 columns, 32 shifts) they are 512 KiB, more than three times the 160 KiB of a compute unit; each thread loads the four
// values of its own columns once per shift (they stay in L2 / the vector cache: every workgroup reads the same 4 S p values) and uses
// them for its kPasses rows.  No reduction, no barrier, no atomics: the same bits on every run.
//
// ciq_stop_kernel (one workgroup) turns the Givens phase's residual estimates into the per-column `done` words and the stop word.
#pragma once

#include "krylov_common.h"

namespace tsgu {

constexpr int kCiqShiftCap = 32;  // shifts per launch (the rule of sparse_inv_sqrt_mm needs 8 ... 20)

// zc /= beta_c (in place).  Per live column c (done[c] == 0), for q = 0 ... S - 1 in that order:
//   w_c = ((qp - sub w_p) - subsub w_pp) / diag   written over w_pp;   up = w_c scale;   t = fma(omega_q, up, t);
//   KEEP: keep[row][q][c] += up
// then acc[row][c] += t.  A done column keeps every bit of w, keep and acc (a lane whose columns are all done touches none of them).
template <typename V, int VEC, bool KEEP>
__global__ __launch_bounds__(kBlock) void ciq_update_kernel(int64_t n, int64_t p, int n_shift, V* __restrict__ zc, const V* __restrict__ qp,
                                                            V* __restrict__ wpp, const V* __restrict__ wp, int64_t np,
                                                            V* __restrict__ acc, V* __restrict__ keep, const V* __restrict__ scal,
                                                            const V* __restrict__ omega, const int* __restrict__ done,
                                                            const int* __restrict__ flags, int lpr, int rpp) {
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    if (!L.on) return;
    V beta[VEC];
    bool live[VEC];
    bool any = false;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        beta[k] = scal[p + L.c + k];
        live[k] = done[L.c + k] == 0;
        any = any || live[k];
    }
    V q[kPasses][VEC], t[kPasses][VEC];
    for_rows(L, n, [&](int ps, int64_t row) {
        const int64_t o = row * p + L.c;
        V z[VEC];
        load_vec<V, VEC>(zc + o, z);
#pragma unroll
        for (int k = 0; k < VEC; ++k) z[k] = z[k] / beta[k];
        store_vec<V, VEC>(zc + o, z);
        if (any) load_vec<V, VEC>(qp + o, q[ps]);
#pragma unroll
        for (int k = 0; k < VEC; ++k) t[ps][k] = 0;
    });
    if (!any) return;
    const int64_t keep_ld = (int64_t)n_shift * p;
    for (int sh = 0; sh < n_shift; ++sh) {
        const V* blk = scal + (int64_t)sh * 12 * p + L.c;
        V* wpp_s = wpp + sh * np;
        const V* wp_s = wp + sh * np;
        const V om = omega[sh];
        V sub[VEC], subsub[VEC], diag[VEC], scale[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            sub[k] = blk[7 * p + k];
            subsub[k] = blk[8 * p + k];
            diag[k] = blk[9 * p + k];
            scale[k] = blk[10 * p + k];
        }
        for_rows(L, n, [&](int ps, int64_t row) {
            const int64_t o = row * p + L.c;
            V w2[VEC], w1[VEC], up[VEC];
            load_vec<V, VEC>(wpp_s + o, w2);
            load_vec<V, VEC>(wp_s + o, w1);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const V wc = ((q[ps][k] - sub[k] * w1[k]) - subsub[k] * w2[k]) / diag[k];
                up[k] = wc * scale[k];
                if (live[k]) {
                    w2[k] = wc;
                    t[ps][k] = fma(om, up[k], t[ps][k]);
                }
            }
            store_vec<V, VEC>(wpp_s + o, w2);
            if constexpr (KEEP) {
                V* kp = keep + row * keep_ld + (int64_t)sh * p + L.c;
                V x[VEC];
                load_vec<V, VEC>(kp, x);
#pragma unroll
                for (int k = 0; k < VEC; ++k) x[k] = live[k] ? x[k] + up[k] : x[k];
                store_vec<V, VEC>(kp, x);
            }
        });
    }
    for_rows(L, n, [&](int ps, int64_t row) {
        const int64_t o = row * p + L.c;
        V a[VEC];
        load_vec<V, VEC>(acc + o, a);
#pragma unroll
        for (int k = 0; k < VEC; ++k) a[k] = live[k] ? a[k] + t[ps][k] : a[k];
        store_vec<V, VEC>(acc + o, a);
    });
}

// est[c] = max_q |scal[q][6][c]| (NaN when one of them is NaN);  done[c] |= est[c] <= tol (NaN compares false);
// flags[0] = 1 when every column is done.  One workgroup.
template <typename V>
__global__ __launch_bounds__(kBlock) void ciq_stop_kernel(int64_t p, int n_shift, const V* __restrict__ scal, V tol, V* __restrict__ est,
                                                          int* __restrict__ done, int* __restrict__ flags) {
    if (flags[0] != 0) return;
    int all = 1;
    for (int64_t c = threadIdx.x; c < p; c += kBlock) {
        V m = 0;
        for (int sh = 0; sh < n_shift; ++sh) {
            const V v = fabs(scal[((int64_t)sh * 12 + 6) * p + c]);
            if (v != v || (m == m && v > m)) m = v;
        }
        est[c] = m;
        const int d = (done[c] != 0 || m <= tol) ? 1 : 0;
        done[c] = d;
        all &= d;
    }
    all = __syncthreads_and(all);
    if (threadIdx.x == 0 && all) flags[0] = 1;
}

}  // namespace tsgu
