// K12: the Chebyshev recurrence of sparse_expm_mm (sparse_expm.py): exp(t A) B ~ sum_k c_k w_k with w_{k+1} = 2 Ahat w_k - w_{k-1},
// Ahat = a A + b I.  The product A w_k is the caller's (the best kernel family of the pattern); the two kernels here are the rest
// of a step, on the lane walk of krylov_common.h.
//
// cheb_step_kernel walks the rows once: new = alpha prod + beta x - gamma prev (+ src), written over prev (the two-buffer ring of
// the recurrence) and, CHUNK, into slot `slot` of a [n][m][p] block — the row-major (n, m p) operand the backward's SDDMM wants, and
// what cheb_combine_kernel reads.  Five planes with a chunk: prod, x and prev read, prev and the slot written.
//
// cheb_combine_kernel touches the T time planes once per CHUNK of m steps instead of once per step (2 T planes per step would
// dwarf the recurrence itself): mode 0 keeps the T sums of a row in registers while the m slots stream past once, mode 1 keeps the
// T planes of G in registers and writes the m source terms of the adjoint recurrence.  The register arrays are
// [kPasses][TT][VEC] values, TT the power of two at or above T: 128 VGPRs at TT = 8 in either value type (4 x 8 x 4 floats,
// 4 x 8 x 2 doubles), which leaves 2 waves per SIMD; the 4 unrolled row passes, not the wave count, keep loads in flight.  The
// m T p coefficients are not staged in LDS: a lane loads the VEC values of its own columns once per (slot, time) and uses them for
// its kPasses rows; every workgroup reads the same table, which stays in L2.
// No reduction, no barrier, no atomics: the same bits on every run.
#pragma once

#include "krylov_common.h"

namespace tsgu {

constexpr int kChebTimeCap = 8;    // time planes of one combine launch (the register arrays above)
constexpr int kChebChunkCap = 64;  // slots of one chunk: a run-time loop, bounded so that a block of 16 columns fills an SDDMM call

// t0 = gamma * prev (0, and prev is not read, when gamma == 0);  t1 = fma(beta, x, -t0);  t2 = fma(alpha, prod, t1) (t1 without
// prod);  new = t2 + src[row][s_src][c] (t2 without src).  new goes over prev and, CHUNK, to chunk[row][slot][c].  src and chunk may
// be one array (and one slot): an element is read before it is written, by the same lane — hence no __restrict__ on the two.
template <typename V, int VEC, bool PROD, bool SRC, bool CHUNK>
__global__ __launch_bounds__(kBlock) void cheb_step_kernel(int64_t n, int64_t p, const V* __restrict__ prod, const V* __restrict__ x,
                                                           V* __restrict__ prev, V alpha, V beta, V gamma, const V* src,
                                                           int64_t src_ld, int64_t src_off, V* chunk, int64_t chunk_ld,
                                                           int64_t chunk_off, const int* __restrict__ flags, int lpr, int rpp) {
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    const bool use_prev = gamma != (V)0;
    for_rows(L, n, [&](int, int64_t row) {
        const int64_t o = row * p + L.c;
        V xv[VEC], pv[VEC] = {}, av[VEC], sv[VEC], out[VEC];
        load_vec<V, VEC>(x + o, xv);
        if (use_prev) load_vec<V, VEC>(prev + o, pv);
        if constexpr (PROD) load_vec<V, VEC>(prod + o, av);
        if constexpr (SRC) load_vec<V, VEC>(src + row * src_ld + src_off + L.c, sv);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const V t0 = use_prev ? gamma * pv[k] : (V)0;
            V t = fma(beta, xv[k], -t0);
            if constexpr (PROD) t = fma(alpha, av[k], t);
            if constexpr (SRC) t = t + sv[k];
            out[k] = t;
        }
        store_vec<V, VEC>(prev + o, out);
        if constexpr (CHUNK) store_vec<V, VEC>(chunk + row * chunk_ld + chunk_off + L.c, out);
    });
}

// MODE 0 (emit), per time j < T:  t = coef[0][j][c] * chunk[row][0][c];  t = fma(coef[s][j][c], chunk[row][s][c], t) for s = 1 ... m - 1
//                 in that order;  planes[j][row][c] = accumulate ? planes[j][row][c] + t : t.
// MODE 1 (spread), per slot s < m: t = coef[s][0][c] * planes[0][row][c];  t = fma(coef[s][j][c], planes[j][row][c], t) for
//                 j = 1 ... T - 1 in that order;  chunk[row][s][c] = t.
template <typename V, int VEC, int TT, int MODE>
__global__ __launch_bounds__(kBlock) void cheb_combine_kernel(int64_t n, int64_t p, int m, int T, int accumulate, V* __restrict__ chunk,
                                                              const V* __restrict__ coef, V* __restrict__ planes, int64_t plane_stride,
                                                              const int* __restrict__ flags, int lpr, int rpp) {
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    if (!L.on) return;
    const int64_t ld = (int64_t)m * p;
    V reg[kPasses][TT][VEC];
    if constexpr (MODE == 0) {
        for (int s = 0; s < m; ++s) {
            V xs[kPasses][VEC];
#pragma unroll
            for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
                for (int k = 0; k < VEC; ++k) xs[ps][k] = 0;
            for_rows(L, n, [&](int ps, int64_t row) { load_vec<V, VEC>(chunk + row * ld + (int64_t)s * p + L.c, xs[ps]); });
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                if (j < T) {
                    V cf[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) cf[k] = coef[((int64_t)s * T + j) * p + L.c + k];
#pragma unroll
                    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) reg[ps][j][k] = s == 0 ? cf[k] * xs[ps][k] : fma(cf[k], xs[ps][k], reg[ps][j][k]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            if (j < T) {
                V* dst = planes + (int64_t)j * plane_stride;
                for_rows(L, n, [&](int ps, int64_t row) {
                    const int64_t o = row * p + L.c;
                    if (accumulate) {
                        V a[VEC];
                        load_vec<V, VEC>(dst + o, a);
#pragma unroll
                        for (int k = 0; k < VEC; ++k) reg[ps][j][k] = a[k] + reg[ps][j][k];
                    }
                    store_vec<V, VEC>(dst + o, reg[ps][j]);
                });
            }
        }
    } else {
#pragma unroll
        for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
            for (int j = 0; j < TT; ++j)
#pragma unroll
                for (int k = 0; k < VEC; ++k) reg[ps][j][k] = 0;
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            if (j < T) {
                const V* g = planes + (int64_t)j * plane_stride;
                for_rows(L, n, [&](int ps, int64_t row) { load_vec<V, VEC>(g + row * p + L.c, reg[ps][j]); });
            }
        }
        for (int s = 0; s < m; ++s) {
            V out[kPasses][VEC];
#pragma unroll
            for (int j = 0; j < TT; ++j) {
                if (j < T) {
                    V cf[VEC];
#pragma unroll
                    for (int k = 0; k < VEC; ++k) cf[k] = coef[((int64_t)s * T + j) * p + L.c + k];
#pragma unroll
                    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) out[ps][k] = j == 0 ? cf[k] * reg[ps][j][k] : fma(cf[k], reg[ps][j][k], out[ps][k]);
                }
            }
            for_rows(L, n, [&](int ps, int64_t row) { store_vec<V, VEC>(chunk + row * ld + (int64_t)s * p + L.c, out[ps]); });
        }
    }
}

}  // namespace tsgu
