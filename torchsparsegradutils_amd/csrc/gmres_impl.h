// K8: the Arnoldi hot path of restarted GMRES(m) on gfx950, every right-hand side at once (contracts: tsgu_hip_gmres.h).
//
// The columns of an [n][p] block are independent problems that advance in lock-step: every column has its own Krylov basis (column
// c of the slabs V_0 ... V_m), its own Hessenberg column, rotations, stopping point and counters, all in device arrays.  One inner
// step with classical Gram-Schmidt and one re-orthogonalisation is
//   (z = M V_j, w = A z by the caller) -> project -> scalar(H1) -> subtract -> project -> scalar(H2) -> subtract(+|w|^2)
//   -> scalar(ROTATE) -> scale
// two global reductions instead of the j + 1 dependent ones of modified Gram-Schmidt.  The streaming kernels are written on the
// lane walk of krylov_common.h: a workgroup keeps its kPasses rows of w in registers and walks the basis in groups of kGmresGroup
// vectors, so w is read once per launch and kGmresGroup * kPasses independent 16-byte loads are in flight per thread.  All sums are
// in a fixed order, without atomics.
//
// scal (value type, rows of p):  0 threshold | 1 estimate | 2 hnorm | 3 g (m + 1) | m + 4 cs (m) | 2m + 4 sn (m) | 3m + 4 y (m)
//                                | 4m + 4 h (m) | 5m + 4 coef (m) | 6m + 4 R (m * m, R[i][j] in row i * m + j)
// flags (int32): [0] stop | [1] every column's cycle has ended | [2] cycles started | [3] inner steps run | then four arrays of p:
//                finished | cycle ended | steps of this cycle | inner steps of the column
#pragma once

#include "krylov_common.h"

namespace tsgu {

constexpr int kGmresCap = 64;   // largest restart length the scalar state is laid out for
constexpr int kGmresGroup = 4;  // basis vectors walked together (accumulators: kGmresGroup * VEC per thread)
constexpr int kGmresFlags = 4;  // words in front of the per-column arrays of `flags`

enum GmresPhase { kGmresStart = 0, kGmresH1 = 1, kGmresH2 = 2, kGmresRotate = 3, kGmresSolve = 4 };

__device__ __forceinline__ bool gmres_idle(const int* __restrict__ flags, int inner) {
    return flags[0] != 0 || (inner && flags[1] != 0);
}

// The partial rows of a group of accumulators at once: dst[g * p + cc] = the sum over the row slots of what lane (slot, cc) holds
// in acc[g], g < cnt.  fold_partial_row sums a column's rpp slots on ONE thread; with few columns (p = 1: 256 slots) and one such
// sum per basis vector that chain, not the basis stream, is what a projection waits for.  Here the cnt * p sums of a group share
// one LDS round, and while they are fewer than the workgroup's threads each is split into up to 16 contiguous runs of slots summed
// by different threads, then the runs in order: a fixed association that depends on (lpr, rpp, cnt) alone, no atomics.
// red: kGmresGroup * kBlock * VEC + kBlock values; called by every thread; ends with a barrier.
constexpr int kGmresRuns = 16;

template <typename V, int VEC>
__device__ __forceinline__ void fold_group(V* red, const V (&acc)[kGmresGroup][VEC], int cnt, const Lanes& L, int64_t p,
                                           V* __restrict__ dst) {
    constexpr int S = kBlock * VEC;
    V* red2 = red + kGmresGroup * S;
    const int W = L.lpr * VEC;  // column slots of a row slot (= p)
    const int t = threadIdx.x;
    if (L.rs < L.rpp) {
#pragma unroll
        for (int g = 0; g < kGmresGroup; ++g)
#pragma unroll
            for (int v = 0; v < VEC; ++v) red[g * S + (L.rs * L.lpr + L.cl) * VEC + v] = acc[g][v];
    }
    __syncthreads();
    const int64_t outs = (int64_t)cnt * p;
    int runs = outs < kBlock ? (int)(kBlock / outs) : 1;
    runs = runs > kGmresRuns ? kGmresRuns : runs;
    runs = runs > L.rpp ? L.rpp : runs;
    if (runs <= 1) {
        for (int64_t o = t; o < outs; o += kBlock) {
            const int g = (int)(o / p), cc = (int)(o % p);
            V sum = 0;
            for (int k = 0; k < L.rpp; ++k) sum += red[g * S + k * W + cc];
            dst[o] = sum;
        }
    } else {
        const int len = (L.rpp + runs - 1) / runs;
        const int o = t % (int)outs, run = t / (int)outs;
        if (run < runs) {
            const int g = o / (int)p, cc = o % (int)p;
            const int k1 = (run + 1) * len < L.rpp ? (run + 1) * len : L.rpp;
            V sum = 0;
            for (int k = run * len; k < k1; ++k) sum += red[g * S + k * W + cc];
            red2[run * (int)outs + o] = sum;
        }
        __syncthreads();
        if (t < outs) {
            V sum = 0;
            for (int r = 0; r < runs; ++r) sum += red2[r * (int)outs + t];
            dst[t] = sum;
        }
    }
    __syncthreads();
}

// partial[b][i][c] = sum over the rows of workgroup b of V_i[row][c] * w[row][c] for i < k; row k: sum of w^2.
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void gmres_project_kernel(int64_t n, int64_t p, int k, const V* __restrict__ w,
                                                               const V* __restrict__ basis, int64_t slab, V* __restrict__ partial,
                                                               const int* __restrict__ flags, int inner, int lpr, int rpp) {
    __shared__ V red[kGmresGroup * kBlock * VEC + kBlock];
    if (gmres_idle(flags, inner)) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    V* dst = partial + (int64_t)blockIdx.x * (k + 1) * p;
    V ww[kPasses][VEC];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
        for (int v = 0; v < VEC; ++v) ww[ps][v] = 0;
    for_rows(L, n, [&](int ps, int64_t row) { load_vec<V, VEC>(w + row * p + L.c, ww[ps]); });
    for (int i0 = 0; i0 < k; i0 += kGmresGroup) {
        V acc[kGmresGroup][VEC];
#pragma unroll
        for (int g = 0; g < kGmresGroup; ++g) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[g][v] = 0;
            if (i0 + g < k) {
                const V* vi = basis + (int64_t)(i0 + g) * slab;
                for_rows(L, n, [&](int ps, int64_t row) {
                    V vv[VEC];
                    load_vec<V, VEC>(vi + row * p + L.c, vv);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[g][v] = fma(vv[v], ww[ps][v], acc[g][v]);
                });
            }
        }
        fold_group<V, VEC>(red, acc, k - i0 < kGmresGroup ? k - i0 : kGmresGroup, L, p, dst + (int64_t)i0 * p);
    }
    V sq[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        sq[v] = 0;
#pragma unroll
        for (int ps = 0; ps < kPasses; ++ps) sq[v] = fma(ww[ps][v], ww[ps][v], sq[v]);
    }
    fold_partial_row<V, VEC>(red, sq, L, p, dst + (int64_t)k * p);
}

// out[row][c] = w[row][c] - sum_{i<k} coef[i][c] V_i[row][c], one fma per basis vector in the order i = 0 ... k - 1;
// partial[b][c] = sum over the rows of workgroup b of out^2.  out may be w.
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void gmres_subtract_kernel(int64_t n, int64_t p, int k, const V* w, const V* __restrict__ basis,
                                                                int64_t slab, const V* __restrict__ coef, V* out,
                                                                V* __restrict__ partial, const int* __restrict__ flags, int inner,
                                                                int lpr, int rpp) {
    __shared__ V red[kBlock * VEC];
    if (gmres_idle(flags, inner)) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    V ww[kPasses][VEC];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
        for (int v = 0; v < VEC; ++v) ww[ps][v] = 0;
    for_rows(L, n, [&](int ps, int64_t row) { load_vec<V, VEC>(w + row * p + L.c, ww[ps]); });
    for (int i0 = 0; i0 < k; i0 += kGmresGroup) {
#pragma unroll
        for (int g = 0; g < kGmresGroup; ++g) {
            if (i0 + g < k) {
                V cf[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) cf[v] = L.on ? -coef[(int64_t)(i0 + g) * p + L.c + v] : (V)0;
                const V* vi = basis + (int64_t)(i0 + g) * slab;
                for_rows(L, n, [&](int ps, int64_t row) {
                    V vv[VEC];
                    load_vec<V, VEC>(vi + row * p + L.c, vv);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) ww[ps][v] = fma(cf[v], vv[v], ww[ps][v]);
                });
            }
        }
    }
    V sq[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) sq[v] = 0;
    for_rows(L, n, [&](int ps, int64_t row) {
        store_vec<V, VEC>(out + row * p + L.c, ww[ps]);
#pragma unroll
        for (int v = 0; v < VEC; ++v) sq[v] = fma(ww[ps][v], ww[ps][v], sq[v]);
    });
    fold_partial_row<V, VEC>(red, sq, L, p, partial + (int64_t)blockIdx.x * p);
}

// out[row][c] = w[row][c] * (1 / hnorm[c]); 0 for a column whose cycle has ended.
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void gmres_scale_kernel(int64_t n, int64_t p, const V* w, const V* __restrict__ hnorm, V* out,
                                                             const int* __restrict__ flags, int inner, int lpr, int rpp) {
    if (gmres_idle(flags, inner)) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    if (!L.on) return;
    const int* ended = flags + kGmresFlags + p;
    V inv[VEC];
    bool act[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        act[v] = ended[L.c + v] == 0;
        inv[v] = act[v] ? (V)1 / hnorm[L.c + v] : (V)0;
    }
    for_rows(L, n, [&](int, int64_t row) {
        V vv[VEC];
        load_vec<V, VEC>(w + row * p + L.c, vv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) vv[v] = act[v] ? vv[v] * inv[v] : (V)0;
        store_vec<V, VEC>(out + row * p + L.c, vv);
    });
}

// x[row][c] += sum_{i < min(k, steps[c])} y[i][c] basis_i[row][c], one fma per basis vector in the order i = 0, 1, ...
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void gmres_update_kernel(int64_t n, int64_t p, int k, V* __restrict__ x,
                                                              const V* __restrict__ basis, int64_t slab, const V* __restrict__ y,
                                                              const int* __restrict__ flags, int lpr, int rpp) {
    if (flags[0] != 0) return;
    const Lanes L = lanes<VEC>(p, lpr, rpp);
    if (!L.on) return;
    const int* steps = flags + kGmresFlags + 2 * p;
    int st[VEC], top = 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        st[v] = steps[L.c + v] < k ? steps[L.c + v] : k;
        top = st[v] > top ? st[v] : top;
    }
    if (top == 0) return;
    V xx[kPasses][VEC];
#pragma unroll
    for (int ps = 0; ps < kPasses; ++ps)
#pragma unroll
        for (int v = 0; v < VEC; ++v) xx[ps][v] = 0;
    for_rows(L, n, [&](int ps, int64_t row) { load_vec<V, VEC>(x + row * p + L.c, xx[ps]); });
    for (int i = 0; i < top; ++i) {
        V yy[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) yy[v] = y[(int64_t)i * p + L.c + v];
        const V* vi = basis + (int64_t)i * slab;
        for_rows(L, n, [&](int ps, int64_t row) {
            V vv[VEC];
            load_vec<V, VEC>(vi + row * p + L.c, vv);
#pragma unroll
            for (int v = 0; v < VEC; ++v) xx[ps][v] = i < st[v] ? fma(yy[v], vv[v], xx[ps][v]) : xx[ps][v];
        });
    }
    for_rows(L, n, [&](int ps, int64_t row) { store_vec<V, VEC>(x + row * p + L.c, xx[ps]); });
}

// The per-column scalar state, one workgroup.  `src`: the partial rows of the phase, `rows` of them, `stride` elements apart
// ((k + 1) p for the projections, p for the norms).
template <typename V>
__global__ __launch_bounds__(kBlock) void gmres_scalar_kernel(int phase, int j, int m, const V* __restrict__ src, int64_t rows,
                                                              int64_t stride, int64_t p, V* __restrict__ scal, int* __restrict__ flags,
                                                              V abstol, V reltol, int maxiter) {
    __shared__ V red[kBlock];
    __shared__ int s_all;
    if (flags[0] != 0) return;
    const int t = threadIdx.x;
    int* fin = flags + kGmresFlags;
    int* ended = fin + p;
    int* steps = ended + p;
    int* iters = steps + p;
    V* thr = scal;
    V* est = scal + p;
    V* hnorm = scal + 2 * p;
    V* g = scal + 3 * p;
    V* cs = scal + (int64_t)(m + 4) * p;
    V* sn = scal + (int64_t)(2 * m + 4) * p;
    V* y = scal + (int64_t)(3 * m + 4) * p;
    V* h = scal + (int64_t)(4 * m + 4) * p;
    V* coef = scal + (int64_t)(5 * m + 4) * p;
    V* R = scal + (int64_t)(6 * m + 4) * p;
    if (phase == kGmresH1 || phase == kGmresH2) {
        // h1 = V^T w; after the re-orthogonalisation h = h1 + h2.  coef: what the next subtraction takes away.
        const int k = j + 1;
        for (int i = 0; i < k; ++i) {
            for (int64_t c0 = 0; c0 < p; c0 += 64) {
                const int w = (int)(p - c0 < 64 ? p - c0 : 64);
                const V s = block_colsum<V>(src + (int64_t)i * p, rows, stride, c0, w, red);
                if (t < w && !ended[c0 + t]) {
                    const int64_t o = (int64_t)i * p + c0 + t;
                    coef[o] = s;
                    h[o] = phase == kGmresH1 ? s : h[o] + s;
                }
            }
        }
        return;
    }
    if (phase == kGmresSolve) {
        // R y = g over the first steps[c] unknowns; rows past them are zero
        for (int64_t c = t; c < p; c += kBlock) {
            const int st = fin[c] ? 0 : steps[c];
            for (int i = m - 1; i >= 0; --i) {
                V s = 0;
                if (i < st) {
                    s = g[(int64_t)i * p + c];
                    for (int l = i + 1; l < st; ++l) s = s - R[((int64_t)i * m + l) * p + c] * y[(int64_t)l * p + c];
                    const V d = R[((int64_t)i * m + i) * p + c];
                    s = d != 0 ? s / d : (V)0;
                }
                y[(int64_t)i * p + c] = s;
            }
        }
        return;
    }
    if (t == 0) s_all = 1;
    __syncthreads();
    const bool first = flags[2] == 0;
    for (int64_t c0 = 0; c0 < p; c0 += 64) {
        const int w = (int)(p - c0 < 64 ? p - c0 : 64);
        const V s0 = block_colsum<V>(src, rows, stride, c0, w, red);
        if (t < w) {
            const int64_t c = c0 + t;
            if (phase == kGmresStart) {
                // the true residual decides: beta = |b - A x|
                const V beta = sqrt(s0);
                if (first) {
                    const V rel = reltol * beta;
                    thr[c] = rel > abstol ? rel : abstol;
                    fin[c] = 0;
                    iters[c] = 0;
                }
                if (!fin[c]) {
                    est[c] = beta;
                    hnorm[c] = beta;
                    g[c] = beta;
                    if (beta <= thr[c] || iters[c] >= maxiter) fin[c] = 1;
                }
                ended[c] = fin[c];
                steps[c] = 0;
                if (!fin[c]) atomicAnd(&s_all, 0);
            } else if (!ended[c]) {
                // rotate column j of the Hessenberg matrix, then the right-hand side
                const V hn = sqrt(s0);
                for (int i = 0; i < j; ++i) {
                    const V a = h[(int64_t)i * p + c], b = h[(int64_t)(i + 1) * p + c];
                    const V ci = cs[(int64_t)i * p + c], si = sn[(int64_t)i * p + c];
                    h[(int64_t)i * p + c] = ci * a + si * b;
                    h[(int64_t)(i + 1) * p + c] = ci * b - si * a;
                }
                const V hj = h[(int64_t)j * p + c];
                const V den = sqrt(hj * hj + hn * hn);
                const V cj = den != 0 ? hj / den : (V)1;
                const V sj = den != 0 ? hn / den : (V)0;
                h[(int64_t)j * p + c] = cj * hj + sj * hn;
                for (int i = 0; i <= j; ++i) R[((int64_t)i * m + j) * p + c] = h[(int64_t)i * p + c];
                cs[(int64_t)j * p + c] = cj;
                sn[(int64_t)j * p + c] = sj;
                const V gj = g[(int64_t)j * p + c];
                const V gn = -(sj * gj);
                g[(int64_t)(j + 1) * p + c] = gn;
                g[(int64_t)j * p + c] = cj * gj;
                const V e = fabs(gn);
                est[c] = e;
                hnorm[c] = hn;
                steps[c] = j + 1;
                iters[c] += 1;
                if (e <= thr[c] || hn == 0 || iters[c] >= maxiter) ended[c] = 1;
                if (!ended[c]) atomicAnd(&s_all, 0);
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        if (phase == kGmresStart) {
            flags[2] += 1;
            flags[0] = s_all;
        } else {
            flags[3] += 1;
        }
        flags[1] = s_all;
    }
}

}  // namespace tsgu
