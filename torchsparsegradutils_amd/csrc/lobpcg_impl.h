// The tall-skinny dense kernels of the LOBPCG loop (tsgu_hip_lobpcg.h): operands are row-major [n][width] views with a leading
// dimension, n in the millions, width <= kTallW = 96 (three blocks of at most kTallK = 32 columns side by side).
//
//   tall_gram_kernel      C = Yᵀ·Z.  The rows are cut into CHUNKS of kTallRows consecutive rows — a property of n alone, not of the
//                         grid.  A workgroup takes chunks at a grid stride; for each it streams the rows through LDS a stage at a
//                         time, and every thread keeps an NT x NT register tile of C (rows ti + 16·ii, columns tj + 16·jj: the LDS
//                         reads of a wave are 4 broadcast addresses of Y and 16 consecutive words of Z, conflict-free).  NT = 1, 2,
//                         3 or 6 is a template argument chosen from the widths (16·NT covers both): the inner loop has no branch,
//                         and a narrow operand is staged 6 / NT times as many rows at a time (192 rows at NT = 1).  Each element is
//                         an fma chain over the rows of a stage, the stages added in ascending order (blocked summation: the error
//                         grows with the stage and the stages per chunk, not with kTallRows), written to partial[chunk].
//   tall_fold_kernel      dst[g] = partial[g·group] + … in ascending order on four interleaved chains, one thread per element: the
//                         launcher folds more than kTallFold partials in two levels (groups of kTallFold, then the groups).  The
//                         grouping depends on the chunk count alone, so the bits do not depend on the grid — no float atomics.
//   tall_combine_kernel   Out_t = beta_t·Out_t + Σ_i S_i·C_ti for up to 6 inputs and 4 outputs in one pass over the rows.  The
//                         (deduplicated) coefficient matrices live in LDS for the whole launch, a tile of rows of every input is
//                         staged beside them; WB = 4, 8, 16 or 32 lanes (a template argument covering the widest block) own a row,
//                         so a tile is (256 / WB)·RPT rows and no lane idles at small k; thread (rr, c) owns column c of RPT rows
//                         and sums over the inputs in ascending (i, j): one staged value per row feeds up to four fmas.
//   residual_kernel       R = AX − X·diag(λ) (a product and a difference: two roundings) and the column sums of squares of R per
//                         chunk, folded as above; WB lanes per row as in the combine.
//
// Plain FMA, not the MFMA tiles of mfma_tile.h: fp32 and fp64 MFMA issue at the vector rate on this chip, so the matrix cores buy
// no FLOPs here; what they would buy is LDS traffic (a wave that keeps its fragments across tiles reads fewer words per fma than
// the 12 words per 36 fmas of the 6 x 6 register tile).  The register tile needs no transposed staging of a [rows][width] operand
// whose k index is the ROW and keeps each element's chain in row order by construction.  An MFMA variant has not been built, so
// the two have not been compared: DESIGN.md §4 says what bounds this kernel and what a variant could gain.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kTallK = 32;        // columns of one block (X, W or P)
constexpr int kTallW = 96;        // columns of an operand of the Gram kernel: three blocks
constexpr int kTallRows = 2048;   // rows of a chunk: one partial tile each
constexpr int kTallFold = 256;    // partials one fold level takes at once
constexpr int kTallIn = 6;        // inputs, outputs and distinct coefficient matrices of one combine
constexpr int kTallOut = 4;
constexpr int kTallCoef = 6;
constexpr int kTallTile = 6;      // side of a thread's register tile of C: 16 x 16 threads x 6 = 96

template <typename V>
constexpr int tall_stage() { return sizeof(V) == 4 ? 32 : 16; }     // rows per LDS stage: 2 x 12 KiB either way

struct GramParams {
    int64_t n, chunks;
    int a, b, same;
    const void* y;
    const void* z;
    int64_t ldy, ldz;
    void* partial;      // [chunks][a·b]
};

// NT: side of a thread's register tile, 16·NT >= both widths (1, 2, 3 or 6: compile time, so the inner loop has no branch).  The
// LDS image of a stage has 16·NT columns, so a narrow operand is staged 6 / NT times as many rows at a time.
template <typename V, int NT>
__global__ __launch_bounds__(kBlock) void tall_gram_kernel(const GramParams P) {
    constexpr int PITCH = 16 * NT;
    constexpr int KS = tall_stage<V>() * (kTallTile / NT);
    static_assert(kTallTile % NT == 0 && KS * PITCH == tall_stage<V>() * kTallW, "a stage fills the same LDS for every NT");
    __shared__ V s_y[KS * PITCH];
    __shared__ V s_z[KS * PITCH];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const V* __restrict__ Y = static_cast<const V*>(P.y);
    const V* __restrict__ Z = static_cast<const V*>(P.z);
    V* __restrict__ partial = static_cast<V*>(P.partial);
    const int a = P.a, b = P.b;
    const V* zs = P.same ? s_y : s_z;
    // columns past the widths stay zero for the whole launch: the stages below write columns < a (< b) only
    for (int v = t; v < KS * PITCH; v += kBlock) {
        s_y[v] = (V)0;
        s_z[v] = (V)0;
    }
    // element v = t + i·kBlock of a [KS][width] stage is (row, column) = (v / width, v % width): stepped, not divided
    const int ya = kBlock / a, yb = kBlock % a, za = kBlock / b, zb = kBlock % b;
    for (int64_t chunk = blockIdx.x; chunk < P.chunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kTallRows;
        const int64_t r1 = r0 + kTallRows < P.n ? r0 + kTallRows : P.n;
        V acc[NT][NT];
#pragma unroll
        for (int ii = 0; ii < NT; ++ii)
#pragma unroll
            for (int jj = 0; jj < NT; ++jj) acc[ii][jj] = (V)0;
        for (int64_t s0 = r0; s0 < r1; s0 += KS) {
            __syncthreads();
            for (int r = t / a, c = t % a; r < KS; r += ya, c += yb) {
                if (c >= a) {
                    c -= a;
                    ++r;
                    if (r >= KS) break;
                }
                s_y[r * PITCH + c] = s0 + r < r1 ? Y[(s0 + r) * P.ldy + c] : (V)0;
            }
            if (!P.same) {
                for (int r = t / b, c = t % b; r < KS; r += za, c += zb) {
                    if (c >= b) {
                        c -= b;
                        ++r;
                        if (r >= KS) break;
                    }
                    s_z[r * PITCH + c] = s0 + r < r1 ? Z[(s0 + r) * P.ldz + c] : (V)0;
                }
            }
            __syncthreads();
            // the stage's rows into a sum of their own, then into the chunk's: chains of KS and kTallRows / KS terms, not of kTallRows
            V part[NT][NT];
#pragma unroll
            for (int ii = 0; ii < NT; ++ii)
#pragma unroll
                for (int jj = 0; jj < NT; ++jj) part[ii][jj] = (V)0;
#pragma unroll 4
            for (int r = 0; r < KS; ++r) {
                V yv[NT], zv[NT];
#pragma unroll
                for (int ii = 0; ii < NT; ++ii) yv[ii] = s_y[r * PITCH + ti + 16 * ii];
#pragma unroll
                for (int jj = 0; jj < NT; ++jj) zv[jj] = zs[r * PITCH + tj + 16 * jj];
#pragma unroll
                for (int ii = 0; ii < NT; ++ii)
#pragma unroll
                    for (int jj = 0; jj < NT; ++jj) part[ii][jj] = fma(yv[ii], zv[jj], part[ii][jj]);
            }
#pragma unroll
            for (int ii = 0; ii < NT; ++ii)
#pragma unroll
                for (int jj = 0; jj < NT; ++jj) acc[ii][jj] += part[ii][jj];
        }
        V* out = partial + chunk * (int64_t)a * b;
#pragma unroll
        for (int ii = 0; ii < NT; ++ii)
#pragma unroll
            for (int jj = 0; jj < NT; ++jj) {
                const int i = ti + 16 * ii, j = tj + 16 * jj;
                if (i < a && j < b) out[i * b + j] = acc[ii][jj];
            }
    }
}

// dst[g][e] = Σ src[p][e] over p in [g·group, min((g + 1)·group, count)), ascending on four interleaved chains.  Element e of a
// [rows][width] tile lands at (e / width)·ld + e % width of the group's destination (`dst_stride` elements apart).
template <typename V>
__global__ __launch_bounds__(kBlock) void tall_fold_kernel(const V* __restrict__ src, int64_t count, int64_t group, int64_t elems,
                                                           V* __restrict__ dst, int64_t dst_stride, int width, int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= elems) return;
    const int64_t g = blockIdx.y;
    const int64_t p0 = g * group;
    const int64_t p1 = p0 + group < count ? p0 + group : count;
    V s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int64_t p = p0;
    for (; p + 3 < p1; p += 4) {
        s0 += src[p * elems + e];
        s1 += src[(p + 1) * elems + e];
        s2 += src[(p + 2) * elems + e];
        s3 += src[(p + 3) * elems + e];
    }
    for (; p < p1; ++p) s0 += src[p * elems + e];
    dst[g * dst_stride + (e / width) * ld + e % width] = (s0 + s1) + (s2 + s3);
}

struct CombineParams {
    int64_t n, tiles;
    int n_in, n_out, n_coef;
    const void* s[kTallIn];
    int64_t s_ld[kTallIn];
    int s_w[kTallIn];
    void* out[kTallOut];
    int64_t out_ld[kTallOut];
    int out_w[kTallOut];
    int has_beta[kTallOut];
    double beta[kTallOut];
    int slot[kTallOut][kTallIn];       // the LDS image C_ti lives in, -1: the block does not contribute
    const void* coef[kTallCoef];
    int64_t coef_ld[kTallCoef];
    int coef_rows[kTallCoef], coef_cols[kTallCoef];
};

template <typename V>
constexpr int combine_rpt() { return sizeof(V) == 4 ? 4 : 1; }      // passes per tile: 24 + 24 KiB of LDS in fp32, 48 + 12 in fp64

// WB: lanes of a row (4, 8, 16 or 32 >= every block's width): kBlock / WB rows per pass, RPT passes per tile, so narrow blocks
// use every lane and take 32 / WB times as many rows per pair of barriers.
template <typename V, int WB>
__global__ __launch_bounds__(kBlock) void tall_combine_kernel(const CombineParams P) {
    constexpr int RPT = combine_rpt<V>();
    constexpr int RPP = kBlock / WB;
    constexpr int TILE = RPP * RPT;
    constexpr int SW = kTallIn * WB;
    __shared__ V s_c[kTallCoef * kTallK * kTallK];
    __shared__ V s_s[TILE * SW];
    const int t = threadIdx.x, rr = t / WB, c = t % WB;
    for (int v = t; v < kTallCoef * kTallK * kTallK; v += kBlock) s_c[v] = (V)0;
    __syncthreads();
    for (int u = 0; u < P.n_coef; ++u) {
        const V* __restrict__ C = static_cast<const V*>(P.coef[u]);
        const int rows = P.coef_rows[u], cols = P.coef_cols[u];
        for (int v = t; v < rows * cols; v += kBlock) {
            const int i = v / cols, j = v - i * cols;
            s_c[u * kTallK * kTallK + i * kTallK + j] = C[i * P.coef_ld[u] + j];
        }
    }
    for (int64_t tile = blockIdx.x; tile < P.tiles; tile += gridDim.x) {
        const int64_t r0 = tile * TILE;
        __syncthreads();
        for (int i = 0; i < P.n_in; ++i) {
            const V* __restrict__ S = static_cast<const V*>(P.s[i]);
            const int w = P.s_w[i];
            if (c < w) {
#pragma unroll
                for (int q = 0; q < RPT; ++q) {
                    const int r = rr + RPP * q;
                    s_s[r * SW + i * WB + c] = r0 + r < P.n ? S[(r0 + r) * P.s_ld[i] + c] : (V)0;
                }
            }
        }
        __syncthreads();
        V acc[RPT][kTallOut];
#pragma unroll
        for (int q = 0; q < RPT; ++q)
#pragma unroll
            for (int o = 0; o < kTallOut; ++o) acc[q][o] = (V)0;
        for (int i = 0; i < P.n_in; ++i) {
            const int w = P.s_w[i];
            int sl[kTallOut];
#pragma unroll
            for (int o = 0; o < kTallOut; ++o) sl[o] = o < P.n_out ? P.slot[o][i] : -1;
            for (int j = 0; j < w; ++j) {
                V sv[RPT];
#pragma unroll
                for (int q = 0; q < RPT; ++q) sv[q] = s_s[(rr + RPP * q) * SW + i * WB + j];
#pragma unroll
                for (int o = 0; o < kTallOut; ++o) {
                    if (sl[o] < 0) continue;
                    const V cv = s_c[sl[o] * kTallK * kTallK + j * kTallK + c];
#pragma unroll
                    for (int q = 0; q < RPT; ++q) acc[q][o] = fma(sv[q], cv, acc[q][o]);
                }
            }
        }
#pragma unroll
        for (int o = 0; o < kTallOut; ++o) {
            if (o >= P.n_out || c >= P.out_w[o]) continue;
            V* __restrict__ O = static_cast<V*>(P.out[o]);
#pragma unroll
            for (int q = 0; q < RPT; ++q) {
                const int64_t row = r0 + rr + RPP * q;
                if (row >= P.n) continue;
                V val = acc[q][o];
                if (P.has_beta[o]) val = fma((V)P.beta[o], O[row * P.out_ld[o] + c], val);
                O[row * P.out_ld[o] + c] = val;
            }
        }
    }
}

struct ResidualParams {
    int64_t n, chunks;
    int k;
    const void* ax;
    const void* x;
    const void* lam;
    void* r;
    int64_t ldax, ldx, ldr;
    void* partial;      // [chunks][k]
};

template <typename V, int WB>
__global__ __launch_bounds__(kBlock) void lobpcg_residual_kernel(const ResidualParams P) {
    constexpr int RPP = kBlock / WB;
    __shared__ V red[kBlock];
    const int t = threadIdx.x, rr = t / WB, c = t % WB;
    const V* __restrict__ AX = static_cast<const V*>(P.ax);
    const V* __restrict__ X = static_cast<const V*>(P.x);
    V* __restrict__ R = static_cast<V*>(P.r);
    V* __restrict__ partial = static_cast<V*>(P.partial);
    const bool live = c < P.k;
    const V lam = live ? static_cast<const V*>(P.lam)[c] : (V)0;
    for (int64_t chunk = blockIdx.x; chunk < P.chunks; chunk += gridDim.x) {
        const int64_t r0 = chunk * kTallRows;
        const int64_t r1 = r0 + kTallRows < P.n ? r0 + kTallRows : P.n;
        V acc = (V)0;
        if (live) {
            for (int64_t row = r0 + rr; row < r1; row += RPP) {
                const V xl = X[row * P.ldx + c] * lam;
                const V rv = AX[row * P.ldax + c] - xl;
                R[row * P.ldr + c] = rv;
                acc = fma(rv, rv, acc);
            }
        }
        __syncthreads();
        red[t] = acc;
        __syncthreads();
        if (rr == 0 && live) {
            V tot = (V)0;
            for (int q = 0; q < RPP; ++q) tot += red[q * WB + c];
            partial[chunk * P.k + c] = tot;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

inline int64_t tall_chunks(int64_t n) { return (n + kTallRows - 1) / kTallRows; }

// partial tiles of `elems` elements for n rows: one per chunk, and one per fold group when a first fold level is needed
inline int64_t tall_partials(int64_t n) {
    const int64_t chunks = tall_chunks(n);
    return chunks + (chunks > kTallFold ? (chunks + kTallFold - 1) / kTallFold : 0);
}

// The partials [chunks][elems] at `partial` (the fold groups follow them) summed into the [elems / width][width] tile at dst.
template <typename V>
inline int tall_fold(V* partial, int64_t chunks, int64_t elems, V* dst, int width, int64_t ld, hipStream_t s) {
    const unsigned bx = (unsigned)((elems + kBlock - 1) / kBlock);
    const V* src = partial;
    int64_t count = chunks;
    if (chunks > kTallFold) {
        const int64_t groups = (chunks + kTallFold - 1) / kTallFold;
        V* mid = partial + chunks * elems;
        hipLaunchKernelGGL(tall_fold_kernel<V>, dim3(bx, (unsigned)groups), dim3(kBlock), 0, s, src, count, (int64_t)kTallFold, elems, mid,
                           elems, (int)elems, elems);
        if (const int rc = check_launch()) return rc;
        src = mid;
        count = groups;
    }
    hipLaunchKernelGGL(tall_fold_kernel<V>, dim3(bx, 1), dim3(kBlock), 0, s, src, count, count, elems, dst, (int64_t)0, width, ld);
    return check_launch();
}

inline int64_t tall_grid(int64_t items, int workgroups, int device) {
    int64_t g = workgroups > 0 ? workgroups : 4 * (int64_t)device_cu_count(device);
    if (g < 1) g = 1;
    return g < items ? g : items;
}

// Do the views [n][w1] at p1 (leading dimension ld1) and [n][w2] at p2 share an element?  Views that interleave in one allocation
// (equal leading dimensions, disjoint column windows) do not; anything else whose address ranges meet counts as shared.
inline bool tall_views_meet(const void* p1, int64_t w1, int64_t ld1, const void* p2, int64_t w2, int64_t ld2, int64_t n, int64_t size) {
    const intptr_t a0 = (intptr_t)p1, a1 = a0 + ((n - 1) * ld1 + w1) * size;
    const intptr_t b0 = (intptr_t)p2, b1 = b0 + ((n - 1) * ld2 + w2) * size;
    if (a1 <= b0 || b1 <= a0) return false;
    if (ld1 != ld2 || (b0 - a0) % size != 0) return true;
    int64_t d = ((b0 - a0) / size) % ld1;
    if (d < 0) d += ld1;
    return !(d >= w1 && d + w2 <= ld1);
}

// f(std::integral_constant<int, WB>{}) for the lanes per row WB = 4, 8, 16 or 32 that cover `width`
template <typename F>
inline int with_row_lanes(int64_t width, F&& f) {
    if (width <= 4) return f(std::integral_constant<int, 4>{});
    if (width <= 8) return f(std::integral_constant<int, 8>{});
    if (width <= 16) return f(std::integral_constant<int, 16>{});
    return f(std::integral_constant<int, 32>{});
}

// f(std::integral_constant<int, NT>{}) for the register tile NT = 1, 2, 3 or 6 with 16·NT >= width
template <typename F>
inline int with_gram_tile(int64_t width, F&& f) {
    if (width <= 16) return f(std::integral_constant<int, 1>{});
    if (width <= 32) return f(std::integral_constant<int, 2>{});
    if (width <= 48) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 6>{});
}

}  // namespace tsgu
