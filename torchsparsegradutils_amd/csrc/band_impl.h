// Banded triangular solves in logarithmic depth (include/tsgu_hip_band.h; entries: band.hip; caller: sparse_banded_solve.py).
//
// T = op(A) is triangular with |row − col| <= W on the solved side, so T x = b is a linear recurrence of order W.  The rows are
// walked in TRAVERSAL order (step g = row for an ascending solve, n − 1 − row for a descending one) and cut into chunks of R
// steps.  The state entering a chunk is the W solutions before it (slot 0: the latest), a W x p block; a chunk maps it affinely,
// S_out = P·S_in + q.  Three phases, every dependency between workgroups a kernel boundary (no flags, no tickets, no waits):
//
//   reduce   band_chunk_kernel, apply = 0: a lane owns (chunk, column).  Columns 0 … p−1 substitute from a zero state with the real
//            right-hand side (q); columns p … p+W−1 from the unit state e_j with a zero right-hand side (column j of P).
//   carry    band_carry_kernel: the chain S_{c+1} = P_c·S_c + q_c over the chunk summaries, by the same reduce / apply over groups
//            of G summaries with a W x W matrix-vector step, recursively, until one workgroup walks what is left.
//   apply    band_chunk_kernel, apply = 1: every chunk substitutes again from its true incoming state and writes X.  Inside a
//            chunk the result is an ordinary substitution in a fixed order (k = 1 … W), whatever R and G are.
//
// Data movement of band_chunk_kernel: a workgroup serves CPB chunks x CT column-lanes.  Strips of S steps of all its chunks are
// copied to LDS in BAND FORM — slot (step, k = |row − col|), zero-filled first, so holes cost nothing and entries on the other side
// of the diagonal fall out — by all 256 threads, one (step, slot) item each and consecutive items on consecutive entries of the
// CSR run (a longer row — entries of the other triangle — is walked with stride W + 1).  Every chunk owns a RING of 2·S + HALO
// steps: the loads of strip s + 1 are issued into registers before strip s is substituted and land in the ring after it, so they
// are in flight during the substitution.  The transposed modes read T[i, i ± k] = A[i ± k, i], slot k of a row visited k steps
// EARLIER: the ring keeps a HALO of W steps behind the strip (and the first strip loads the W steps before the chunk), which is
// all the column-read costs.  The ring's stride per chunk is odd, so lanes of different chunks meet in different banks; lanes of
// one chunk read one address (a broadcast).  A lane's own right-hand-side values need no exchange: they are prefetched to registers.
//
// Non-finite values: a slot that is zero contributes nothing (not 0·inf), in the chunks and in the carry, so a row without a
// diagonal poisons exactly the rows that depend on it.  For that to hold across chunks an entry of P must be non-zero exactly
// when its state row depends on that incoming state: the homogeneous lanes carry W dependency bits beside their values, and a
// dependent entry that has underflowed to zero is stored as the smallest normal number.
#pragma once

#include <cfloat>

#include "tsgu_common.h"

namespace tsgu {

constexpr int kBandMaxW = 8;
constexpr int kBandTile = 64;        // column-lanes of a workgroup at most
constexpr int kBandMaxS = 8;         // steps of a strip at most (a lane prefetches that many right-hand-side values)
constexpr int kBandItems = 6;        // (step, slot) items a thread keeps in flight per strip
constexpr int kBandLds = 64 * 1024;  // per workgroup: two fit a CU's 160 KiB
constexpr int kBandMaxLevels = 48;

struct BandParams {
    int64_t n, nnz, nch;
    const void *ptr, *idx, *val, *B;
    void* X;
    int64_t ldb, ldx;
    void* sum;            // reduce: [nch][W][p + W]
    const void* st;       // apply: [nch][W][p]
    int p, ncols, a_lower, unit, apply, R;
    int S, CT, CPB, NR, bstride;
};

struct BandCarryParams {
    const void* src;      // [m][W][p + W]
    void* dst;            // reduce: [ng][W][p + W]
    const void* st_up;    // apply: [ng][W][p], NULL: a zero state
    void* st;             // apply: [m][W][p], the state ENTERING every element
    int64_t m, ng, G;
    int p, apply;
};

template <typename V>
__device__ __forceinline__ V band_min_normal();
template <>
__device__ __forceinline__ float band_min_normal<float>() { return FLT_MIN; }
template <>
__device__ __forceinline__ double band_min_normal<double>() { return DBL_MIN; }

// the summary of a homogeneous column: a dependent entry is never stored as zero
template <typename V>
__device__ __forceinline__ V band_summary(V v, bool homogeneous, unsigned dep, int i) {
    return (homogeneous && (dep >> i & 1u) && v == V(0)) ? band_min_normal<V>() : v;
}

template <typename V, typename I, int W, bool ASC, bool COLREAD>
__global__ __launch_bounds__(kBlock) void band_chunk_kernel(const BandParams P) {
    constexpr int HALO = COLREAD ? W : 0;
    constexpr int W1 = W + 1;
    extern __shared__ __align__(16) unsigned char band_smem[];
    V* band = reinterpret_cast<V*>(band_smem);
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* __restrict__ B = static_cast<const V*>(P.B);
    V* __restrict__ X = static_cast<V*>(P.X);
    const int tid = threadIdx.x;
    const int S = P.S, CT = P.CT, CPB = P.CPB, NR = P.NR, R = P.R, bstride = P.bstride;
    const int64_t n = P.n, chunk0 = (int64_t)blockIdx.x * CPB;
    const int lo_unit = P.unit ? 1 : 0;

    // ---- staging: items (chunk, step, slot) of the steps [lo, lo + cnt) of every chunk of the workgroup ------------------------
    // the ring slot base of an item and its row; false when the step is not a row of the matrix (or not of this chunk's walk)
    auto item = [&](int it, int lo, int cnt, int& base, int& j, int64_t& row) -> bool {
        j = it % W1;
        const int q = it / W1, r = q % cnt, cl = q / cnt;
        const int step = lo + r;
        base = cl * bstride + ((step + HALO) % NR) * W1;          // (it < CPB·cnt·W1 at every call: cl < CPB)
        const int64_t c = chunk0 + cl, g = c * R + step;
        row = ASC ? g : n - 1 - g;
        return c < P.nch && step < R && g >= 0 && g < n;
    };
    // the entries e, e + W1, … of `row` into their slots
    auto scatter = [&](int base, int64_t row, int64_t e, int64_t end) {
        for (; e < end; e += W1) {
            const int64_t c = (int64_t)idx[e], k = P.a_lower ? row - c : c - row;
            if (k >= lo_unit && k <= W) band[base + (int)k] = val[e];
        }
    };
    auto row_end = [&](int64_t row) {
        const int64_t end = (int64_t)ptr[row + 1];
        return end < P.nnz ? end : P.nnz;
    };
    auto zero_fill = [&](int lo, int cnt) {
        const int total = CPB * cnt * W1;
        for (int it = tid; it < total; it += kBlock) {
            int base, j;
            int64_t row;
            item(it, lo, cnt, base, j, row);
            band[base + j] = V(0);
        }
    };
    auto fill_direct = [&](int lo, int cnt, int first) {
        const int total = CPB * cnt * W1;
        for (int it = first + tid; it < total; it += kBlock) {
            int base, j;
            int64_t row;
            if (item(it, lo, cnt, base, j, row)) scatter(base, row, (int64_t)ptr[row] + j, row_end(row));
        }
    };

    // ---- the lane: (chunk, column) -------------------------------------------------------------------------------------------------
    const int cl = tid / CT, cc = tid % CT;
    const int64_t chunk = chunk0 + cl;
    const int col = blockIdx.y * CT + cc;
    const bool lane = cl < CPB && chunk < P.nch && col < P.ncols;
    const bool real = col < P.p;
    const int64_t g0 = chunk * R;
    const int len = lane ? (int)((n - g0) < R ? (n - g0) : R) : 0;
    V s[W];
    unsigned dep = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) s[i] = V(0);
    if (lane && P.apply) {
        const V* st = static_cast<const V*>(P.st) + (chunk * W) * P.p + col;
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] = st[(int64_t)i * P.p];
    } else if (lane && !real) {
        dep = 1u << (col - P.p);
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] = (i == col - P.p) ? V(1) : V(0);
    }
    auto load_rhs = [&](int strip, V (&b)[kBandMaxS]) {
#pragma unroll
        for (int r = 0; r < kBandMaxS; ++r) {
            const int step = strip * S + r;
            b[r] = V(0);
            if (r < S && real && step < len) {
                const int64_t g = g0 + step;
                b[r] = B[(ASC ? g : n - 1 - g) * P.ldb + col];
            }
        }
    };

    // ---- prologue: the halo and strip 0, directly ---------------------------------------------------------------------------------
    zero_fill(-HALO, S + HALO);
    __syncthreads();
    fill_direct(-HALO, S + HALO, 0);
    V bcur[kBandMaxS], bnext[kBandMaxS];
    load_rhs(0, bcur);
    __syncthreads();

    const int nstrips = (R + S - 1) / S;
    for (int strip = 0; strip < nstrips; ++strip) {
        // (1) strip + 1: clear its ring slots and issue its loads into registers
        const bool more = strip + 1 < nstrips;
        const int lo = (strip + 1) * S;
        V rv[kBandItems];
        int rslot[kBandItems];          // the LDS slot of the prefetched entry, −1: nothing to store
        unsigned tail = 0;              // bit u: the row of item u has further entries for this thread (walked after the strip)
        if (more) {
            zero_fill(lo, S);
            const int total = CPB * S * W1;
#pragma unroll
            for (int u = 0; u < kBandItems; ++u) {
                const int it = tid + u * kBlock;
                rslot[u] = -1;
                rv[u] = V(0);
                int base, j;
                int64_t row;
                if (it < total && item(it, lo, S, base, j, row)) {
                    const int64_t e = (int64_t)ptr[row] + j, end = row_end(row);
                    if (e < end) {
                        const int64_t c = (int64_t)idx[e], k = P.a_lower ? row - c : c - row;
                        if (k >= lo_unit && k <= W) {
                            rslot[u] = base + (int)k;
                            rv[u] = val[e];
                        }
                        if (e + W1 < end) tail |= 1u << u;
                    }
                }
            }
            load_rhs(strip + 1, bnext);
        }
        // (2) substitute strip `strip`
        if (lane) {
            int rp = (strip * S + HALO) % NR;
#pragma unroll
            for (int r = 0; r < kBandMaxS; ++r) {
                const int step = strip * S + r;
                if (r < S && step < len) {
                    const V* rowp = band + cl * bstride + rp * W1;
                    const V d = P.unit ? V(1) : rowp[0];
                    V acc = V(0);
                    unsigned bit = 0;
#pragma unroll
                    for (int k = 1; k <= W; ++k) {
                        int q = rp - k;
                        q += q < 0 ? NR : 0;
                        const V c = COLREAD ? band[cl * bstride + q * W1 + k] : rowp[k];
                        const V t = c * s[k - 1];
                        acc = c != V(0) ? acc + t : acc;
                        bit |= c != V(0) ? (dep >> (k - 1) & 1u) : 0u;
                    }
                    const V x = (bcur[r] - acc) / d;
#pragma unroll
                    for (int i = W - 1; i > 0; --i) s[i] = s[i - 1];
                    s[0] = x;
                    dep = (dep << 1 | bit) & ((1u << W) - 1u);
                    if (P.apply) {
                        const int64_t g = g0 + step;
                        X[(ASC ? g : n - 1 - g) * P.ldx + col] = x;
                    }
                }
                rp = rp + 1 == NR ? 0 : rp + 1;
            }
        }
        // (3) land strip + 1 in the ring (behind the zero fill), then whatever was not prefetched
        __syncthreads();
        if (more) {
#pragma unroll
            for (int u = 0; u < kBandItems; ++u) {
                if (rslot[u] >= 0) band[rslot[u]] = rv[u];
                if (tail >> u & 1u) {
                    int base, j;
                    int64_t row;
                    if (item(tid + u * kBlock, lo, S, base, j, row)) scatter(base, row, (int64_t)ptr[row] + j + W1, row_end(row));
                }
            }
            fill_direct(lo, S, kBandItems * kBlock);
#pragma unroll
            for (int r = 0; r < kBandMaxS; ++r) bcur[r] = bnext[r];
        }
        __syncthreads();
    }

    if (lane && !P.apply) {
        V* sum = static_cast<V*>(P.sum) + (chunk * W) * P.ncols + col;
#pragma unroll
        for (int i = 0; i < W; ++i) sum[(int64_t)i * P.ncols] = band_summary(s[i], !real, dep, i);
    }
}

// The chain over summaries: lane = (group, column).  reduce: from the zero / unit state over the group's G summaries → the group's
// summary; apply: from the group's true incoming state, leaving the state that enters every summary of the group.
template <typename V, int W>
__global__ __launch_bounds__(kBlock) void band_carry_kernel(const BandCarryParams Q) {
    const int pc = Q.p + W, ncols = Q.apply ? Q.p : pc;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t g = gid / ncols;
    const int col = (int)(gid % ncols);
    if (g >= Q.ng) return;
    const bool real = col < Q.p;
    const V* __restrict__ src = static_cast<const V*>(Q.src);
    V s[W];
    unsigned dep = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) s[i] = V(0);
    if (Q.apply) {
        if (Q.st_up) {
            const V* up = static_cast<const V*>(Q.st_up) + (g * W) * Q.p + col;
#pragma unroll
            for (int i = 0; i < W; ++i) s[i] = up[(int64_t)i * Q.p];
        }
    } else if (!real) {
        dep = 1u << (col - Q.p);
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] = (i == col - Q.p) ? V(1) : V(0);
    }
    const int64_t c1 = (g + 1) * Q.G < Q.m ? (g + 1) * Q.G : Q.m;
    for (int64_t c = g * Q.G; c < c1; ++c) {
        if (Q.apply) {
            V* st = static_cast<V*>(Q.st) + (c * W) * Q.p + col;
#pragma unroll
            for (int i = 0; i < W; ++i) st[(int64_t)i * Q.p] = s[i];
        }
        const V* Pc = src + (c * W) * pc;
        V t[W];
        unsigned nd = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            V acc = real ? Pc[(int64_t)i * pc + col] : V(0);
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const V a = Pc[(int64_t)i * pc + Q.p + j];
                const V prod = a * s[j];
                acc = a != V(0) ? acc + prod : acc;
                nd |= (a != V(0) && (dep >> j & 1u)) ? 1u << i : 0u;
            }
            t[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < W; ++i) s[i] = t[i];
        dep = nd;
    }
    if (!Q.apply) {
        V* dst = static_cast<V*>(Q.dst) + (g * W) * pc + col;
#pragma unroll
        for (int i = 0; i < W; ++i) dst[(int64_t)i * pc] = band_summary(s[i], !real, dep, i);
    }
}

// ---- host: geometry (pure functions of n, p, w and the value type) ---------------------------------------------------------------
struct BandLevels {
    int Wt, R, G, top, L;
    int64_t m[kBandMaxLevels];
};

inline int band_template_width(int w) { return w <= 1 ? 1 : w <= 2 ? 2 : w <= 4 ? 4 : 8; }

// false: arguments out of range
inline bool band_levels(int64_t n, int w, int chunk_rows, int group_chunks, BandLevels& lv) {
    if (n < 0 || w < 0 || w > kBandMaxW || chunk_rows < 0 || group_chunks < 0 || group_chunks == 1) return false;
    lv.Wt = band_template_width(w);
    lv.R = chunk_rows ? chunk_rows : (n >= (int64_t(1) << 18) ? 64 : 32);
    lv.G = group_chunks ? group_chunks : 32;
    lv.top = 8 * lv.G;
    lv.L = 1;
    lv.m[0] = (n + lv.R - 1) / lv.R;
    while (lv.m[lv.L - 1] > lv.top) {
        if (lv.L == kBandMaxLevels) return false;
        lv.m[lv.L] = (lv.m[lv.L - 1] + lv.G - 1) / lv.G;
        ++lv.L;
    }
    return true;
}

inline int64_t band_work_values(const BandLevels& lv, int64_t p) {
    int64_t v = 0;
    for (int l = 0; l < lv.L; ++l) v += lv.m[l] * lv.Wt * (2 * p + lv.Wt);
    return v;
}

// the launch shape of band_chunk_kernel for `ncols` column-lanes per chunk: column-lanes and chunks of a workgroup, the strip
// and the ring that fit the LDS budget and the in-flight items of a thread
inline void band_shape(BandParams& P, int Wt, bool colread, int vbytes) {
    const int W1 = Wt + 1, halo = colread ? Wt : 0;
    int CT = 1;
    while (CT < kBandTile && CT < P.ncols) CT *= 2;
    int CPB = kBlock / CT, S = kBandMaxS;
    auto lds = [&] { return (int64_t)CPB * (((2 * S + halo) * W1) | 1) * vbytes; };
    while (S > 1 && (lds() > kBandLds || CPB * S * W1 > kBandItems * kBlock)) S /= 2;
    while (CPB > 1 && lds() > kBandLds) CPB /= 2;
    if (S > P.R) S = P.R > 1 ? (P.R >= 8 ? 8 : P.R >= 4 ? 4 : P.R >= 2 ? 2 : 1) : 1;
    P.CT = CT;
    P.CPB = CPB;
    P.S = S;
    P.NR = 2 * S + halo;
    P.bstride = (P.NR * W1) | 1;
}

}  // namespace tsgu
