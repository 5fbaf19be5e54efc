// The k largest of scale·Q·Kᵀ + key_bias per row, straight into CSR arrays: a flash-style product on the matrix cores whose epilogue is
// a running per-row selection instead of a softmax.  The scores live in registers and LDS only.  Entries: tsgu_hip_topk.h.
//
// A workgroup owns R = 16·MT query rows and walks the keys in tiles of 64, ascending; its four waves take 16 keys each.  A score
// tile is C[row][key] = sum_t Q[row][t]·K[key][t] on 16 x 16 MFMA tiles over LDS stages of KC columns (zero-filled tails): the lane
// maps, the staging and the MFMA step are the matrix-core tile layer's (mfma_tile.h).  Q stays staged when d fits one stage.
//
// The selection is "keep the best k, replace the worst".  Every row has k slots in LDS (initially a sentinel that loses to every
// score) and the key of its worst entry as the row's threshold.  The order is total: key(score) (an unsigned
// integer, monotone in the score, -0 = +0, NaN on top), then the LOWER column.  Keys arrive in ascending column order, so a later
// score that merely equals the threshold has lost already: the filter on the per-score path is one integer compare per score.
//   filter   a lane whose score beats its row's threshold takes a slot of the row's pending list (one LDS add) and stores
//            (score, column).  At most 64 per row and tile: the list cannot overflow.  No barrier, no loop.
//   drain    after the tile's barrier a wave takes the pending lists of its own R / 4 rows, a row's slots and one candidate per lane in
//            registers: the candidates that do not beat the worst entry drop out together (one ballot); one that does replaces it,
//            and the worst entry is found again (a DPP / v_readlane reduction, no LDS traffic) before the next.  A row with an empty
//            list costs one load.  The result does not depend on the order of the list: the best k of a set.
//   output   a row's stored entries are ranked by column (k loads per lane) and written ascending at the offsets crow gives.
// Nothing waits for another workgroup, nothing is summed across lanes: the same bits on every run.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

constexpr int kTopkCap = 128;                 // the largest k
constexpr int kTopkKeys = 64;                 // keys per tile: 16 per wave
constexpr int kTopkMaxLds = 80 * 1024;        // two workgroups per CU at the largest k
constexpr int kTopkNoCol = 0x7fffffff;        // the column of a sentinel (m is below it)
enum { kTopkCausal = 1, kTopkExcludeSelf = 2 };

// row tiles of 16 per workgroup: what leaves the selection's LDS of the largest k below kTopkMaxLds
template <typename V>
struct TopkG {
    static constexpr int MT = 2;
};
template <>
struct TopkG<double> {
    static constexpr int MT = 1;
};

// The order of the scores as an unsigned integer: greater is better.  -0 counts as +0, every NaN is the one largest key; the key of
// -inf is above 0, the sentinel's.
__device__ __forceinline__ uint32_t topk_key(float s) {
    if (s != s) return 0xffffffffu;
    const uint32_t u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t topk_key(double s) {
    if (s != s) return ~0ull;
    const uint64_t u = (uint64_t)__double_as_longlong(s + 0.0);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
template <typename A>
struct TopkKeyT {
    using U = decltype(topk_key(A{}));
};

template <typename V>
struct TopkParams {
    using Acc = typename MfmaT<V>::Part;
    const V* Q;              // [batch][n][d]
    const V* K;              // [batch][m][d]
    const V* bias;           // [batch][m] or NULL
    const void* crow;        // [n + 1], shared by the batch items
    void* col;               // [batch][nnz]
    V* val;                  // [batch][nnz]
    int64_t n, m, d;
    int64_t off;             // causal: column j of row i is allowed when j <= i + off
    int64_t q_stride, k_stride, bias_stride, out_stride;
    int64_t tiles;           // workgroups per batch item
    int k, flags;
    Acc scale;
};

template <typename V>
struct TopkLds {
    using Acc = typename MfmaT<V>::Part;
    using U = typename TopkKeyT<Acc>::U;
    static constexpr int MT = TopkG<V>::MT, R = 16 * MT, T = kTopkKeys, KC = MfmaT<V>::KC, P = mfma_pitch<V>();
    static constexpr int kQ = R * P * (int)sizeof(V), kK = T * P * (int)sizeof(V);
    static_assert(kQ % 16 == 0 && kK % 16 == 0, "16-byte images");
    // images, then per row: k + T scores, k + T columns, the worst entry's pair and the pending count
    static constexpr int bytes(int k) { return kQ + kK + R * ((k + T) * ((int)sizeof(Acc) + 4) + (int)sizeof(U) + 8); }
    static_assert(bytes(kTopkCap) <= kTopkMaxLds, "two workgroups per CU at the largest k");
};

// Orders one wave's plain LDS accesses for the compiler (the hardware serves a wave's LDS operations in order).
__device__ __forceinline__ void topk_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Words across the lanes of a wave without LDS traffic: DPP inside a row of 16 lanes, v_readlane for a uniform lane.
template <int CTRL>
__device__ __forceinline__ uint32_t topk_dpp(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ uint64_t topk_dpp(uint64_t x) {
    return ((uint64_t)topk_dpp<CTRL>((uint32_t)(x >> 32)) << 32) | topk_dpp<CTRL>((uint32_t)x);
}
__device__ __forceinline__ uint32_t topk_lane(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }
__device__ __forceinline__ uint64_t topk_lane(uint64_t x, int l) {
    return ((uint64_t)topk_lane((uint32_t)(x >> 32), l) << 32) | topk_lane((uint32_t)x, l);
}
__device__ __forceinline__ float topk_lane(float x, int l) { return __uint_as_float(topk_lane(__float_as_uint(x), l)); }
__device__ __forceinline__ double topk_lane(double x, int l) { return __longlong_as_double((long long)topk_lane((uint64_t)__double_as_longlong(x), l)); }

// An entry in the order of the selection: (key of the score, kTopkNoCol - column), compared as a pair; the lower one is the worse.
// A sentinel is (0, 0), below every score; a slot past k is (all ones, 2^31), above every entry.
template <typename U>
__device__ __forceinline__ bool topk_below(U ka, uint32_t na, U kb, uint32_t nb) {
    return ka < kb || (ka == kb && na < nb);
}

// The lowest (k, n) of the wave in every lane: an all-reduce over the rows of 16 by DPP, the four rows by v_readlane.
template <typename U>
__device__ __forceinline__ void topk_wave_min(U& k, uint32_t& n) {
    auto fold = [&](U ok, uint32_t on) {
        if (topk_below(ok, on, k, n)) {
            k = ok;
            n = on;
        }
    };
    fold(topk_dpp<0xB1>(k), topk_dpp<0xB1>(n));         // lanes i ^ 1
    fold(topk_dpp<0x4E>(k), topk_dpp<0x4E>(n));         // i ^ 2
    fold(topk_dpp<0x141>(k), topk_dpp<0x141>(n));       // 7 - i
    fold(topk_dpp<0x140>(k), topk_dpp<0x140>(n));       // 15 - i
    const U k1 = topk_lane(k, 16), k2 = topk_lane(k, 32), k3 = topk_lane(k, 48);
    const uint32_t n1 = topk_lane(n, 16), n2 = topk_lane(n, 32), n3 = topk_lane(n, 48);
    k = topk_lane(k, 0);
    n = topk_lane(n, 0);
    fold(k1, n1);
    fold(k2, n2);
    fold(k3, n3);
}

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) topk_mm_kernel(TopkParams<V> p) {
    using L = TopkLds<V>;
    using Acc = typename MfmaT<V>::Part;
    using AccV = typename MfmaT<V>::Acc;
    using U = typename L::U;
    constexpr int MT = L::MT, R = L::R, T = L::T, KC = L::KC, P = L::P, KS = MfmaT<V>::KS, RPW = R / 4, SL = kTopkCap / kWave;
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
    const int k = p.k;
    unsigned char* sm = topk_smem;
    V* Qs = reinterpret_cast<V*>(sm);
    sm += L::kQ;
    V* Ks = reinterpret_cast<V*>(sm);
    sm += L::kK;
    Acc* ent_s = reinterpret_cast<Acc*>(sm);          // [R][k]
    Acc* pend_s = ent_s + R * k;                      // [R][T]
    U* thr = reinterpret_cast<U*>(pend_s + R * T);    // [R]
    int* ent_c = reinterpret_cast<int*>(thr + R);     // [R][k]
    int* pend_c = ent_c + R * k;                      // [R][T]
    uint32_t* thr_n = reinterpret_cast<uint32_t*>(pend_c + R * T);      // [R]: with thr the worst entry as the pair of topk_below
    int* pend_n = reinterpret_cast<int*>(thr_n + R);  // [R]

    const int64_t b = blockIdx.x / p.tiles;
    const int64_t row0 = (blockIdx.x % p.tiles) * R;
    const int rows = (int)min((int64_t)R, p.n - row0);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const V* Qb = p.Q + b * p.q_stride;
    const V* Kb = p.K + b * p.k_stride;
    const V* bias = p.bias ? p.bias + b * p.bias_stride : nullptr;
    const bool causal = p.flags & kTopkCausal, no_self = p.flags & kTopkExcludeSelf;

    for (int e = threadIdx.x; e < R * k; e += kBlock) {
        ent_s[e] = (Acc)0;
        ent_c[e] = kTopkNoCol;
    }
    for (int e = threadIdx.x; e < R; e += kBlock) {
        thr[e] = 0;
        thr_n[e] = 0;
        pend_n[e] = 0;
    }
    // (a sentinel's score is never read as one: its column marks it)

    // keys any row of the tile may take
    int64_t j_end = p.m;
    if (causal) j_end = max((int64_t)0, min(p.m, row0 + rows + p.off));
    const bool q_stays = p.d <= KC;
    auto stage_q = [&](int64_t c0) {
        stage_kmajor<V, R, KC, P>(Qs, Qb, rows, (int)min((int64_t)KC, p.d - c0), [&](int row) { return (row0 + row) * p.d + c0; });
    };
    if (q_stays) stage_q(0);

    for (int64_t j0 = 0; j0 < j_end; j0 += T) {
        AccV acc[MT][1];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][0] = AccV{};
        const int64_t j = j0 + 16 * wave + r;         // this lane's key
        const bool key_ok = j < p.m;
        const Acc bj = bias && key_ok ? (Acc)VT<V>::up(bias[j]) : (Acc)0;
        for (int64_t c0 = 0; c0 < p.d; c0 += KC) {
            if (c0 > 0) __syncthreads();           // the previous stage has been multiplied
            const int k_ok = (int)min((int64_t)KC, p.d - c0);
            if (!q_stays) stage_q(c0);
            stage_kmajor<V, T, KC, P>(Ks, Kb, (int)min((int64_t)T, p.m - j0), k_ok, [&](int row) { return (j0 + row) * p.d + c0; });
            __syncthreads();
            mfma_step<V, MT, 1>(acc, 0, MT, 1, (k_ok + KS - 1) / KS * KS, [&](int mt, int c) { return frag_k<V, P>(Qs, 16 * mt + r, c, q); },
                                [&](int, int c) { return frag_k<V, P>(Ks, 16 * wave + r, c, q); });
        }
        {   // the filter: this lane's key against the thresholds of its 4·MT rows
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = 16 * mt + acc_row<V>(lane, reg);
                    const int64_t i = row0 + row;
                    Acc s = p.scale * acc[mt][0][reg];
                    if (bias) s += bj;
                    const bool allowed = key_ok && row < rows && (!causal || j <= i + p.off) && (!no_self || j != i);
                    if (allowed && topk_key(s) > thr[row]) {
                        const int at = atomicAdd(&pend_n[row], 1);      // < T: a row meets a key once
                        pend_s[row * T + at] = s;
                        pend_c[row * T + at] = (int)j;
                    }
                }
        }
        __syncthreads();
        // the drain: this wave's rows.  A lane holds the row's slots lane, lane + 64 and one pending candidate in registers; the
        // candidates that do not beat the worst entry drop out together, the others go in one at a time.
        for (int row = wave * RPW; row < (wave + 1) * RPW; ++row) {
            const int pn = pend_n[row];
            if (pn == 0) continue;
            Acc* es = ent_s + row * k;
            int* ec = ent_c + row * k;
            U ek[SL];
            uint32_t en[SL];
#pragma unroll
            for (int s = 0; s < SL; ++s) {
                const int e = lane + kWave * s;
                ek[s] = ~(U)0;
                en[s] = 0x80000000u;
                if (e < k) {
                    const int c = ec[e];
                    en[s] = (uint32_t)(kTopkNoCol - c);
                    ek[s] = c == kTopkNoCol ? (U)0 : topk_key(es[e]);
                }
            }
            const bool has = lane < pn;
            const Acc cs = has ? pend_s[row * T + lane] : (Acc)0;
            const int cc = has ? pend_c[row * T + lane] : 0;
            const U ck = topk_key(cs);
            const uint32_t cn = (uint32_t)(kTopkNoCol - cc);
            U wk = thr[row];
            uint32_t wn = thr_n[row];
            auto worst = [&]() {
                wk = ek[0];
                wn = en[0];
#pragma unroll
                for (int s = 1; s < SL; ++s)
                    if (topk_below(ek[s], en[s], wk, wn)) {
                        wk = ek[s];
                        wn = en[s];
                    }
                topk_wave_min(wk, wn);
            };
            uint64_t live = __ballot(has && topk_below(wk, wn, ck, cn));
            while (live) {
                const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(live));
                const Acc bs = topk_lane(cs, src);
                const U bk = topk_lane(ck, src);
                const uint32_t bn = topk_lane(cn, src);
                int slot = -1;                        // the worst entry's slot, in the first lane that holds one like it
#pragma unroll
                for (int s = SL - 1; s >= 0; --s)
                    if (ek[s] == wk && en[s] == wn) slot = s;
                const uint64_t owners = __ballot(slot >= 0);
                if (lane == __builtin_ctzll(owners)) {
#pragma unroll
                    for (int s = 0; s < SL; ++s)
                        if (s == slot) {
                            ek[s] = bk;
                            en[s] = bn;
                        }
                    es[lane + kWave * slot] = bs;
                    ec[lane + kWave * slot] = kTopkNoCol - (int)bn;
                }
                worst();
                live &= __ballot(has && topk_below(wk, wn, ck, cn)) & ~(1ull << src);
            }
            if (lane == 0) {
                thr[row] = wk;
                thr_n[row] = wn;
                pend_n[row] = 0;
            }
            topk_wave_sync();
        }
    }
    if (j_end <= 0) __syncthreads();                   // (the slots were initialised by other waves)

    // output: this wave's rows, columns ascending
    I* out_c = static_cast<I*>(p.col) + b * p.out_stride;
    V* out_v = p.val + b * p.out_stride;
    for (int row = wave * RPW; row < (wave + 1) * RPW; ++row) {
        if (row >= rows) break;
        const int64_t at = ld_idx<I>(p.crow, row0 + row);
        const int64_t cnt = ld_idx<I>(p.crow, row0 + row + 1) - at;
        const Acc* es = ent_s + row * k;
        const int* ec = ent_c + row * k;
        for (int e = lane; e < k; e += kWave) {
            const int ce = ec[e];
            if (ce == kTopkNoCol) continue;
            int rank = 0;
            for (int o = 0; o < k; ++o) rank += ec[o] < ce;
            if (rank < cnt) {
                out_c[at + rank] = (I)ce;
                out_v[at + rank] = to_v<V>(es[e]);
            }
        }
    }
}

template <typename V, typename I>
int topk_launch(const TopkParams<V>& P, int64_t grid, hipStream_t s) {
    return launch_large_lds<topk_mm_kernel<V, I>>(current_device(), grid, kBlock, TopkLds<V>::bytes(P.k), kTopkMaxLds, s, P);
}

}  // namespace tsgu
