// 2:4 semi-structured operands: prune, expand, A·Yᵀ on the sparse matrix instruction (bf16) or on an expanded image, Aᵀ·G and the
// SDDMM on the kept positions.  Entries and the storage layout: tsgu_hip_semi.h.
//
// An (m, k) operand keeps two of every four consecutive entries of a row: `val` is (m, k/2), the kept entries in column order, and
// `meta` holds one nibble p0 | p1 << 2 (0 <= p0 < p1 <= 3, the kept positions) per group of four.  The nibbles of a row are ordered
// for v_smfmac_f32_16x16x32_bf16 (lane map in mfma_tile.h): the 128 dense columns of one bf16 LDS stage own four dwords, dword q
// (the lane quarter) holds in byte s (the instruction of the stage, its `abid`) the nibbles of the groups 8 s + 2 q (low) and
// 8 s + 2 q + 1 (high), i.e. of the dense columns 32 s + 8 q .. + 8 that lane (r, q) multiplies in instruction s.  A lane's position
// register for a whole stage is ONE dword, a row's four dwords are one 16-byte load.
//
// All products are C[x][y] = sum_t X[x][t]·Y[y][t] on the matrix-core tile layer: two LDS images, 16 x 16 tiles, one MFMA per
// (tile, k step), k ascending.  The sparse instruction reads the compressed image (half the LDS bytes of A) and never touches the
// B elements of a dropped position; the expanding paths write a dense image with zeros there and run the dense step.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

enum { kSemiDenseT = 1, kSemiOutT = 2 };
constexpr int kSemiTile = 64;        // rows and columns of a result tile (Aᵀ·G: 128 x 64)
constexpr int kSemiStage = 128;      // dense columns per block of four position dwords
constexpr int kSemiPadNibble = 0x4;  // (0, 1): the groups past k

__host__ __device__ inline int64_t semi_meta_words(int64_t k) { return 4 * ((k + kSemiStage - 1) / kSemiStage); }

// The position byte of the dense columns 8 c8 .. 8 c8 + 8 of a row (low nibble: the first group).
__device__ __forceinline__ uint32_t semi_byte(const uint32_t* mrow, int64_t c8) {
    const int w = (int)(c8 & 15);
    return (mrow[4 * (c8 >> 4) + (w & 3)] >> (8 * (w >> 2))) & 0xffu;
}

// |w| as an unsigned integer that orders like the magnitude: -0 = +0, every NaN on top (above inf).
__device__ __forceinline__ uint64_t semi_mag(bf16_t w) {
    const uint32_t u = w.bits & 0x7fffu;
    return u > 0x7f80u ? ~0ull : u;
}
__device__ __forceinline__ uint64_t semi_mag(float w) {
    const uint32_t u = __float_as_uint(w) & 0x7fffffffu;
    return u > 0x7f800000u ? ~0ull : u;
}
__device__ __forceinline__ uint64_t semi_mag(double w) {
    const uint64_t u = (uint64_t)__double_as_longlong(w) & 0x7fffffffffffffffull;
    return u > 0x7ff0000000000000ull ? ~0ull : u;
}

// The nibble of one group: the two entries that rank first by (magnitude descending, column ascending).
template <typename V>
__device__ __forceinline__ uint32_t semi_select(const V* w) {
    uint64_t g[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = semi_mag(w[e]);
    int p0 = -1, p1 = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int rank = 0;
#pragma unroll
        for (int o = 0; o < 4; ++o) rank += (g[o] > g[e]) || (g[o] == g[e] && o < e);
        if (rank < 2) {
            if (p0 < 0) p0 = e; else p1 = e;
        }
    }
    return (uint32_t)(p0 | (p1 << 2));
}

template <typename V>
__device__ __forceinline__ V semi_pick(const V* w, int pos) {
    V out = w[0];
#pragma unroll
    for (int e = 1; e < 4; ++e)
        if (pos == e) out = w[e];
    return out;
}

// d[0 .. 8) = the dense columns of one position byte: `v` holds the `cnt` (2 or 4) kept values.
template <typename V>
__device__ __forceinline__ void semi_spread(V (&d)[8], uint32_t byte, const V* v, int cnt) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p0 = (byte >> (4 * h)) & 3, p1 = (byte >> (4 * h + 2)) & 3;
        const bool on = 2 * h < cnt;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[4 * h + e] = on && e == p0 ? v[2 * h] : on && e == p1 ? v[2 * h + 1] : V{};
    }
}

// ---- prune and expand: one thread per position byte (eight dense columns, four kept values) -------------------------------------

template <typename V>
struct SemiConvParams {
    const V* dense_in;      // prune: W (m, k)
    V* dense_out;           // expand: (m, k)
    const V* val_in;        // expand
    V* val_out;             // prune
    uint32_t* meta_out;     // prune
    const uint32_t* meta_in;
    int64_t m, k, ldd, ldv, ldm;
    int64_t units;          // position bytes per row: 4 ldm' = 16 * stages (prune), ceil(k / 8) (expand)
};

template <typename V>
__global__ void __launch_bounds__(kBlock) semi_prune_kernel(SemiConvParams<V> p) {
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= p.m * p.units) return;
    const int64_t row = u / p.units, c8 = u % p.units, c = 8 * c8;
    const int cnt = c + 8 <= p.k ? 8 : c < p.k ? 4 : 0;      // k % 4 == 0
    uint32_t byte = kSemiPadNibble | (kSemiPadNibble << 4);
    if (cnt) {
        V w[8];
        const V* s = p.dense_in + row * p.ldd + c;
        if (cnt == 8 && al16(s)) {
            constexpr int N16 = 8 * (int)sizeof(V) / 16;
            uint4 raw[N16];
#pragma unroll
            for (int j = 0; j < N16; ++j) raw[j] = reinterpret_cast<const uint4*>(s)[j];
            __builtin_memcpy(w, raw, sizeof(w));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = e < cnt ? s[e] : V{};
        }
        V* v = p.val_out + row * p.ldv + c / 2;
        const uint32_t lo = semi_select(w);
        v[0] = semi_pick(w, lo & 3);
        v[1] = semi_pick(w, lo >> 2);
        byte = lo | (kSemiPadNibble << 4);
        if (cnt == 8) {
            const uint32_t hi = semi_select(w + 4);
            v[2] = semi_pick(w + 4, hi & 3);
            v[3] = semi_pick(w + 4, hi >> 2);
            byte = lo | (hi << 4);
        }
    }
    // byte s of dword q of the stage's four (little endian: one byte store, no other thread writes it)
    const int wi = (int)(c8 & 15);
    reinterpret_cast<uint8_t*>(p.meta_out + row * p.ldm + 4 * (c8 >> 4) + (wi & 3))[wi >> 2] = (uint8_t)byte;
}

template <typename V>
__global__ void __launch_bounds__(kBlock) semi_expand_kernel(SemiConvParams<V> p) {
    const int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (u >= p.m * p.units) return;
    const int64_t row = u / p.units, c8 = u % p.units, c = 8 * c8;
    const int cnt = c + 8 <= p.k ? 4 : 2;                     // kept values of this byte (units = ceil(k / 8): c < k)
    const uint32_t byte = semi_byte(p.meta_in + row * p.ldm, c8);
    const V* vs = p.val_in + row * p.ldv + c / 2;
    V v[4], d[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < cnt ? vs[e] : V{};
    semi_spread(d, byte, v, cnt);
    V* o = p.dense_out + row * p.ldd + c;
    if (cnt == 4 && al16(o)) {
        constexpr int N16 = 8 * (int)sizeof(V) / 16;
        uint4 raw[N16];
        __builtin_memcpy(raw, d, sizeof(d));
#pragma unroll
        for (int j = 0; j < N16; ++j) reinterpret_cast<uint4*>(o)[j] = raw[j];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < 2 * cnt) o[e] = d[e];
    }
}

// ---- the expanded LDS image of a tile of A ------------------------------------------------------------------------------------------
// ROWS rows of A from i_base (i_ok of them exist) by CW dense columns from c_base (a multiple of CW; CW divides 128), zeros at the
// dropped positions, past k and past i_ok.  Plain: T[i][c - c_base]; TRANS: T[c - c_base][i].  Reads the compressed bytes only.
template <typename V, int ROWS, int CW, int P, bool TRANS>
__device__ __forceinline__ void semi_expand_tile(V* T, const V* __restrict__ val, const uint32_t* __restrict__ meta, int64_t i_base, int i_ok,
                                                 int64_t c_base, int64_t k, int64_t ldv, int64_t ldm) {
    constexpr int PER_ROW = CW / 8;
    for (int u = threadIdx.x; u < ROWS * PER_ROW; u += kBlock) {
        const int i = u / PER_ROW, c8 = u % PER_ROW;
        const int64_t c = c_base + 8 * c8;
        V d[8];
        if (i < i_ok && c < k) {
            const int cnt = c + 8 <= k ? 4 : 2;
            const uint32_t byte = semi_byte(meta + (i_base + i) * ldm, c >> 3);
            const V* vs = val + (i_base + i) * ldv + (c >> 1);
            V v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = e < cnt ? vs[e] : V{};
            semi_spread(d, byte, v, cnt);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = V{};
        }
        if constexpr (TRANS) {
#pragma unroll
            for (int e = 0; e < 8; ++e) T[(8 * c8 + e) * P + i] = d[e];
        } else {
            constexpr int N16 = 8 * (int)sizeof(V) / 16;
            uint4 raw[N16];
            __builtin_memcpy(raw, d, sizeof(d));
            uint4* dst = reinterpret_cast<uint4*>(T + i * P + 8 * c8);     // (a row's pitch and 8 elements are multiples of 16 bytes)
#pragma unroll
            for (int j = 0; j < N16; ++j) dst[j] = raw[j];
        }
    }
}

// ---- products -------------------------------------------------------------------------------------------------------------------------

template <typename V>
struct SemiParams {
    const V* val;            // (m, k / 2), ldv
    const uint32_t* meta;    // (m, ldm)
    const V* Y;              // the dense operand (mm: Y; mm_t: G; sddmm: Y)
    const V* G;              // sddmm: the cotangent
    const V* bias;           // mm: [m] or NULL
    V* out;
    int64_t m, k, p, ldv, ldm, ldy, ldg, ldo;
    int64_t tiles_x;         // tiles along the result's second tile index
    int flags;
};

// One result element: out[x][y], or out[y][x] when the result is stored transposed.
template <typename V>
__device__ __forceinline__ void semi_store(V* out, int64_t ldo, bool out_t, int64_t x, int64_t y, typename MfmaT<V>::Part a) {
    out[out_t ? y * ldo + x : x * ldo + y] = to_v<V>(a);
}

// The dense operand's image T[row][t] for rows from r0 and t from t0: `src` is (rows, T) with t contiguous, or, transposed, (T, rows).
template <typename V, int ROWS, int P>
__device__ __forceinline__ void semi_stage_dense(V* T, const V* __restrict__ src, bool transposed, int64_t r0, int rows_ok, int64_t t0, int t_ok,
                                                 int64_t ld) {
    constexpr int KC = MfmaT<V>::KC;
    if (transposed) stage_rmajor<V, ROWS, KC, P>(T, src, rows_ok, t_ok, [&](int t) { return (t0 + t) * ld + r0; });
    else stage_kmajor<V, ROWS, KC, P>(T, src, rows_ok, t_ok, [&](int row) { return (r0 + row) * ld + t0; });
}

template <int S>
__device__ __forceinline__ void semi_smfmac_step(mfma_f32x4 (&acc)[4], const bf16_t* Ac, int pc, const uint32_t* Am, const bf16_t* Ys, int py,
                                                 int arow, int r, int q, int n_cnt) {
    const mfma_bf16x4 a = *reinterpret_cast<const mfma_bf16x4*>(Ac + arow * pc + 16 * S + 4 * q);
    const int idx = (int)Am[arow * 4 + q];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
        if (nt < n_cnt) {
            const mfma_bf16x8 b = *reinterpret_cast<const mfma_bf16x8*>(Ys + (16 * nt + r) * py + 32 * S + 8 * q);
            acc[nt] = smfmac_16x16x32(a, b, acc[nt], idx, std::integral_constant<int, S>{});
        }
}

// C[i][n] = sum_c A[i][c]·Y[n][c].  A workgroup owns 64 rows of A by 64 rows of Y; wave w the row tile w and four column tiles.
// SPARSE (bf16): the compressed rows and their position dwords in LDS, v_smfmac; else the expanded image and the dense step.
template <typename V, bool SPARSE>
__global__ void __launch_bounds__(kBlock) semi_mm_kernel(SemiParams<V> p) {
    using AccV = typename MfmaT<V>::Acc;
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>(), TM = kSemiTile, TN = kSemiTile;
    constexpr int PC = KC / 2 + lds_pad<V>();                            // pitch of the compressed image
    __shared__ __attribute__((aligned(16))) V As[SPARSE ? TM * PC : TM * P];
    __shared__ __attribute__((aligned(16))) V Ys[TN * P];
    __shared__ __attribute__((aligned(16))) uint32_t Am[SPARSE ? TM * 4 : 4];
    const int64_t i0 = (blockIdx.x / p.tiles_x) * TM, n0 = (blockIdx.x % p.tiles_x) * TN;
    const int rows = (int)min((int64_t)TM, p.m - i0), cols = (int)min((int64_t)TN, p.p - n0);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1), r = lane & 15, q = lane >> 4;
    const int n_cnt = (cols + 15) / 16;
    AccV acc[1][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[0][nt] = AccV{};
    for (int64_t c0 = 0; c0 < p.k; c0 += KC) {
        if (c0 > 0) __syncthreads();
        const int k_ok = (int)min((int64_t)KC, p.k - c0);
        if constexpr (SPARSE) {
            static_assert(KC == kSemiStage, "one block of position dwords per stage");
            stage_kmajor<V, TM, KC / 2, PC>(As, p.val, rows, k_ok / 2, [&](int row) { return (i0 + row) * p.ldv + c0 / 2; });
            if (threadIdx.x < TM) {
                const int row = threadIdx.x;
                uint4 w = make_uint4(0, 0, 0, 0);
                if (row < rows) w = *reinterpret_cast<const uint4*>(p.meta + (i0 + row) * p.ldm + 4 * (c0 / kSemiStage));
                *reinterpret_cast<uint4*>(Am + 4 * row) = w;
            }
        } else {
            semi_expand_tile<V, TM, KC, P, false>(As, p.val, p.meta, i0, rows, c0, p.k, p.ldv, p.ldm);
        }
        semi_stage_dense<V, TN, P>(Ys, p.Y, p.flags & kSemiDenseT, n0, cols, c0, k_ok, p.ldy);
        __syncthreads();
        if constexpr (SPARSE) {
            const int arow = 16 * wave + r;
            semi_smfmac_step<0>(acc[0], As, PC, Am, Ys, P, arow, r, q, n_cnt);
            if (k_ok > 32) semi_smfmac_step<1>(acc[0], As, PC, Am, Ys, P, arow, r, q, n_cnt);
            if (k_ok > 64) semi_smfmac_step<2>(acc[0], As, PC, Am, Ys, P, arow, r, q, n_cnt);
            if (k_ok > 96) semi_smfmac_step<3>(acc[0], As, PC, Am, Ys, P, arow, r, q, n_cnt);
        } else {
            mfma_step<V, 1, 4>(acc, 0, 1, n_cnt, (k_ok + KS - 1) / KS * KS, [&](int, int c) { return frag_k<V, P>(As, 16 * wave + r, c, q); },
                               [&](int nt, int c) { return frag_k<V, P>(Ys, 16 * nt + r, c, q); });
        }
    }
    const bool out_t = p.flags & kSemiOutT;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t i = i0 + 16 * wave + acc_row<V>(lane, reg), n = n0 + 16 * nt + r;
            if (i < p.m && n < p.p) {
                typename MfmaT<V>::Part a = acc[0][nt][reg];
                if (p.bias) a += VT<V>::up(p.bias[i]);
                semi_store<V>(p.out, p.ldo, out_t, i, n, a);
            }
        }
}

// D[c][n] = sum_i A[i][c]·G[i][n]: A's sparse dimension is an output dimension, so the tile of A is expanded TRANSPOSED and the step
// is dense.  A workgroup owns 128 dense columns of A (one block of position dwords per row) by 64 columns of G; wave w the column
// tiles 2 w, 2 w + 1 of A.  `Y` of the parameters is G: (m, p), or (p, m) with kSemiDenseT.
template <typename V>
__global__ void __launch_bounds__(kBlock) semi_mm_t_kernel(SemiParams<V> p) {
    using AccV = typename MfmaT<V>::Acc;
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>(), TC = kSemiStage, TN = kSemiTile;
    __shared__ __attribute__((aligned(16))) V As[TC * P];
    __shared__ __attribute__((aligned(16))) V Gs[TN * P];
    const int64_t c0 = (blockIdx.x / p.tiles_x) * TC, n0 = (blockIdx.x % p.tiles_x) * TN;
    const int cols = (int)min((int64_t)TN, p.p - n0);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1), r = lane & 15, q = lane >> 4;
    const int n_cnt = (cols + 15) / 16;
    AccV acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = AccV{};
    for (int64_t i0 = 0; i0 < p.m; i0 += KC) {
        if (i0 > 0) __syncthreads();
        const int i_ok = (int)min((int64_t)KC, p.m - i0);
        semi_expand_tile<V, KC, TC, P, true>(As, p.val, p.meta, i0, i_ok, c0, p.k, p.ldv, p.ldm);
        // G's image is [n][i]: the canonical (m, p) operand has n contiguous
        semi_stage_dense<V, TN, P>(Gs, p.Y, !(p.flags & kSemiDenseT), n0, cols, i0, i_ok, p.ldy);
        __syncthreads();
        mfma_step<V, 2, 4>(acc, 0, 2, n_cnt, (i_ok + KS - 1) / KS * KS, [&](int mt, int t) { return frag_k<V, P>(As, 32 * wave + 16 * mt + r, t, q); },
                           [&](int nt, int t) { return frag_k<V, P>(Gs, 16 * nt + r, t, q); });
    }
    const bool out_t = p.flags & kSemiOutT;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t c = c0 + 32 * wave + 16 * mt + acc_row<V>(lane, reg), n = n0 + 16 * nt + r;
                if (c < p.k && n < p.p) semi_store<V>(p.out, p.ldo, out_t, c, n, acc[mt][nt][reg]);
            }
}

// out[i][s] = sum_n G[i][n]·Y[col(i, s)][n]: dense tiles of G·Yᵀ over (rows, dense columns); the epilogue keeps the two positions of
// every group.  G is (m, p) and Y (k, p), or, with kSemiDenseT, (p, m) and (p, k).
template <typename V>
__global__ void __launch_bounds__(kBlock) semi_sddmm_kernel(SemiParams<V> p) {
    using AccV = typename MfmaT<V>::Acc;
    using Part = typename MfmaT<V>::Part;
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>(), TM = kSemiTile, TC = kSemiTile, PS = TC + 1;
    constexpr int kImages = (TM + TC) * P * (int)sizeof(V), kTile = TM * PS * (int)sizeof(Part);
    __shared__ __attribute__((aligned(16))) unsigned char smem[kImages > kTile ? kImages : kTile];
    V* Gs = reinterpret_cast<V*>(smem);
    V* Ys = Gs + TM * P;
    Part* S = reinterpret_cast<Part*>(smem);                           // the result tile, once the images have been multiplied
    const int64_t i0 = (blockIdx.x / p.tiles_x) * TM, c0 = (blockIdx.x % p.tiles_x) * TC;
    const int rows = (int)min((int64_t)TM, p.m - i0), cols = (int)min((int64_t)TC, p.k - c0);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1), r = lane & 15, q = lane >> 4;
    const int n_cnt = (cols + 15) / 16;
    const bool tr = p.flags & kSemiDenseT;
    AccV acc[1][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[0][nt] = AccV{};
    for (int64_t t0 = 0; t0 < p.p; t0 += KC) {
        if (t0 > 0) __syncthreads();
        const int t_ok = (int)min((int64_t)KC, p.p - t0);
        semi_stage_dense<V, TM, P>(Gs, p.G, tr, i0, rows, t0, t_ok, p.ldg);
        semi_stage_dense<V, TC, P>(Ys, p.Y, tr, c0, cols, t0, t_ok, p.ldy);
        __syncthreads();
        mfma_step<V, 1, 4>(acc, 0, 1, n_cnt, (t_ok + KS - 1) / KS * KS, [&](int, int t) { return frag_k<V, P>(Gs, 16 * wave + r, t, q); },
                           [&](int nt, int t) { return frag_k<V, P>(Ys, 16 * nt + r, t, q); });
    }
    __syncthreads();                                                    // the images are dead: their bytes hold the tile now
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) S[(16 * wave + acc_row<V>(lane, reg)) * PS + 16 * nt + r] = acc[0][nt][reg];
    __syncthreads();
    for (int u = threadIdx.x; u < TM * (TC / 4); u += kBlock) {
        const int row = u / (TC / 4), g = u % (TC / 4);
        const int64_t i = i0 + row, c = c0 + 4 * g;
        if (i >= p.m || c >= p.k) continue;
        const uint32_t nib = (semi_byte(p.meta + i * p.ldm, c >> 3) >> (4 * (int)((c >> 2) & 1))) & 15u;
        V* o = p.out + i * p.ldo + (c >> 1);
        o[0] = to_v<V>(S[row * PS + 4 * g + (int)(nib & 3)]);
        o[1] = to_v<V>(S[row * PS + 4 * g + (int)(nib >> 2)]);
    }
}

}  // namespace tsgu
