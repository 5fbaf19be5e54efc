// The matrix-core tile layer: what the kernels that multiply on the MFMA units share (indexed_mm_impl.h, bsr_impl.h,
// bsr_attention_impl.h, topk_impl.h, semi_impl.h).  Every product is C[m][n] = sum_k X[m][k] * Y[n][k] over two LDS images, each row with one 16-byte pad, on
// 16 x 16 tiles.  MFMA lane maps (cdna_hip_programming.md §3), lane l = (r, q) = (l & 15, l >> 4):
//   f32  16x16x4f32:  lane l holds X[r][k0 + q] and Y[r][k0 + q];              C: col = r, row = 4 q + reg
//   f64  16x16x4f64:  A/B as f32;                                             C: col = r, row = q + 4 reg
//   bf16 16x16x32:    lane l holds X[r][k0 + 8 q + j], j < 8 (and Y alike);    C as f32
// The f32 form is bit for bit a k-ordered fmaf chain; the bf16 form multiplies exactly and accumulates in fp32.
// The 2:4 sparse form v_smfmac_f32_16x16x32_bf16 (smfmac_16x16x32 below; established with one-hot operands, all 64 lanes x 4
// elements x 4 position values x 4 abid agree, EXPERIMENTS.md §32):
//   X is compressed: lane l holds the FOUR kept values e = 0 .. 3 of X[r][k0 + 8 q .. + 8): e = 0, 1 belong to the group of four
//   dense k at k0 + 8 q, e = 2, 3 to the group at k0 + 8 q + 4, each pair in ascending k.  Y and C are those of the dense bf16 form.
//   idx: with cbsz = 0 the instruction reads byte `abid` (0 .. 3) of the lane's own idx register; bits [2 e + 1 : 2 e] of that byte
//   are the position of value e INSIDE its group, so value e multiplies Y[n][k0 + 8 q + 4 (e / 2) + bits].  The other three
//   bytes are ignored: one register serves the four instructions of a 128-wide stage.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

typedef __bf16 mfma_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));
typedef double mfma_f64x4 __attribute__((ext_vector_type(4)));

template <typename V>
struct MfmaT;
template <>
struct MfmaT<float> {
    static constexpr int KC = 64;              // k per LDS stage
    static constexpr int KS = 4;               // k per MFMA
    using Acc = mfma_f32x4;                    // one lane's share of a 16 x 16 result
    using Part = float;                        // its element
    using Frag = float;                        // one lane's share of an operand
};
template <>
struct MfmaT<double> {
    static constexpr int KC = 32;
    static constexpr int KS = 4;
    using Acc = mfma_f64x4;
    using Part = double;
    using Frag = double;
};
template <>
struct MfmaT<bf16_t> {
    static constexpr int KC = 128;
    static constexpr int KS = 32;
    using Acc = mfma_f32x4;
    using Part = float;
    using Frag = mfma_bf16x8;
};

template <typename V>
constexpr int lds_pad() { return 16 / (int)sizeof(V); }                      // one 16-byte pad per LDS row
template <typename V>
constexpr int mfma_pitch() { return MfmaT<V>::KC + lds_pad<V>(); }            // pitch of an image of KC elements per row

template <typename I>
__device__ __forceinline__ int64_t ld_idx(const void* p, int64_t i) { return (int64_t) static_cast<const I*>(p)[i]; }

// Largest e in [0, n) with ptr[e] <= t (ptr ascending, ptr[0] = 0 <= t).
template <typename I>
__device__ __forceinline__ int64_t upper_slot(const void* ptr, int64_t n, int64_t t) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (ld_idx<I>(ptr, mid) <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// T[row][k] (pitch P) = src[base(row) + k] for row < ROWS, k < KC; zero where row >= rows_ok, k >= k_ok or base(row) < 0.
// k is contiguous in memory: 16-byte loads and 16-byte LDS writes where the address allows.
template <typename V, int ROWS, int KC, int P, typename Base>
__device__ __forceinline__ void stage_kmajor(V* T, const V* __restrict__ src, int rows_ok, int k_ok, Base base) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_ROW = KC / W;
    for (int v = threadIdx.x; v < ROWS * PER_ROW; v += kBlock) {
        const int row = v / PER_ROW, k = (v % PER_ROW) * W;
        V* dst = T + row * P + k;
        const int64_t off = row < rows_ok ? base(row) : -1;
        if (off < 0 || k >= k_ok) {
            *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
            continue;
        }
        const V* s = src + off + k;
        if (k + W <= k_ok && al16(s)) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(s);
        } else {
            V tmp[W];
#pragma unroll
            for (int j = 0; j < W; ++j) tmp[j] = k + j < k_ok ? s[j] : V{};
            __builtin_memcpy(dst, tmp, 16);
        }
    }
}

// T[row][k] (pitch P) = src[base(k) + row]: the row index is contiguous in memory (16-byte loads, scattered LDS writes).
template <typename V, int ROWS, int KC, int P, typename Base>
__device__ __forceinline__ void stage_rmajor(V* T, const V* __restrict__ src, int rows_ok, int k_ok, Base base) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_K = ROWS / W;
    for (int v = threadIdx.x; v < KC * PER_K; v += kBlock) {
        const int k = v / PER_K, row = (v % PER_K) * W;
        const int64_t off = k < k_ok ? base(k) : -1;
        V tmp[W];
        if (off < 0 || row >= rows_ok) {
#pragma unroll
            for (int j = 0; j < W; ++j) tmp[j] = V{};
        } else {
            const V* s = src + off + row;
            if (row + W <= rows_ok && al16(s)) {
                const uint4 raw = *reinterpret_cast<const uint4*>(s);
                __builtin_memcpy(tmp, &raw, 16);
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j) tmp[j] = row + j < rows_ok ? s[j] : V{};
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) T[(row + j) * P + k] = tmp[j];
    }
}

// MFMA operand of lane (r, q) from an image with k contiguous: T[row][k0 ..]
template <typename V, int P>
__device__ __forceinline__ typename MfmaT<V>::Frag frag_k(const V* T, int row, int k0, int q) {
    if constexpr (std::is_same<V, bf16_t>::value) return *reinterpret_cast<const mfma_bf16x8*>(T + row * P + k0 + 8 * q);
    else return T[row * P + k0 + q];
}
// ... and from an image stored the other way round: T[k][row]
template <typename V, int P>
__device__ __forceinline__ typename MfmaT<V>::Frag frag_t(const V* T, int row, int k0, int q) {
    if constexpr (std::is_same<V, bf16_t>::value) {
        uint16_t w[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = T[(k0 + 8 * q + j) * P + row].bits;
        mfma_bf16x8 f;
        __builtin_memcpy(&f, w, 16);
        return f;
    } else {
        return T[(k0 + q) * P + row];
    }
}

// c + a · bᵀ on one 16 x 16 tile: the MFMA of the value type.
template <typename V>
__device__ __forceinline__ typename MfmaT<V>::Acc mfma_16x16(typename MfmaT<V>::Frag a, typename MfmaT<V>::Frag b, typename MfmaT<V>::Acc c) {
    if constexpr (std::is_same<V, bf16_t>::value) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    else if constexpr (std::is_same<V, double>::value) return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[mt][nt] += X(mt, k0) · Y(nt, k0)ᵀ over k0 in [0, k_end) in ascending order, one MFMA per (mt, nt, k0), for the row tiles
// [m_lo, m_hi) and the first n_cnt column tiles (all uniform over the wave).  fx(mt, k0) and fy(nt, k0) load the lane's
// fragments (frag_k, frag_t).
template <typename V, int MT, int NT, typename FX, typename FY>
__device__ __forceinline__ void mfma_step(typename MfmaT<V>::Acc (&acc)[MT][NT], int m_lo, int m_hi, int n_cnt, int k_end, FX fx, FY fy) {
    constexpr int KS = MfmaT<V>::KS;
    for (int k0 = 0; k0 < k_end; k0 += KS) {
        typename MfmaT<V>::Frag yb[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (nt < n_cnt) yb[nt] = fy(nt, k0);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (mt < m_lo || mt >= m_hi) continue;
            const typename MfmaT<V>::Frag xa = fx(mt, k0);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if (nt < n_cnt) acc[mt][nt] = mfma_16x16<V>(xa, yb[nt], acc[mt][nt]);
        }
    }
}

// c + a · bᵀ with a 2:4 sparse `a` on one 16 x 16 tile over 32 dense k: `a` is the lane's four kept values, `idx` its position
// register, of which the instruction reads byte ABID (the header comment has the maps).  semi_impl.h is the one user.
typedef __bf16 mfma_bf16x4 __attribute__((ext_vector_type(4)));
template <int ABID>
__device__ __forceinline__ mfma_f32x4 smfmac_16x16x32(mfma_bf16x4 a, mfma_bf16x8 b, mfma_f32x4 c, int idx, std::integral_constant<int, ABID>) {
    static_assert(ABID >= 0 && ABID < 4, "one of the four position bytes");
    return __builtin_amdgcn_smfmac_f32_16x16x32_bf16(a, b, c, idx, 0, ABID);
}

// Row inside a 16 x 16 MFMA result of accumulator register `reg` on lane `lane` (its column: lane & 15).
template <typename V>
__device__ __forceinline__ int acc_row(int lane, int reg) {
    if constexpr (std::is_same<V, double>::value) return (lane >> 4) + 4 * reg;
    else return 4 * (lane >> 4) + reg;
}

template <typename V>
__device__ __forceinline__ V to_v(typename MfmaT<V>::Part x) {
    if constexpr (std::is_same<V, bf16_t>::value) return VT<bf16_t>::down(x);
    else return x;
}

}  // namespace tsgu
