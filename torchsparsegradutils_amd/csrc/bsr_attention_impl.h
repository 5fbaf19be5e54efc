// Block-sparse attention on the matrix cores: softmax_row(scale·QKᵀ restricted to the stored blocks + bias)·V for a BSR pattern,
// flash style — the logits and probabilities live in registers and LDS only.  Entries: include/tsgu_hip_bsr_attention.h.
//
// A workgroup owns T rows of the walked side and one head: T / oh whole block rows while the block height oh fits, else one piece
// of one block row (the per_tile / pieces scheme of BsrMM, bsr_impl.h).  The block rows of a tile are walked one after the other;
// the stored blocks of one are concatenated along the other side in stored order, S elements per LDS stage, so a wide block is
// walked in pieces and narrow ones share a stage.  Every product is C[m][n] = sum_k X[m][k]·Y[n][k] on 16 x 16 MFMA tiles: the lane
// maps, the fragment loaders and the MFMA step are the matrix-core tile layer's (mfma_tile.h); the four waves split n (the stage's
// elements for the logits, the d columns for the results).
//
//   forward      per stage: S = Q_tile·Kᵀ, + bias block, online softmax (running max m and sum l per row, kept in LDS; 256 / T
//                lanes per row), P through LDS, O = O·exp(m_old − m_new) + P·V.  Writes O / l and lse = m + log l.
//   row pass     recomputed from lse: P = exp(t − lse), dP = dO·Vᵀ, dS = P (dP − δ), dQ += dS·K; δ = <dO, O> in a prologue.  dA is
//                the sum of dS over the heads: with dA the workgroup loops over the heads itself and adds into its own block.
//   column pass  the same over the transposed block walk (tptr, tidx, perm) with the roles swapped: a workgroup owns T keys, a
//                stage holds S query rows; dV += Pᵀ·dO, dK += dSᵀ·Q.
//
// fp32 / fp64 accumulate in their own type.  bf16 runs all five products on the bf16 MFMA with fp32 accumulation: P and dS are
// ROUNDED TO bf16 before they are multiplied (unlike attention_impl.h, whose bf16 is the fp32 path rounded once) — dS once, P as
// two terms (the rounded value and its rounded remainder), because one rounding is 2^-8 at worst and a row or column of a single
// 16-wide block has no long sum to average it over; lse, δ and dA
// stay fp32 and results are rounded once when stored.  δ = <dO, O> must not inherit the rounding of P (dA has no 2^-9 to spare): for
// bf16 the forward, when asked for O_acc, also multiplies the two bf16 residuals of P (P = hi + mid + lo to fp32 precision) into a
// second accumulator, and O_acc = (both) / l is what the row pass reads.  Deterministic: no atomics, every sum in an order fixed by the element's own
// block row (block column); nothing waits for another workgroup.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

// (T, S) per value type and head width: the largest that leave every kernel's LDS images below the CU's 160 KiB.
template <typename V, int D>
struct BatG {
    static constexpr int T = 64;
    static constexpr int S = std::is_same<V, float>::value && D == 128 ? 32 : 64;
};
template <int D>
struct BatG<double, D> {
    static constexpr int T = D >= 64 ? 32 : 64;
    static constexpr int S = D == 16 ? 64 : D == 128 ? 16 : 32;
};

constexpr int kBatMaxLds = 160 * 1024;

template <typename V>
struct BsrAttn {
    using Acc = typename MfmaT<V>::Part;
    const void* ptr;         // [n_groups + 1]: the walked side (block rows; block columns in the column pass)
    const void* idx;         // [nnzb]: block column (column pass: block row) of every walked block
    const void* perm;        // column pass: position of every walked block in val; NULL: identity
    const V* val;            // the bias blocks, NULL: no bias
    const V* Q;
    const V* K;
    const V* Vv;
    const V* dO;
    const typename MfmaT<V>::Part* O;   // row pass: the forward's result before its rounding (its Oacc for bf16)
    V* out0;                 // O, dQ, dK
    V* out1;                 // dV
    Acc* Oacc;               // forward, bf16: the result unrounded, [rows, heads·d] packed; NULL: not wanted
    Acc* lse;
    Acc* delta;
    Acc* dA;                 // row pass: NULL when not wanted
    int64_t ldq, ldk, ldv, lddo, ldo, ld0, ld1;
    int64_t n_groups, bh, bw;
    int64_t oh, kb;          // owned and walked elements per block: (bh, bw), column pass (bw, bh)
    int64_t per_tile, pieces;
    int heads, heads_y;      // heads_y: heads spread over the grid (1: the workgroup loops over them)
    int i64;                 // index type
    Acc scale;
};

__device__ __forceinline__ int64_t bat_idx(const void* p, int64_t i, int i64) {
    return i64 ? static_cast<const int64_t*>(p)[i] : (int64_t) static_cast<const int32_t*>(p)[i];
}

// k extent of an image over the head width: the bf16 MFMA sums 32 elements, d = 16 is padded with zeros
template <typename V, int D>
constexpr int bat_dk() { return std::is_same<V, bf16_t>::value && D < 32 ? 32 : D; }

// Img[i][0 .. DK) (pitch P) = src[row(i)·ld + c], c < D, zero for row(i) < 0 and for the padding c >= D; 16-byte lanes throughout.
template <typename V, int ROWS, int D, int DK, int P, typename Row>
__device__ __forceinline__ void bat_stage_k(V* Img, const V* __restrict__ src, int64_t ld, Row row) {
    constexpr int W = VT<V>::kWide, PER = DK / W;
    for (int v = threadIdx.x; v < ROWS * PER; v += kBlock) {
        const int i = v / PER, c = (v % PER) * W;
        const int64_t r = row(i);
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (r >= 0 && c < D) raw = *reinterpret_cast<const uint4*>(src + r * ld + c);
        *reinterpret_cast<uint4*>(Img + i * P + c) = raw;
    }
}
// Img[c][i] (pitch P) = src[row(i)·ld + c]: the same rows stored the other way round.
template <typename V, int ROWS, int D, int P, typename Row>
__device__ __forceinline__ void bat_stage_t(V* Img, const V* __restrict__ src, int64_t ld, Row row) {
    constexpr int W = VT<V>::kWide, PER = D / W;
    for (int v = threadIdx.x; v < ROWS * PER; v += kBlock) {
        const int i = v % ROWS, c = (v / ROWS) * W;
        const int64_t r = row(i);
        V tmp[W] = {};
        if (r >= 0) {
            const uint4 raw = *reinterpret_cast<const uint4*>(src + r * ld + c);
            __builtin_memcpy(tmp, &raw, 16);
        }
#pragma unroll
        for (int j = 0; j < W; ++j) Img[(c + j) * P + i] = tmp[j];
    }
}

template <typename A>
__device__ __forceinline__ A bat_exp(A x) {
    if constexpr (std::is_same<A, double>::value) return exp(x);
    else return expf(x);
}
template <typename A>
__device__ __forceinline__ A bat_log(A x) {
    if constexpr (std::is_same<A, double>::value) return log(x);
    else return logf(x);
}
template <typename A>
__device__ __forceinline__ A bat_inf() { return (A)__builtin_inff(); }
template <typename A>
__device__ __forceinline__ A bat_nan() { return (A)__builtin_nanf(""); }

// The tile of workgroup `t`: block rows [g_lo, g_hi) of the walked side, rows_each owned rows of each from row r0 of the blocks.
template <typename V, int T>
struct BatTile {
    int64_t g_lo, g_hi, r0, row0;
    int rows_each, rows;
    __device__ __forceinline__ BatTile(const BsrAttn<V>& p, int64_t t) {
        g_lo = p.pieces > 1 ? t / p.pieces : t * p.per_tile;
        g_hi = p.pieces > 1 ? g_lo + 1 : min(p.n_groups, g_lo + p.per_tile);
        r0 = p.pieces > 1 ? (t % p.pieces) * T : 0;
        rows_each = (int)min((int64_t)T, p.oh - r0);
        rows = (int)(g_hi - g_lo) * rows_each;
        row0 = g_lo * p.oh + r0;                  // first owned dense row: the tile's rows are consecutive
    }
};

// xoff[k], far[k] of the stage that starts at element k0 of block row g's concatenated blocks (e_lo: its first block; k_all:
// their total length).  xoff: offset in val of (block, walked element) at the block's first owned row / column, -1 past the end;
// far: the dense row of the other side that the element names.
template <typename V, int S, bool COLS>
__device__ __forceinline__ void bat_stage_index(const BsrAttn<V>& p, int64_t e_lo, int64_t k0, int64_t k_all, int64_t* xoff, int64_t* far) {
    for (int k = threadIdx.x; k < S; k += kBlock) {
        int64_t xo = -1, fr = -1;
        if (k0 + k < k_all) {
            const int64_t q = (k0 + k) / p.kb, kk = (k0 + k) - q * p.kb;
            const int64_t e = e_lo + q;
            const int64_t at = COLS && p.perm ? bat_idx(p.perm, e, p.i64) : e;
            xo = at * p.bh * p.bw + (COLS ? kk * p.bw : kk);
            fr = bat_idx(p.idx, e, p.i64) * p.kb + kk;
        }
        xoff[k] = xo;
        far[k] = fr;
    }
}

template <typename V, int D>
struct BatLds {
    using Acc = typename MfmaT<V>::Part;
    static constexpr int T = BatG<V, D>::T, S = BatG<V, D>::S;
    static constexpr int DK = bat_dk<V, D>(), PD = DK + lds_pad<V>(), PS = S + lds_pad<V>(), PL = S + 1;
    static constexpr int up16(int b) { return (b + 15) / 16 * 16; }
    static constexpr int kIndex = 2 * S * 8;
    static constexpr int kOwn = up16(T * PD * (int)sizeof(V)), kFar = up16(S * PD * (int)sizeof(V));
    static constexpr int kVt = up16(D * PS * (int)sizeof(V)), kP = up16(T * PS * (int)sizeof(V));
    static constexpr int kLogit = up16(T * PL * (int)sizeof(Acc));
    static constexpr int kSplit = std::is_same<V, bf16_t>::value ? 2 * kP : 0;      // the two residuals of P (forward, O_acc)
    static constexpr int kFwd = kIndex + up16(3 * T * (int)sizeof(Acc)) + kLogit + kOwn + kFar + kVt + kP + kSplit;
    static constexpr int kRows = kIndex + up16(2 * T * (int)sizeof(Acc)) + 2 * kOwn + 2 * kFar + kP;
    static constexpr int kCols = kIndex + up16(2 * S * (int)sizeof(Acc)) + 2 * kOwn + 2 * kFar + 2 * kP + kSplit / 2;
    static_assert(kFwd <= kBatMaxLds && kRows <= kBatMaxLds && kCols <= kBatMaxLds, "the LDS images must fit one CU");
    static_assert(S % MfmaT<V>::KS == 0 && DK % MfmaT<V>::KS == 0 && S % 16 == 0 && kBlock % T == 0, "whole MFMA steps");
};

template <typename V, int D>
__global__ void __launch_bounds__(kBlock) bat_fwd_kernel(BsrAttn<V> p) {
    using L = BatLds<V, D>;
    using Acc = typename MfmaT<V>::Part;
    using AccV = typename MfmaT<V>::Acc;
    constexpr int T = L::T, S = L::S, MT = T / 16, DK = L::DK, PD = L::PD, PS = L::PS, PL = L::PL;
    constexpr int NT_S = (S / 16 + 3) / 4, NT_O = (D / 16 + 3) / 4, TPR = kBlock / T;
    extern __shared__ __attribute__((aligned(16))) unsigned char bat_smem[];
    unsigned char* sm = bat_smem;
    int64_t* xoff = reinterpret_cast<int64_t*>(sm);
    int64_t* far = xoff + S;
    sm += L::kIndex;
    Acc* row_m = reinterpret_cast<Acc*>(sm);
    Acc* row_l = row_m + T;
    Acc* row_a = row_l + T;
    sm += L::up16(3 * T * (int)sizeof(Acc));
    Acc* Ss = reinterpret_cast<Acc*>(sm);
    sm += L::kLogit;
    V* Qs = reinterpret_cast<V*>(sm);
    sm += L::kOwn;
    V* Ks = reinterpret_cast<V*>(sm);
    sm += L::kFar;
    V* Vt = reinterpret_cast<V*>(sm);
    sm += L::kVt;
    V* Ps = reinterpret_cast<V*>(sm);
    sm += L::kP;
    // bf16: P·V takes P as two bf16 terms (Ps + Pm: a row of one narrow block has no sum to average one rounding over); with O_acc a
    // third (Pl: P to fp32 precision) goes into a second accumulator that holds what the two left out
    constexpr bool kCanSplit = std::is_same<V, bf16_t>::value;
    const bool split = kCanSplit && p.Oacc;
    V* Pm = reinterpret_cast<V*>(sm);
    V* Pl = Pm + (kCanSplit ? T * PS : 0);

    const int64_t t = blockIdx.x / p.heads_y;
    const int h = (int)(blockIdx.x % p.heads_y);
    const BatTile<V, T> tile(p, t);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const int nbs = wave * NT_S * 16, nbo = wave * NT_O * 16;
    const int ns_cnt = max(0, min(NT_S, (S - nbs) / 16)), no_cnt = max(0, min(NT_O, (D - nbo) / 16));
    const int64_t hc = (int64_t)h * D;

    bat_stage_k<V, T, D, DK, PD>(Qs, p.Q + hc, p.ldq, [&](int i) { return i < tile.rows ? tile.row0 + i : (int64_t)-1; });
    for (int i = threadIdx.x; i < T; i += kBlock) {
        row_m[i] = -bat_inf<Acc>();
        row_l[i] = 0;
    }
    AccV acc[MT][NT_O], rest[MT][NT_O];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT_O; ++nt) acc[mt][nt] = rest[mt][nt] = AccV{};

    for (int64_t g = tile.g_lo; g < tile.g_hi; ++g) {
        const int a_lo = (int)(g - tile.g_lo) * tile.rows_each, a_hi = a_lo + tile.rows_each;
        const int m_lo = a_lo / 16, m_hi = a_hi / 16;
        const int64_t e_lo = bat_idx(p.ptr, g, p.i64);
        const int64_t k_all = (bat_idx(p.ptr, g + 1, p.i64) - e_lo) * p.kb;
        for (int64_t k0 = 0; k0 < k_all; k0 += S) {
            bat_stage_index<V, S, false>(p, e_lo, k0, k_all, xoff, far);
            __syncthreads();
            bat_stage_k<V, S, D, DK, PD>(Ks, p.K + hc, p.ldk, [&](int i) { return far[i]; });
            bat_stage_t<V, S, D, PS>(Vt, p.Vv + hc, p.ldv, [&](int i) { return far[i]; });
            __syncthreads();
            {   // the logits of this wave's keys
                AccV s[MT][NT_S];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT_S; ++nt) s[mt][nt] = AccV{};
                mfma_step<V, MT, NT_S>(s, m_lo, m_hi, ns_cnt, DK, [&](int mt, int k) { return frag_k<V, PD>(Qs, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_k<V, PD>(Ks, nbs + 16 * nt + r, k, q); });
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (mt < m_lo || mt >= m_hi) continue;
#pragma unroll
                    for (int nt = 0; nt < NT_S; ++nt) {
                        if (nt >= ns_cnt) continue;
                        const int key = nbs + 16 * nt + r;
                        const int64_t xo = xoff[key];
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int row = 16 * mt + acc_row<V>(lane, reg);
                            Acc tt = -bat_inf<Acc>();
                            if (xo >= 0) {
                                tt = p.scale * s[mt][nt][reg];
                                if (p.val) tt += VT<V>::up(p.val[xo + (tile.r0 + row - a_lo) * p.bw]);
                            }
                            Ss[row * PL + key] = tt;
                        }
                    }
                }
            }
            __syncthreads();
            {   // online softmax: TPR lanes per row, each a strided share of the stage
                const int row = a_lo + threadIdx.x / TPR, sub = threadIdx.x % TPR;
                const bool live = row < a_hi;
                const int rr = live ? row : a_lo;
                Acc mx = -bat_inf<Acc>();
                for (int k = sub; k < S; k += TPR) mx = fmax(mx, Ss[rr * PL + k]);
#pragma unroll
                for (int w = 1; w < TPR; w <<= 1) mx = fmax(mx, shfl_xor_acc(mx, w));
                const Acc m_old = row_m[rr];
                const Acc m_new = fmax(m_old, mx);
                const Acc m_safe = m_new == -bat_inf<Acc>() ? (Acc)0 : m_new;
                Acc sum = 0;
                for (int k = sub; k < S; k += TPR) {
                    const Acc pv = bat_exp<Acc>(Ss[rr * PL + k] - m_safe);
                    sum += pv;
                    if (live) {
                        const V hi = to_v<V>(pv);
                        Ps[rr * PS + k] = hi;
                        if constexpr (kCanSplit) {
                            const Acc r1 = pv - VT<V>::up(hi);
                            const V mid = to_v<V>(r1);
                            Pm[rr * PS + k] = mid;
                            if (split) Pl[rr * PS + k] = to_v<V>(r1 - VT<V>::up(mid));
                        }
                    }
                }
#pragma unroll
                for (int w = 1; w < TPR; w <<= 1) sum += shfl_xor_acc(sum, w);
                if (live && sub == 0) {
                    const Acc alpha = bat_exp<Acc>(m_old - m_safe);
                    row_m[rr] = m_new;
                    row_l[rr] = row_l[rr] * alpha + sum;
                    row_a[rr] = alpha;
                }
            }
            __syncthreads();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (mt < m_lo || mt >= m_hi) continue;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const Acc alpha = row_a[16 * mt + acc_row<V>(lane, reg)];
#pragma unroll
                    for (int nt = 0; nt < NT_O; ++nt) {
                        acc[mt][nt][reg] *= alpha;
                        if constexpr (kCanSplit) rest[mt][nt][reg] *= alpha;
                    }
                }
            }
            mfma_step<V, MT, NT_O>(acc, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Ps, 16 * mt + r, k, q); },
                                   [&](int nt, int k) { return frag_k<V, PS>(Vt, nbo + 16 * nt + r, k, q); });
            if constexpr (kCanSplit) {
                mfma_step<V, MT, NT_O>(acc, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Pm, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_k<V, PS>(Vt, nbo + 16 * nt + r, k, q); });
                if (split)
                    mfma_step<V, MT, NT_O>(rest, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Pl, 16 * mt + r, k, q); },
                                           [&](int nt, int k) { return frag_k<V, PS>(Vt, nbo + 16 * nt + r, k, q); });
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // epilogue: 16 lanes write 16 consecutive columns of one row
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * mt + acc_row<V>(lane, reg);
            if (row >= tile.rows) continue;
            const int64_t g = tile.g_lo + row / tile.rows_each;
            const bool has = bat_idx(p.ptr, g + 1, p.i64) > bat_idx(p.ptr, g, p.i64);
            const Acc l = row_l[row], m = row_m[row];
            const bool none = has && l == 0;              // nothing but -inf
            const Acc lse = !has ? -bat_inf<Acc>() : none ? bat_nan<Acc>() : m + bat_log<Acc>(l);
            if (wave == 0 && r == 0) p.lse[(tile.row0 + row) * p.heads + h] = lse;
            V* o = p.out0 + (tile.row0 + row) * p.ld0 + hc;
#pragma unroll
            for (int nt = 0; nt < NT_O; ++nt) {
                if (nt >= no_cnt) continue;
                const Acc x = !has ? (Acc)0 : none ? bat_nan<Acc>() : acc[mt][nt][reg] / l;
                o[nbo + 16 * nt + r] = to_v<V>(x);
                if (p.Oacc) {
                    Acc xa = x;
                    if constexpr (kCanSplit)
                        if (has && !none) xa = (acc[mt][nt][reg] + rest[mt][nt][reg]) / l;
                    p.Oacc[(tile.row0 + row) * p.heads * D + hc + nbo + 16 * nt + r] = xa;
                }
            }
        }
}

// Row pass: dQ (and dA) of the tile's rows; δ in the prologue, written out for the column pass.
template <typename V, int D>
__global__ void __launch_bounds__(kBlock) bat_rows_kernel(BsrAttn<V> p) {
    using L = BatLds<V, D>;
    using Acc = typename MfmaT<V>::Part;
    using AccV = typename MfmaT<V>::Acc;
    constexpr int T = L::T, S = L::S, MT = T / 16, DK = L::DK, PD = L::PD, PS = L::PS;
    constexpr int NT_S = (S / 16 + 3) / 4, NT_O = (D / 16 + 3) / 4, TPR = kBlock / T;
    extern __shared__ __attribute__((aligned(16))) unsigned char bat_smem[];
    unsigned char* sm = bat_smem;
    int64_t* xoff = reinterpret_cast<int64_t*>(sm);
    int64_t* far = xoff + S;
    sm += L::kIndex;
    Acc* row_lse = reinterpret_cast<Acc*>(sm);
    Acc* row_d = row_lse + T;
    sm += L::up16(2 * T * (int)sizeof(Acc));
    V* Qs = reinterpret_cast<V*>(sm);
    sm += L::kOwn;
    V* Gs = reinterpret_cast<V*>(sm);
    sm += L::kOwn;
    V* Ks = reinterpret_cast<V*>(sm);
    sm += L::kFar;
    V* Vs = reinterpret_cast<V*>(sm);
    sm += L::kFar;
    V* Ps = reinterpret_cast<V*>(sm);

    const int64_t t = blockIdx.x / p.heads_y;
    const int h_lo = p.heads_y > 1 ? (int)(blockIdx.x % p.heads_y) : 0;
    const int h_hi = p.heads_y > 1 ? h_lo + 1 : p.heads;
    const BatTile<V, T> tile(p, t);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const int nbs = wave * NT_S * 16, nbo = wave * NT_O * 16;
    const int ns_cnt = max(0, min(NT_S, (S - nbs) / 16)), no_cnt = max(0, min(NT_O, (D - nbo) / 16));
    auto own_row = [&](int i) { return i < tile.rows ? tile.row0 + i : (int64_t)-1; };

    for (int h = h_lo; h < h_hi; ++h) {
        const int64_t hc = (int64_t)h * D;
        __syncthreads();                       // the previous head's images are no longer read
        bat_stage_k<V, T, D, DK, PD>(Qs, p.Q + hc, p.ldq, own_row);
        bat_stage_k<V, T, D, DK, PD>(Gs, p.dO + hc, p.lddo, own_row);
        {   // δ = <dO, O> of every row: TPR lanes per row
            const int row = threadIdx.x / TPR, sub = threadIdx.x % TPR;
            const bool live = row < tile.rows;
            Acc s = 0;
            if (live) {
                const V* g = p.dO + (tile.row0 + row) * p.lddo + hc;
                const Acc* o = p.O + (tile.row0 + row) * p.ldo + hc;
                for (int c = sub; c < D; c += TPR) s += VT<V>::up(g[c]) * o[c];
            }
#pragma unroll
            for (int w = 1; w < TPR; w <<= 1) s += shfl_xor_acc(s, w);
            if (live && sub == 0) {
                row_d[row] = s;
                row_lse[row] = p.lse[(tile.row0 + row) * p.heads + h];
                p.delta[(tile.row0 + row) * p.heads + h] = s;
            }
        }
        AccV acc[MT][NT_O];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT_O; ++nt) acc[mt][nt] = AccV{};

        for (int64_t g = tile.g_lo; g < tile.g_hi; ++g) {
            const int a_lo = (int)(g - tile.g_lo) * tile.rows_each, a_hi = a_lo + tile.rows_each;
            const int m_lo = a_lo / 16, m_hi = a_hi / 16;
            const int64_t e_lo = bat_idx(p.ptr, g, p.i64);
            const int64_t k_all = (bat_idx(p.ptr, g + 1, p.i64) - e_lo) * p.kb;
            for (int64_t k0 = 0; k0 < k_all; k0 += S) {
                bat_stage_index<V, S, false>(p, e_lo, k0, k_all, xoff, far);
                __syncthreads();
                bat_stage_k<V, S, D, DK, PD>(Ks, p.K + hc, p.ldk, [&](int i) { return far[i]; });
                bat_stage_k<V, S, D, DK, PD>(Vs, p.Vv + hc, p.ldv, [&](int i) { return far[i]; });
                __syncthreads();
                {
                    AccV s[MT][NT_S], dp[MT][NT_S];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT_S; ++nt) s[mt][nt] = dp[mt][nt] = AccV{};
                    mfma_step<V, MT, NT_S>(s, m_lo, m_hi, ns_cnt, DK, [&](int mt, int k) { return frag_k<V, PD>(Qs, 16 * mt + r, k, q); },
                                           [&](int nt, int k) { return frag_k<V, PD>(Ks, nbs + 16 * nt + r, k, q); });
                    mfma_step<V, MT, NT_S>(dp, m_lo, m_hi, ns_cnt, DK, [&](int mt, int k) { return frag_k<V, PD>(Gs, 16 * mt + r, k, q); },
                                           [&](int nt, int k) { return frag_k<V, PD>(Vs, nbs + 16 * nt + r, k, q); });
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        if (mt < m_lo || mt >= m_hi) continue;
#pragma unroll
                        for (int nt = 0; nt < NT_S; ++nt) {
                            if (nt >= ns_cnt) continue;
                            const int key = nbs + 16 * nt + r;
                            const int64_t xo = xoff[key];
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) {
                                const int row = 16 * mt + acc_row<V>(lane, reg);
                                Acc ds = 0;
                                if (xo >= 0) {
                                    const int64_t at = xo + (tile.r0 + row - a_lo) * p.bw;
                                    Acc tt = p.scale * s[mt][nt][reg];
                                    if (p.val) tt += VT<V>::up(p.val[at]);
                                    const Acc pv = bat_exp<Acc>(tt - row_lse[row]);
                                    ds = pv * (dp[mt][nt][reg] - row_d[row]);
                                    if (p.dA) p.dA[at] = h == h_lo ? ds : p.dA[at] + ds;
                                }
                                Ps[row * PS + key] = to_v<V>(ds);
                            }
                        }
                    }
                }
                __syncthreads();
                mfma_step<V, MT, NT_O>(acc, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Ps, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_t<V, PD>(Ks, nbo + 16 * nt + r, k, q); });
                __syncthreads();
            }
        }

#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = 16 * mt + acc_row<V>(lane, reg);
                if (row >= tile.rows) continue;
                V* o = p.out0 + (tile.row0 + row) * p.ld0 + hc;
#pragma unroll
                for (int nt = 0; nt < NT_O; ++nt)
                    if (nt < no_cnt) o[nbo + 16 * nt + r] = to_v<V>(p.scale * acc[mt][nt][reg]);
            }
    }
}

// Column pass: dK and dV of the tile's keys over the transposed block walk.
template <typename V, int D>
__global__ void __launch_bounds__(kBlock) bat_cols_kernel(BsrAttn<V> p) {
    using L = BatLds<V, D>;
    using Acc = typename MfmaT<V>::Part;
    using AccV = typename MfmaT<V>::Acc;
    constexpr int T = L::T, S = L::S, MT = T / 16, DK = L::DK, PD = L::PD, PS = L::PS;
    constexpr int NT_S = (S / 16 + 3) / 4, NT_O = (D / 16 + 3) / 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char bat_smem[];
    unsigned char* sm = bat_smem;
    int64_t* xoff = reinterpret_cast<int64_t*>(sm);
    int64_t* far = xoff + S;
    sm += L::kIndex;
    Acc* far_lse = reinterpret_cast<Acc*>(sm);
    Acc* far_d = far_lse + S;
    sm += L::up16(2 * S * (int)sizeof(Acc));
    V* Ks = reinterpret_cast<V*>(sm);
    sm += L::kOwn;
    V* Vs = reinterpret_cast<V*>(sm);
    sm += L::kOwn;
    V* Qf = reinterpret_cast<V*>(sm);
    sm += L::kFar;
    V* Gf = reinterpret_cast<V*>(sm);
    sm += L::kFar;
    V* Pt = reinterpret_cast<V*>(sm);
    sm += L::kP;
    V* St = reinterpret_cast<V*>(sm);
    sm += L::kP;
    // bf16: a column with few rows has no sum to average the rounding of P over, and one rounding (2^-8 relative at worst) is more
    // than dV's 2^-9 share: Pᵀ·dO takes P as two bf16 terms (hi + mid)
    constexpr bool kCanSplit = std::is_same<V, bf16_t>::value;
    V* Pm = reinterpret_cast<V*>(sm);

    const int64_t t = blockIdx.x / p.heads_y;
    const int h = (int)(blockIdx.x % p.heads_y);
    const BatTile<V, T> tile(p, t);
    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const int nbs = wave * NT_S * 16, nbo = wave * NT_O * 16;
    const int ns_cnt = max(0, min(NT_S, (S - nbs) / 16)), no_cnt = max(0, min(NT_O, (D - nbo) / 16));
    const int64_t hc = (int64_t)h * D;
    auto own_row = [&](int i) { return i < tile.rows ? tile.row0 + i : (int64_t)-1; };

    bat_stage_k<V, T, D, DK, PD>(Ks, p.K + hc, p.ldk, own_row);
    bat_stage_k<V, T, D, DK, PD>(Vs, p.Vv + hc, p.ldv, own_row);
    AccV dk[MT][NT_O], dv[MT][NT_O];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT_O; ++nt) dk[mt][nt] = dv[mt][nt] = AccV{};

    for (int64_t g = tile.g_lo; g < tile.g_hi; ++g) {
        const int a_lo = (int)(g - tile.g_lo) * tile.rows_each, a_hi = a_lo + tile.rows_each;
        const int m_lo = a_lo / 16, m_hi = a_hi / 16;
        const int64_t e_lo = bat_idx(p.ptr, g, p.i64);
        const int64_t k_all = (bat_idx(p.ptr, g + 1, p.i64) - e_lo) * p.kb;
        for (int64_t k0 = 0; k0 < k_all; k0 += S) {
            bat_stage_index<V, S, true>(p, e_lo, k0, k_all, xoff, far);
            __syncthreads();
            bat_stage_k<V, S, D, DK, PD>(Qf, p.Q + hc, p.ldq, [&](int i) { return far[i]; });
            bat_stage_k<V, S, D, DK, PD>(Gf, p.dO + hc, p.lddo, [&](int i) { return far[i]; });
            for (int i = threadIdx.x; i < S; i += kBlock) {
                const int64_t row = far[i];
                far_lse[i] = row >= 0 ? p.lse[row * p.heads + h] : (Acc)0;
                far_d[i] = row >= 0 ? p.delta[row * p.heads + h] : (Acc)0;
            }
            __syncthreads();
            {
                AccV s[MT][NT_S], dp[MT][NT_S];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT_S; ++nt) s[mt][nt] = dp[mt][nt] = AccV{};
                mfma_step<V, MT, NT_S>(s, m_lo, m_hi, ns_cnt, DK, [&](int mt, int k) { return frag_k<V, PD>(Ks, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_k<V, PD>(Qf, nbs + 16 * nt + r, k, q); });
                mfma_step<V, MT, NT_S>(dp, m_lo, m_hi, ns_cnt, DK, [&](int mt, int k) { return frag_k<V, PD>(Vs, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_k<V, PD>(Gf, nbs + 16 * nt + r, k, q); });
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (mt < m_lo || mt >= m_hi) continue;
#pragma unroll
                    for (int nt = 0; nt < NT_S; ++nt) {
                        if (nt >= ns_cnt) continue;
                        const int i = nbs + 16 * nt + r;          // the stage's query row
                        const int64_t xo = xoff[i];
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const int key = 16 * mt + acc_row<V>(lane, reg);
                            Acc pv = 0, ds = 0;
                            if (xo >= 0) {
                                Acc tt = p.scale * s[mt][nt][reg];
                                if (p.val) tt += VT<V>::up(p.val[xo + tile.r0 + key - a_lo]);
                                pv = bat_exp<Acc>(tt - far_lse[i]);
                                ds = pv * (dp[mt][nt][reg] - far_d[i]);
                            }
                            const V hi = to_v<V>(pv);
                            Pt[key * PS + i] = hi;
                            if constexpr (kCanSplit) Pm[key * PS + i] = to_v<V>(pv - VT<V>::up(hi));
                            St[key * PS + i] = to_v<V>(ds);
                        }
                    }
                }
            }
            __syncthreads();
            mfma_step<V, MT, NT_O>(dv, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Pt, 16 * mt + r, k, q); },
                                   [&](int nt, int k) { return frag_t<V, PD>(Gf, nbo + 16 * nt + r, k, q); });
            if constexpr (kCanSplit)
                mfma_step<V, MT, NT_O>(dv, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(Pm, 16 * mt + r, k, q); },
                                       [&](int nt, int k) { return frag_t<V, PD>(Gf, nbo + 16 * nt + r, k, q); });
            mfma_step<V, MT, NT_O>(dk, m_lo, m_hi, no_cnt, S, [&](int mt, int k) { return frag_k<V, PS>(St, 16 * mt + r, k, q); },
                                   [&](int nt, int k) { return frag_t<V, PD>(Qf, nbo + 16 * nt + r, k, q); });
            __syncthreads();
        }
    }

#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * mt + acc_row<V>(lane, reg);
            if (row >= tile.rows) continue;
            V* ok = p.out0 + (tile.row0 + row) * p.ld0 + hc;
            V* ov = p.out1 + (tile.row0 + row) * p.ld1 + hc;
#pragma unroll
            for (int nt = 0; nt < NT_O; ++nt) {
                if (nt >= no_cnt) continue;
                ok[nbo + 16 * nt + r] = to_v<V>(p.scale * dk[mt][nt][reg]);
                ov[nbo + 16 * nt + r] = to_v<V>(dv[mt][nt][reg]);
            }
        }
}

enum { kBatFwd = 0, kBatRows = 1, kBatCols = 2 };

template <typename V, int D>
int bat_launch(int mode, const BsrAttn<V>& P, int64_t grid, hipStream_t s) {
    using L = BatLds<V, D>;
    const int dev = current_device();
    if (mode == kBatFwd) return launch_large_lds<bat_fwd_kernel<V, D>>(dev, grid, kBlock, L::kFwd, kBatMaxLds, s, P);
    if (mode == kBatRows) return launch_large_lds<bat_rows_kernel<V, D>>(dev, grid, kBlock, L::kRows, kBatMaxLds, s, P);
    return launch_large_lds<bat_cols_kernel<V, D>>(dev, grid, kBlock, L::kCols, kBatMaxLds, s, P);
}

// One translation unit per value type (bsr_attention_f32 / _f64 / _bf16.hip) instantiates this, and with it the kernels of that type.
template <typename V>
int bat_dispatch(int mode, int d, const BsrAttn<V>& P, int64_t grid, hipStream_t s) {
    switch (d) {
        case 16: return bat_launch<V, 16>(mode, P, grid, s);
        case 32: return bat_launch<V, 32>(mode, P, grid, s);
        case 64: return bat_launch<V, 64>(mode, P, grid, s);
        case 128: return bat_launch<V, 128>(mode, P, grid, s);
    }
    return TSGU_ERR_BAD_ARG;
}
template <typename V>
constexpr void bat_geometry(int d, int* tile_rows, int* stage_keys) {
    *tile_rows = d == 16 ? BatG<V, 16>::T : d == 32 ? BatG<V, 32>::T : d == 64 ? BatG<V, 64>::T : BatG<V, 128>::T;
    *stage_keys = d == 16 ? BatG<V, 16>::S : d == 32 ? BatG<V, 32>::S : d == 64 ? BatG<V, 64>::S : BatG<V, 128>::S;
}
extern template int bat_dispatch<float>(int, int, const BsrAttn<float>&, int64_t, hipStream_t);
extern template int bat_dispatch<double>(int, int, const BsrAttn<double>&, int64_t, hipStream_t);
extern template int bat_dispatch<bf16_t>(int, int, const BsrAttn<bf16_t>&, int64_t, hipStream_t);

}  // namespace tsgu
