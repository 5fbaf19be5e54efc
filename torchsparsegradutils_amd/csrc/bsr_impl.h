// Block-sparse (BSR) × dense products on the matrix cores: sparse_bsr_mm's forward, its transposed product and the block SDDMM.
//
// The LDS images, their padding (one 16-byte pad per row), the MFMA lane maps and the k-major / row-major staging are the
// matrix-core tile layer's (mfma_tile.h).  Every product is C[m][n] = sum_k X[m][k] * Y[n][k]:
//   forward     X = the stored blocks' rows (k along bw, contiguous in memory), Y = the slab of B the block column names (n contiguous)
//   transposed  X = V[perm]ᵀ (m along bw, contiguous in memory; k along bh),   Y = the slab of G the block row names
//   SDDMM       X = rows of G, Y = rows of B, both with k = the dense column contiguous; one block (or one 64 x 64 piece of it)
// Forward and transposed product are one kernel (TRANS): a workgroup owns kBsrTM output rows — kBsrTM / oh whole output block rows
// while the output block height oh fits, else one piece of one block row — and BN columns.  The block rows of a tile are walked one
// after the other; the blocks of one are concatenated along k, KC elements per LDS stage, in stored order, so a block wider than a
// stage is walked in pieces and several narrow ones share a stage.  The four waves split the tile's columns, and every wave
// multiplies only the 16-row MFMA tiles the current block row touches.  Zero padding inside the tiles adds exact zeros.
// A workgroup's work follows from its grid index alone; nothing waits for another workgroup.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

constexpr int kBsrTM = 64;                     // output rows of one workgroup (both products) and the SDDMM's piece of a block
constexpr int kBsrMT = kBsrTM / 16;

template <typename V>
constexpr int bsr_tile_cols(int64_t p) { return !std::is_same<V, double>::value && p > 64 ? 128 : 64; }

// acc[mt][nt] += X[16 mt .. +16][0 .. k_end) · Y[nb + 16 nt .. +16][0 .. k_end)ᵀ for the row tiles mt in [m_lo, m_hi) (uniform).
template <typename V, int NT, int P>
__device__ __forceinline__ void bsr_mfma(const V* X, const V* Y, int nb, int m_lo, int m_hi, int k_end,
                                         typename MfmaT<V>::Acc (&acc)[kBsrMT][NT]) {
    constexpr int KS = MfmaT<V>::KS;
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    for (int k0 = 0; k0 < k_end; k0 += KS) {
        typename MfmaT<V>::Frag yb[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) yb[nt] = frag_k<V, P>(Y, nb + 16 * nt + r, k0, q);
#pragma unroll
        for (int mt = 0; mt < kBsrMT; ++mt) {
            if (mt < m_lo || mt >= m_hi) continue;
            const typename MfmaT<V>::Frag xa = frag_k<V, P>(X, 16 * mt + r, k0, q);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_16x16<V>(xa, yb[nt], acc[mt][nt]);
        }
    }
}

template <typename V>
struct BsrMM {
    const void* ptr;         // [n_groups + 1]: the walked side (block rows; block columns for TRANS)
    const void* idx;         // [nnzb]: block column (TRANS: block row) of every walked block
    const void* perm;        // TRANS: position of every walked block in val; NULL: identity
    const V* val;
    const V* D;              // the dense operand (B; TRANS: G)
    V* out;
    int64_t ldd, ldo;
    int64_t n_groups, p;
    int64_t bh, bw;          // the stored blocks
    int64_t oh, kb;          // output rows and summed elements per block: (bh, bw), TRANS (bw, bh)
    int64_t per_tile;        // output block rows per workgroup (oh <= kBsrTM), else 1
    int64_t pieces;          // workgroups per output block row (oh > kBsrTM), else 1
    int lanes;               // 1: val, D, ldd, bw and p allow whole aligned 16-byte lanes everywhere (bsr_stage_lanes)
};

// X[row][k] for the rows [16 m_lo, 16 m_hi) of the tile, of which [a_lo, a_hi) are rows r0 + (row - a_lo) of the current blocks;
// k contiguous in memory.  xoff[k]: offset of (block, k) at block row 0, < 0 past the end.  `vec`: bw is a multiple of a 16-byte lane.
template <typename V, int KC, int P>
__device__ __forceinline__ void bsr_stage_x_kmajor(V* T, const V* __restrict__ val, const int64_t* xoff, int m_lo, int m_hi, int a_lo,
                                                   int a_hi, int64_t r0, int64_t bw, bool vec) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_ROW = KC / W;
    const int first = 16 * m_lo, n = 16 * (m_hi - m_lo) * PER_ROW;
    for (int v = threadIdx.x; v < n; v += kBlock) {
        const int row = first + v / PER_ROW, k = (v % PER_ROW) * W;
        V* dst = T + row * P + k;
        V tmp[W] = {};
        if (row >= a_lo && row < a_hi) {
            const int64_t ro = (r0 + (row - a_lo)) * bw;
            if (vec) {               // a lane never straddles two blocks, and a stage ends on a lane boundary
                if (xoff[k] >= 0) {
                    const V* s = val + xoff[k] + ro;
                    if (al16(s)) {
                        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(s);
                        continue;
                    }
#pragma unroll
                    for (int j = 0; j < W; ++j) tmp[j] = s[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (xoff[k + j] >= 0) tmp[j] = val[xoff[k + j] + ro];
            }
        }
        __builtin_memcpy(dst, tmp, 16);
    }
}

// The same image with the ROW index contiguous in memory (the transposed product: X = V[perm]ᵀ).
template <typename V, int KC, int P>
__device__ __forceinline__ void bsr_stage_x_rmajor(V* T, const V* __restrict__ val, const int64_t* xoff, int m_lo, int m_hi, int a_lo,
                                                   int a_hi, int64_t r0) {
    constexpr int W = VT<V>::kWide;
    const int first = 16 * m_lo, per_k = 16 * (m_hi - m_lo) / W;
    for (int v = threadIdx.x; v < KC * per_k; v += kBlock) {
        const int k = v / per_k, row = first + (v % per_k) * W;
        V tmp[W] = {};
        if (xoff[k] >= 0) {
            const V* s = val + xoff[k] + r0 + (row - a_lo);
            if (row >= a_lo && row + W <= a_hi && al16(s)) {
                const uint4 raw = *reinterpret_cast<const uint4*>(s);
                __builtin_memcpy(tmp, &raw, 16);
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (row + j >= a_lo && row + j < a_hi) tmp[j] = s[j];
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) T[(row + j) * P + k] = tmp[j];
    }
}

// Both images of one stage for operands that aligned 16-byte lanes serve whole (BsrMM::lanes): every load of the stage is issued
// before the first LDS write, so a thread waits for memory once per stage and not once per lane.  Same images as the element-wise
// staging above.
template <typename V, int KC, int P, int BN, bool TRANS>
__device__ __forceinline__ void bsr_stage_lanes(V* Xs, V* Ys, const BsrMM<V>& p, const int64_t* xoff, const int64_t* drow, int m_lo,
                                                int m_hi, int a_lo, int a_hi, int64_t r0, int64_t n0, int cols) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_ROW = KC / W;
    constexpr int XI = kBsrTM * PER_ROW / kBlock, YI = BN * PER_ROW / kBlock;
    // Y is written transposed, element by element: LR neighbouring lanes take one 16-byte lane each of LR·16 contiguous bytes of a
    // dense row and the next lanes the next k, so that a wave's writes of one element fall on distinct LDS banks (pitch: 68 words)
    constexpr int LR = sizeof(V) == 2 ? 2 : 4;
    static_assert(XI * kBlock == kBsrTM * PER_ROW && YI * kBlock == BN * PER_ROW && (BN / W) % LR == 0, "a stage is a whole number of passes");
    const int first = 16 * m_lo, per_k = 16 * (m_hi - m_lo) / W, nx = per_k * KC;
    uint4 xr[XI], yr[YI];
#pragma unroll
    for (int it = 0; it < XI; ++it) {
        const int v = threadIdx.x + it * kBlock;
        xr[it] = make_uint4(0, 0, 0, 0);
        if (v >= nx) continue;
        if constexpr (TRANS) {      // (transposed writes: the lane map of Y below)
            const int k = (v / LR) % KC, row = first + (v / (LR * KC) * LR + v % LR) * W;
            if (xoff[k] >= 0 && row >= a_lo && row < a_hi) xr[it] = *reinterpret_cast<const uint4*>(p.val + xoff[k] + r0 + (row - a_lo));
        } else {
            const int row = first + v / PER_ROW, k = (v % PER_ROW) * W;
            if (xoff[k] >= 0 && row >= a_lo && row < a_hi)
                xr[it] = *reinterpret_cast<const uint4*>(p.val + xoff[k] + (r0 + (row - a_lo)) * p.bw);
        }
    }
#pragma unroll
    for (int it = 0; it < YI; ++it) {
        const int v = threadIdx.x + it * kBlock;
        const int k = (v / LR) % KC, row = (v / (LR * KC) * LR + v % LR) * W;
        yr[it] = make_uint4(0, 0, 0, 0);
        if (drow[k] >= 0 && row < cols) yr[it] = *reinterpret_cast<const uint4*>(p.D + n0 + drow[k] * p.ldd + row);
    }
#pragma unroll
    for (int it = 0; it < XI; ++it) {
        const int v = threadIdx.x + it * kBlock;
        if (v >= nx) continue;
        if constexpr (TRANS) {
            const int k = (v / LR) % KC, row = first + (v / (LR * KC) * LR + v % LR) * W;
            V tmp[W];
            __builtin_memcpy(tmp, &xr[it], 16);
#pragma unroll
            for (int j = 0; j < W; ++j) Xs[(row + j) * P + k] = tmp[j];
        } else {
            const int row = first + v / PER_ROW, k = (v % PER_ROW) * W;
            *reinterpret_cast<uint4*>(Xs + row * P + k) = xr[it];
        }
    }
#pragma unroll
    for (int it = 0; it < YI; ++it) {
        const int v = threadIdx.x + it * kBlock;
        const int k = (v / LR) % KC, row = (v / (LR * KC) * LR + v % LR) * W;
        V tmp[W];
        __builtin_memcpy(tmp, &yr[it], 16);
#pragma unroll
        for (int j = 0; j < W; ++j) Ys[(row + j) * P + k] = tmp[j];
    }
}

// The SDDMM's two k-major images (rows of G, rows of B) the same way (BsrSddmm::lanes).
template <typename V, int KC, int P>
__device__ __forceinline__ void bsr_stage_rows_lanes(V* Xs, V* Ys, const V* __restrict__ g, const V* __restrict__ b, int64_t ldg,
                                                     int64_t ldb, int m_ok, int n_ok, int k_ok) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_ROW = KC / W, IT = kBsrTM * PER_ROW / kBlock;
    uint4 xr[IT], yr[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int v = threadIdx.x + it * kBlock;
        const int row = v / PER_ROW, k = (v % PER_ROW) * W;
        xr[it] = yr[it] = make_uint4(0, 0, 0, 0);
        if (k < k_ok && row < m_ok) xr[it] = *reinterpret_cast<const uint4*>(g + row * ldg + k);
        if (k < k_ok && row < n_ok) yr[it] = *reinterpret_cast<const uint4*>(b + row * ldb + k);
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int v = threadIdx.x + it * kBlock;
        const int row = v / PER_ROW, k = (v % PER_ROW) * W;
        *reinterpret_cast<uint4*>(Xs + row * P + k) = xr[it];
        *reinterpret_cast<uint4*>(Ys + row * P + k) = yr[it];
    }
}

template <typename V, typename I, int BN, bool TRANS>
__global__ void __launch_bounds__(kBlock) bsr_mm_kernel(BsrMM<V> p) {
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>();
    constexpr int NT = BN / 16 / (kBlock / kWave);
    __shared__ __attribute__((aligned(16))) V Xs[kBsrTM * P];
    __shared__ __attribute__((aligned(16))) V Ys[BN * P];
    __shared__ int64_t xoff[KC];          // offset in val of (block, k) at the block's first output row, -1 past the end
    __shared__ int64_t drow[KC];          // row of the dense operand that k multiplies, -1 past the end

    const int64_t t = blockIdx.x;
    const int64_t g_lo = p.pieces > 1 ? t / p.pieces : t * p.per_tile;
    const int64_t g_hi = p.pieces > 1 ? g_lo + 1 : min(p.n_groups, g_lo + p.per_tile);
    const int64_t r0 = p.pieces > 1 ? (t % p.pieces) * kBsrTM : 0;           // first row of the blocks this tile covers
    const int rows_each = (int)min((int64_t)kBsrTM, p.oh - r0);             // rows of one block row in this tile
    const int64_t n0 = (int64_t)blockIdx.y * BN;
    const int cols = (int)min((int64_t)BN, p.p - n0);
    const bool vec = p.bw % VT<V>::kWide == 0;

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int nb = wave * NT * 16;
    typename MfmaT<V>::Acc acc[kBsrMT][NT];
#pragma unroll
    for (int mt = 0; mt < kBsrMT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = typename MfmaT<V>::Acc{};

    for (int64_t g = g_lo; g < g_hi; ++g) {
        const int a_lo = (int)(g - g_lo) * rows_each, a_hi = a_lo + rows_each;
        const int m_lo = a_lo / 16, m_hi = (a_hi + 15) / 16;
        const int64_t e_lo = ld_idx<I>(p.ptr, g);
        const int64_t k_all = (ld_idx<I>(p.ptr, g + 1) - e_lo) * p.kb;
        for (int64_t k0 = 0; k0 < k_all; k0 += KC) {
            const int k_ok = (int)min((int64_t)KC, k_all - k0);
            for (int k = threadIdx.x; k < KC; k += kBlock) {
                int64_t xo = -1, dr = -1;
                if (k < k_ok) {
                    int64_t e, kk;
                    if (k_all <= 0xffffffffLL) {          // (uniform) one 32-bit division
                        const uint32_t q = (uint32_t)(k0 + k) / (uint32_t)p.kb;
                        e = e_lo + q, kk = (k0 + k) - (int64_t)q * p.kb;
                    } else {
                        e = e_lo + (k0 + k) / p.kb, kk = (k0 + k) % p.kb;
                    }
                    const int64_t at = p.perm ? ld_idx<I>(p.perm, e) : e;
                    xo = at * p.bh * p.bw + (TRANS ? kk * p.bw : kk);
                    dr = ld_idx<I>(p.idx, e) * p.kb + kk;
                }
                xoff[k] = xo;
                drow[k] = dr;
            }
            __syncthreads();
            if (p.lanes) {
                bsr_stage_lanes<V, KC, P, BN, TRANS>(Xs, Ys, p, xoff, drow, m_lo, m_hi, a_lo, a_hi, r0, n0, cols);
            } else {
                if constexpr (TRANS) bsr_stage_x_rmajor<V, KC, P>(Xs, p.val, xoff, m_lo, m_hi, a_lo, a_hi, r0);
                else bsr_stage_x_kmajor<V, KC, P>(Xs, p.val, xoff, m_lo, m_hi, a_lo, a_hi, r0, p.bw, vec);
                stage_rmajor<V, BN, KC, P>(Ys, p.D + n0, cols, k_ok, [&](int k) { return drow[k] * p.ldd; });
            }
            __syncthreads();
            if (nb < cols) bsr_mfma<V, NT, P>(Xs, Ys, nb, m_lo, m_hi, (k_ok + KS - 1) / KS * KS, acc);
            __syncthreads();
        }
    }

    // epilogue: 16 lanes write 16 consecutive columns of one output row
    const int rows = (int)(g_hi - g_lo) * rows_each;
    V* out = p.out + (g_lo * p.oh + r0) * p.ldo + n0;
#pragma unroll
    for (int mt = 0; mt < kBsrMT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * mt + acc_row<V>(lane, reg);
            if (row >= rows) continue;
            V* o = out + (int64_t)row * p.ldo;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = nb + 16 * nt + (lane & 15);
                if (col < cols) o[col] = to_v<V>(acc[mt][nt][reg]);
            }
        }
}

template <typename V>
struct BsrSddmm {
    const void* ptr;         // [n_block_rows + 1]
    const void* idx;         // [nnzb]
    const V* G;
    const V* B;
    V* dval;
    int64_t ldg, ldb;
    int64_t n_block_rows, p, bh, bw;
    int64_t pieces_n;        // 64-column pieces of a block (grid.y = pieces_m * pieces_n)
    int lanes;               // 1: G, B, ldg, ldb and p allow whole aligned 16-byte lanes everywhere (bsr_stage_rows_lanes)
};

// dval[e] (or one kBsrTM x kBsrTM piece of it) = G[I bh .. +bh, :] · B[J bw .. +bw, :]ᵀ; the block row I by a search over ptr.
// The blocks of a block row read the same rows of G: they are neighbours in the grid, and the rows come from L2.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) bsr_sddmm_kernel(BsrSddmm<V> p) {
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>();
    __shared__ __attribute__((aligned(16))) V Xs[kBsrTM * P];
    __shared__ __attribute__((aligned(16))) V Ys[kBsrTM * P];

    const int64_t e = blockIdx.x;
    const int64_t bi = upper_slot<I>(p.ptr, p.n_block_rows, e);
    const int64_t bj = ld_idx<I>(p.idx, e);
    const int64_t m0 = (int64_t)(blockIdx.y / p.pieces_n) * kBsrTM, n0 = (int64_t)(blockIdx.y % p.pieces_n) * kBsrTM;
    const int m_ok = (int)min((int64_t)kBsrTM, p.bh - m0), n_ok = (int)min((int64_t)kBsrTM, p.bw - n0);
    const int64_t grow = bi * p.bh + m0, brow = bj * p.bw + n0;

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int nb = wave * 16;
    typename MfmaT<V>::Acc acc[kBsrMT][1];
#pragma unroll
    for (int mt = 0; mt < kBsrMT; ++mt) acc[mt][0] = typename MfmaT<V>::Acc{};

    for (int64_t k0 = 0; k0 < p.p; k0 += KC) {
        const int k_ok = (int)min((int64_t)KC, p.p - k0);
        if (p.lanes) {
            bsr_stage_rows_lanes<V, KC, P>(Xs, Ys, p.G + grow * p.ldg + k0, p.B + brow * p.ldb + k0, p.ldg, p.ldb, m_ok, n_ok, k_ok);
        } else {
            stage_kmajor<V, kBsrTM, KC, P>(Xs, p.G + k0, m_ok, k_ok, [&](int i) { return (grow + i) * p.ldg; });
            stage_kmajor<V, kBsrTM, KC, P>(Ys, p.B + k0, n_ok, k_ok, [&](int i) { return (brow + i) * p.ldb; });
        }
        __syncthreads();
        if (nb < n_ok) bsr_mfma<V, 1, P>(Xs, Ys, nb, 0, (m_ok + 15) / 16, (k_ok + KS - 1) / KS * KS, acc);
        __syncthreads();
    }

    V* out = p.dval + e * p.bh * p.bw + m0 * p.bw + n0;
    const int col = nb + (lane & 15);
#pragma unroll
    for (int mt = 0; mt < kBsrMT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = 16 * mt + acc_row<V>(lane, reg);
            if (row < m_ok && col < n_ok) out[(int64_t)row * p.bw + col] = to_v<V>(acc[mt][0][reg]);
        }
}

template <typename V, typename I, bool TRANS>
int bsr_mm_launch(const BsrMM<V>& P, hipStream_t s) {
    const int bn = bsr_tile_cols<V>(P.p);
    const int64_t nx = P.pieces > 1 ? P.n_groups * P.pieces : (P.n_groups + P.per_tile - 1) / P.per_tile;
    const int64_t ny = (P.p + bn - 1) / bn;
    if (nx > 0x7fffffffLL || ny > 65535) return TSGU_ERR_TOO_LARGE;
    const dim3 grid((unsigned)nx, (unsigned)ny);
    if constexpr (std::is_same<V, double>::value) {
        hipLaunchKernelGGL((bsr_mm_kernel<V, I, 64, TRANS>), grid, dim3(kBlock), 0, s, P);
    } else {
        if (bn == 128) hipLaunchKernelGGL((bsr_mm_kernel<V, I, 128, TRANS>), grid, dim3(kBlock), 0, s, P);
        else hipLaunchKernelGGL((bsr_mm_kernel<V, I, 64, TRANS>), grid, dim3(kBlock), 0, s, P);
    }
    return check_launch();
}

template <typename V, typename I>
int bsr_sddmm_launch(const BsrSddmm<V>& P, int64_t nnzb, hipStream_t s) {
    const int64_t ny = ((P.bh + kBsrTM - 1) / kBsrTM) * P.pieces_n;
    if (nnzb > 0x7fffffffLL || ny > 65535) return TSGU_ERR_TOO_LARGE;
    hipLaunchKernelGGL((bsr_sddmm_kernel<V, I>), dim3((unsigned)nnzb, (unsigned)ny), dim3(kBlock), 0, s, P);
    return check_launch();
}

// One translation unit per value type (bsr_f32 / _f64 / _bf16.hip) instantiates these, and with them the kernels of that type.
template <typename V>
int bsr_mm_dispatch(int itype, bool trans, const BsrMM<V>& P, hipStream_t s) {
    return with_index_type(itype, [&](auto i) {
        return trans ? bsr_mm_launch<V, decltype(i), true>(P, s) : bsr_mm_launch<V, decltype(i), false>(P, s);
    });
}
template <typename V>
int bsr_sddmm_dispatch(int itype, const BsrSddmm<V>& P, int64_t nnzb, hipStream_t s) {
    return with_index_type(itype, [&](auto i) { return bsr_sddmm_launch<V, decltype(i)>(P, nnzb, s); });
}
extern template int bsr_mm_dispatch<float>(int, bool, const BsrMM<float>&, hipStream_t);
extern template int bsr_mm_dispatch<double>(int, bool, const BsrMM<double>&, hipStream_t);
extern template int bsr_mm_dispatch<bf16_t>(int, bool, const BsrMM<bf16_t>&, hipStream_t);
extern template int bsr_sddmm_dispatch<float>(int, const BsrSddmm<float>&, int64_t, hipStream_t);
extern template int bsr_sddmm_dispatch<double>(int, const BsrSddmm<double>&, int64_t, hipStream_t);
extern template int bsr_sddmm_dispatch<bf16_t>(int, const BsrSddmm<bf16_t>&, int64_t, hipStream_t);

}  // namespace tsgu
