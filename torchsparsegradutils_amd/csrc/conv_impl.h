// neighbor_mm: sparse convolution as an implicit GEMM on the matrix cores (sparse_conv.py).
//
//   out[i] = bias + sum_k x[nbr[i][k]] @ w[k]          nbr (n_out, K) row-major; an entry outside [0, n_in) is an absent neighbour
//
// Forward / grad_x (nmm_fwd_kernel): one workgroup owns a kNmmBM x BN tile of `out` and keeps it in accumulators over the whole
// reduction, which runs over the flattened (offset, channel) axis of Xg[128][K * d1] · w.view(K * d1, d2).  One LDS stage of KC
// elements along that axis is a run of SEGMENTS:
//   d1 <= KC  ("packed")  S = min(kNmmSegs, KC / d1) whole offsets of d1 channels each, the tail zero; an offset never straddles a stage
//   d1 >  KC  ("wide")    one offset, ceil(d1 / KC) stages of KC channels
// Per stage the 128 x S neighbour indices go to LDS as element offsets into x (-1: absent), reduced on the way to "any neighbour
// present" (__syncthreads_or): a stage without one is skipped before anything else is loaded.  The gathered rows of x and the image
// of w are staged by segment (stage_segments; w with its columns contiguous through stage_rmajor), then multiplied by the tile
// layer's mfma_step.  grad_x is the same kernel on the inverse table with w read as its transposed view (ws1 == 1).
//
// grad_w (nmm_gradw_kernel): one workgroup owns offset k, a kNmmGT x kNmmGT tile of (d1, d2) and a chunk of rows; the reduction
// runs over the rows, KC at a time, both images stored with the row as the LDS row (frag_t), the x image gathered through column k
// of nbr.  Chunk partials go to a workspace [chunks][K][d1][d2] in the accumulator type and are folded in ascending chunk order
// (nmm_fold_kernel); a single chunk writes grad_w directly.  No atomics anywhere: every sum has one fixed order.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

constexpr int kNmmBM = 128;                    // rows of one forward tile
constexpr int kNmmGT = 64;                     // grad_w output tile: kNmmGT x kNmmGT of (d1, d2)
constexpr int kNmmSegs = 8;                    // most offsets of one packed stage
constexpr int kNmmNoSeg = 255;                 // seg_of[] of a k beyond the last segment

template <typename V>
__host__ __device__ inline int nmm_segs(int64_t d1) {
    constexpr int KC = MfmaT<V>::KC;
    if (d1 > KC) return 1;
    const int s = KC / (int)d1;
    return s < kNmmSegs ? s : kNmmSegs;
}

// The (segment, channel) of every k of a stage, for segments of `segw` elements of which the first `segs_max` exist.
template <int KC>
__device__ __forceinline__ void nmm_fill_tables(uint8_t* seg_of, uint8_t* col_of, int segw, int segs_max) {
    for (int k = threadIdx.x; k < KC; k += kBlock) {
        const int s = k / segw;
        seg_of[k] = (uint8_t)(s < segs_max ? s : kNmmNoSeg);
        col_of[k] = (uint8_t)(k - s * segw);
    }
}

// T[row][k] (pitch P) for row < ROWS, k < KC, the k axis cut into segments by (seg_of, col_of):
//   T[row][k] = src[base(row, s) + c],  (s, c) = (seg_of[k], col_of[k]);  zero where row >= rows_ok, s >= segs, c >= c_ok or base < 0.
// `units`: the segment width is a multiple of the 16-byte unit, so a unit lies in one segment (16-byte loads where the address
// allows); otherwise every element finds its own segment.
template <typename V, int ROWS, int KC, int P, typename Base>
__device__ __forceinline__ void stage_segments(V* T, const V* __restrict__ src, int rows_ok, int segs, int c_ok, bool units,
                                               const uint8_t* seg_of, const uint8_t* col_of, Base base) {
    constexpr int W = VT<V>::kWide;
    constexpr int PER_ROW = KC / W;
    for (int v = threadIdx.x; v < ROWS * PER_ROW; v += kBlock) {
        const int row = v / PER_ROW, k = (v % PER_ROW) * W;
        V* dst = T + row * P + k;
        if (units) {
            const int s = seg_of[k], c = col_of[k];
            const int64_t off = row < rows_ok && s < segs && c < c_ok ? base(row, s) : -1;
            if (off < 0) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(0, 0, 0, 0);
                continue;
            }
            const V* p = src + off + c;
            if (c + W <= c_ok && al16(p)) {
                *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(p);
            } else {
                V tmp[W];
#pragma unroll
                for (int j = 0; j < W; ++j) tmp[j] = c + j < c_ok ? p[j] : V{};
                __builtin_memcpy(dst, tmp, 16);
            }
        } else {
            V tmp[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                const int s = seg_of[k + j], c = col_of[k + j];
                const int64_t off = row < rows_ok && s < segs && c < c_ok ? base(row, s) : -1;
                tmp[j] = off >= 0 ? src[off + c] : V{};
            }
            __builtin_memcpy(dst, tmp, 16);
        }
    }
}

template <typename V>
struct NmmFwd {
    const void* nbr;         // (n_out, K) row-major
    const V* x;              // (n_in, d1), row stride ldx
    const V* w;              // (K, d1, d2) through its strides; ws2 == 1 or ws1 == 1
    const V* bias;           // (d2) or NULL
    V* out;                  // (n_out, d2), row stride ldo
    int64_t ldx, ldo, ws0, ws1, ws2;
    int64_t n_in, n_out, K, d1, d2;
};

template <typename V, typename I, int BN>
__global__ void __launch_bounds__(kBlock) nmm_fwd_kernel(NmmFwd<V> p) {
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = mfma_pitch<V>(), W = VT<V>::kWide;
    constexpr int MT = kNmmBM / 16 / (kBlock / kWave), NT = BN / 16;
    __shared__ __attribute__((aligned(16))) V Xs[kNmmBM * P];
    __shared__ __attribute__((aligned(16))) V Ys[BN * P];
    __shared__ int64_t xoff[kNmmBM * kNmmSegs];          // [row][s]: element offset of the gathered row in x, -1 absent
    __shared__ uint8_t seg_of[KC], col_of[KC];

    const int64_t row0 = (int64_t)blockIdx.x * kNmmBM;
    const int rows = (int)min((int64_t)kNmmBM, p.n_out - row0);
    const int64_t n0 = (int64_t)blockIdx.y * BN;
    const int cols = (int)min((int64_t)BN, p.d2 - n0);
    const bool packed = p.d1 <= KC;
    const int S = nmm_segs<V>(p.d1);
    const int segw = packed ? (int)p.d1 : KC;
    const int nsub = packed ? 1 : (int)((p.d1 + KC - 1) / KC);
    const bool units = segw % W == 0;
    nmm_fill_tables<KC>(seg_of, col_of, segw, S);        // (read after the first barrier of the loop below)

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const int mb = wave * MT * 16;
    const int n_cnt = (cols + 15) / 16;
    typename MfmaT<V>::Acc acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = typename MfmaT<V>::Acc{};

    for (int64_t kf = 0; kf < p.K; kf += S) {
        const int segs = (int)min((int64_t)S, p.K - kf);
        int any = 0;
        for (int i = threadIdx.x; i < kNmmBM * kNmmSegs; i += kBlock) {
            const int row = i / kNmmSegs, s = i % kNmmSegs;
            int64_t j = -1;
            if (row < rows && s < segs) j = ld_idx<I>(p.nbr, (row0 + row) * p.K + kf + s);
            const bool ok = j >= 0 && j < p.n_in;
            xoff[i] = ok ? j * p.ldx : -1;
            any |= ok;
        }
        if (!__syncthreads_or(any)) continue;             // occupancy skip: no row of the tile has one of these offsets
        for (int sub = 0; sub < nsub; ++sub) {
            const int64_t c0 = (int64_t)sub * KC;
            const int c_ok = packed ? segw : (int)min((int64_t)KC, p.d1 - c0);
            stage_segments<V, kNmmBM, KC, P>(Xs, p.x + c0, rows, segs, c_ok, units, seg_of, col_of,
                                             [&](int row, int s) { return xoff[row * kNmmSegs + s]; });
            if (p.ws2 == 1)   // w[k][c][n] with n contiguous (forward): with w contiguous, one run of flat rows
                stage_rmajor<V, BN, KC, P>(Ys, p.w + n0, cols, KC, [&](int k) {
                    const int s = seg_of[k], c = col_of[k];
                    return s < segs && c < c_ok ? (kf + s) * p.ws0 + (c0 + c) * p.ws1 : (int64_t)-1;
                });
            else              // c contiguous (a transposed view: the grad_x product), by offset segment
                stage_segments<V, BN, KC, P>(Ys, p.w + c0, cols, segs, c_ok, units, seg_of, col_of,
                                             [&](int n, int s) { return (kf + s) * p.ws0 + (n0 + n) * p.ws2; });
            __syncthreads();
            const int k_end = ((packed ? segs * segw : c_ok) + KS - 1) / KS * KS;
            mfma_step<V, MT, NT>(acc, 0, MT, n_cnt, k_end,
                                 [&](int mt, int k0) { return frag_k<V, P>(Xs, mb + 16 * mt + r, k0, q); },
                                 [&](int nt, int k0) { return frag_k<V, P>(Ys, 16 * nt + r, k0, q); });
            __syncthreads();
        }
    }

    // epilogue: bias, one rounding; 16 lanes write 16 consecutive columns of one output row
    typename MfmaT<V>::Part bv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = 16 * nt + r;
        bv[nt] = p.bias && col < cols ? (typename MfmaT<V>::Part)VT<V>::up(p.bias[n0 + col]) : 0;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = mb + 16 * mt + acc_row<V>(lane, reg);
            if (row >= rows) continue;
            V* o = p.out + (row0 + row) * p.ldo + n0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = 16 * nt + r;
                if (col < cols) o[col] = to_v<V>(acc[mt][nt][reg] + bv[nt]);
            }
        }
}

template <typename V>
struct NmmGradW {
    const void* nbr;         // (n_out, K) row-major
    const V* x;              // (n_in, d1), row stride ldx
    const V* g;              // (n_out, d2), row stride ldg
    V* gw;                   // (K, d1, d2) contiguous
    typename MfmaT<V>::Part* part;   // [chunks][K][d1][d2] when chunks > 1
    int64_t ldx, ldg;
    int64_t n_in, n_out, K, d1, d2, chunk, chunks;
};

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) nmm_gradw_kernel(NmmGradW<V> p) {
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS, P = kNmmGT + lds_pad<V>();
    constexpr int MT = kNmmGT / 16 / (kBlock / kWave), NT = kNmmGT / 16;
    static_assert(MT == 1, "one 16-row strip of the tile per wave");
    __shared__ __attribute__((aligned(16))) V Xs[KC * P];    // [row of the stage][c1]
    __shared__ __attribute__((aligned(16))) V Ys[KC * P];    // [row of the stage][c2]
    __shared__ int64_t src[KC];

    const int64_t c = blockIdx.x, k = blockIdx.y;
    const int64_t tn = (p.d2 + kNmmGT - 1) / kNmmGT;
    const int64_t m0 = ((int64_t)blockIdx.z / tn) * kNmmGT, n0 = ((int64_t)blockIdx.z % tn) * kNmmGT;
    const int m_ok = (int)min((int64_t)kNmmGT, p.d1 - m0), n_ok = (int)min((int64_t)kNmmGT, p.d2 - n0);
    const int64_t lo = c * p.chunk, hi = min(lo + p.chunk, p.n_out);

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
    const int mb = wave * 16;
    const int m_hi = mb < m_ok ? 1 : 0, n_cnt = (n_ok + 15) / 16;
    typename MfmaT<V>::Acc acc[MT][NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[0][nt] = typename MfmaT<V>::Acc{};

    for (int64_t r0 = lo; r0 < hi; r0 += KC) {
        const int k_ok = (int)min((int64_t)KC, hi - r0);
        int any = 0;
        for (int i = threadIdx.x; i < KC; i += kBlock) {
            const int64_t j = i < k_ok ? ld_idx<I>(p.nbr, (r0 + i) * p.K + k) : -1;
            const bool ok = j >= 0 && j < p.n_in;
            src[i] = ok ? j : -1;
            any |= ok;
        }
        if (!__syncthreads_or(any)) continue;             // no row of the stage has this neighbour
        stage_kmajor<V, KC, kNmmGT, P>(Xs, p.x + m0, k_ok, m_ok, [&](int i) { return src[i] < 0 ? (int64_t)-1 : src[i] * p.ldx; });
        stage_kmajor<V, KC, kNmmGT, P>(Ys, p.g + n0, k_ok, n_ok, [&](int i) { return src[i] < 0 ? (int64_t)-1 : (r0 + i) * p.ldg; });
        __syncthreads();
        mfma_step<V, MT, NT>(acc, 0, m_hi, n_cnt, (k_ok + KS - 1) / KS * KS,
                             [&](int, int k0) { return frag_t<V, P>(Xs, mb + r, k0, q); },
                             [&](int nt, int k0) { return frag_t<V, P>(Ys, 16 * nt + r, k0, q); });
        __syncthreads();
    }

    const bool direct = p.chunks == 1;
    const int64_t at0 = k * p.d1 * p.d2;
    typename MfmaT<V>::Part* slot = direct ? nullptr : p.part + c * p.K * p.d1 * p.d2;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int m = mb + acc_row<V>(lane, reg);
        if (m >= m_ok) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = 16 * nt + r;
            if (n >= n_ok) continue;
            const int64_t at = at0 + (m0 + m) * p.d2 + n0 + n;
            if (direct) p.gw[at] = to_v<V>(acc[0][nt][reg]);
            else slot[at] = acc[0][nt][reg];
        }
    }
}

// grad_w = the chunk partials added in ascending chunk order.
template <typename V>
__global__ void __launch_bounds__(kBlock) nmm_fold_kernel(NmmGradW<V> p) {
    const int64_t per = p.K * p.d1 * p.d2;
    const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (at >= per) return;
    typename MfmaT<V>::Part s = 0;
    for (int64_t c = 0; c < p.chunks; ++c) s += p.part[c * per + at];
    p.gw[at] = to_v<V>(s);
}

template <typename V, typename I>
int nmm_fwd_launch(const NmmFwd<V>& P, hipStream_t s) {
    constexpr bool f64 = std::is_same<V, double>::value;
    const int bn = P.d2 <= 32 ? 32 : (P.d2 <= 64 || f64 ? 64 : 128);
    const int64_t nx = (P.n_out + kNmmBM - 1) / kNmmBM, ny = (P.d2 + bn - 1) / bn;
    if (nx > 0x7fffffffLL || ny > 65535) return TSGU_ERR_TOO_LARGE;
    const dim3 grid((unsigned)nx, (unsigned)ny);
    if (bn == 32) hipLaunchKernelGGL((nmm_fwd_kernel<V, I, 32>), grid, dim3(kBlock), 0, s, P);
    else if (bn == 64) hipLaunchKernelGGL((nmm_fwd_kernel<V, I, 64>), grid, dim3(kBlock), 0, s, P);
    else if constexpr (!f64) hipLaunchKernelGGL((nmm_fwd_kernel<V, I, 128>), grid, dim3(kBlock), 0, s, P);
    return check_launch();
}

template <typename V, typename I>
int nmm_gradw_launch(const NmmGradW<V>& P, hipStream_t s) {
    const int64_t tiles = ((P.d1 + kNmmGT - 1) / kNmmGT) * ((P.d2 + kNmmGT - 1) / kNmmGT);
    const int64_t per = P.K * P.d1 * P.d2, nf = (per + kBlock - 1) / kBlock;
    if (P.chunks > 0x7fffffffLL || P.K > 65535 || tiles > 65535 || nf > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    hipLaunchKernelGGL((nmm_gradw_kernel<V, I>), dim3((unsigned)P.chunks, (unsigned)P.K, (unsigned)tiles), dim3(kBlock), 0, s, P);
    if (const int rc = check_launch()) return rc;
    if (P.chunks == 1) return TSGU_OK;
    return launch(nmm_fold_kernel<V>, nf, s, P);
}

}  // namespace tsgu
