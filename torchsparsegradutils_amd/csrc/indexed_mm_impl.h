// Segmented / gathered dense products on the matrix cores (gather_mm, segment_mm and their gradients).
//
// Rows are grouped into segments by a plan built on the host side with device torch ops (indexed_matmul.py):
//   offsets[n_seg + 3]:  0 = offsets[0] <= offsets[1] <= ... <= offsets[n_seg + 1] <= offsets[n_seg + 2] = n.
//     Extended segment e in [0, n_seg + 2) holds the (permuted) rows [offsets[e], offsets[e + 1]); extended segments 1 .. n_seg
//     are the real ones (b[e - 1]); 0 and n_seg + 1 hold rows whose index lies outside [0, n_seg) and are written as zeros.
//   tile_ptr[n_seg + 3]: tile_ptr[e] = sum_{e' < e} ceil(len_e' / kImmBM), the first row tile of extended segment e.
// A workgroup finds its (segment, tile) by a binary search over tile_ptr, so the grid needs no host read-back: it is launched
// with a bound (ceil(n / BM) + min(n_seg, n) + 2 >= tile_ptr[n_seg + 2]) and the workgroups beyond the last tile exit.
//
// The LDS images, their padding, the MFMA lane maps and the staging are the matrix-core tile layer's (mfma_tile.h): X = a's row
// tile (forward) or aᵀ (grad_b), Y = b[r]ᵀ (forward) or gᵀ (grad_b), both with k contiguous.  Zero padding past D1 / D2 / the
// segment end adds exact zeros.
#pragma once

#include "mfma_tile.h"

namespace tsgu {

constexpr int kImmBM = 128;                    // rows of one forward tile
constexpr int kImmGT = 64;                     // grad_b output tile: kImmGT x kImmGT of (D1, D2)

// acc[mt][nt] += X[mb + 16 mt .. +16][0 .. KC) · Y[16 nt .. +16][0 .. KC)ᵀ for one wave.
template <typename V, int MT, int NT, int P>
__device__ __forceinline__ void mfma_stage(const V* X, const V* Y, int mb, typename MfmaT<V>::Acc (&acc)[MT][NT]) {
    constexpr int KC = MfmaT<V>::KC, KS = MfmaT<V>::KS;
    const int lane = threadIdx.x & (kWave - 1);
    const int r = lane & 15, q = lane >> 4;
#pragma unroll 2
    for (int k0 = 0; k0 < KC; k0 += KS) {
        typename MfmaT<V>::Frag xa[MT], yb[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) xa[mt] = frag_k<V, P>(X, mb + 16 * mt + r, k0, q);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) yb[nt] = frag_k<V, P>(Y, 16 * nt + r, k0, q);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma_16x16<V>(xa[mt], yb[nt], acc[mt][nt]);
    }
}

template <typename V>
struct ImmFwd {
    const void* offsets;
    const void* tile_ptr;
    const void* perm;        // NULL: identity
    const V* a;
    const V* b;
    V* out;
    int64_t lda, ldo, bs0, bs1, bs2;
    int64_t n_seg, d1, d2;
};

// out[perm[i]] = a[perm[i]] @ b[r] for the rows i of one row tile of segment r, columns [n0, n0 + BN).
template <typename V, typename I, int BN>
__global__ void __launch_bounds__(kBlock) imm_fwd_kernel(ImmFwd<V> p) {
    constexpr int KC = MfmaT<V>::KC, P = mfma_pitch<V>();
    constexpr int MT = kImmBM / 16 / (kBlock / kWave), NT = BN / 16;
    __shared__ __attribute__((aligned(16))) V Xs[kImmBM * P];
    __shared__ __attribute__((aligned(16))) V Ys[BN * P];
    __shared__ int64_t src_row[kImmBM];

    const int64_t t = blockIdx.x;
    const int64_t n_ext = p.n_seg + 2;
    if (t >= ld_idx<I>(p.tile_ptr, n_ext)) return;
    const int64_t e = upper_slot<I>(p.tile_ptr, n_ext + 1, t);
    const int64_t seg_lo = ld_idx<I>(p.offsets, e), seg_hi = ld_idx<I>(p.offsets, e + 1);
    const int64_t row0 = seg_lo + (t - ld_idx<I>(p.tile_ptr, e)) * kImmBM;
    const int rows = (int)min((int64_t)kImmBM, seg_hi - row0);
    const int64_t n0 = (int64_t)blockIdx.y * BN;
    const int cols = (int)min((int64_t)BN, p.d2 - n0);
    const bool live = e >= 1 && e <= p.n_seg;                    // else: rows of an index outside [0, R) -> zeros

    for (int i = threadIdx.x; i < kImmBM; i += kBlock)
        src_row[i] = i < rows ? (p.perm ? ld_idx<I>(p.perm, row0 + i) : row0 + i) : -1;
    __syncthreads();

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int mb = wave * MT * 16;
    typename MfmaT<V>::Acc acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = typename MfmaT<V>::Acc{};

    if (live) {
        const int64_t bro = (e - 1) * p.bs0;
        for (int64_t k0 = 0; k0 < p.d1; k0 += KC) {
            const int k_ok = (int)min((int64_t)KC, p.d1 - k0);
            stage_kmajor<V, kImmBM, KC, P>(Xs, p.a + k0, rows, k_ok, [&](int i) { return src_row[i] * p.lda; });
            if (p.bs2 == 1)   // b[r][k][n] with n contiguous (forward)
                stage_rmajor<V, BN, KC, P>(Ys, p.b + bro + n0, cols, k_ok, [&](int k) { return (k0 + k) * p.bs1; });
            else              // k contiguous (a transposed view: the grad_a product)
                stage_kmajor<V, BN, KC, P>(Ys, p.b + bro + k0 * p.bs1, cols, k_ok, [&](int n) { return (n0 + n) * p.bs2; });
            __syncthreads();
            mfma_stage<V, MT, NT, P>(Xs, Ys, mb, acc);
            __syncthreads();
        }
    }

    // epilogue: 16 lanes write 16 consecutive columns of one output row
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = mb + 16 * mt + acc_row<V>(lane, reg);
            if (row >= rows) continue;
            V* o = p.out + src_row[row] * p.ldo + n0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int col = 16 * nt + (lane & 15);
                if (col < cols) o[col] = to_v<V>(acc[mt][nt][reg]);
            }
        }
}

template <typename V>
struct ImmGradB {
    const void* offsets;     // as for the forward (extended: n_seg + 3 entries)
    const void* chunk_ptr;   // [n_seg + 1]: first chunk of real segment r
    const void* part_ptr;    // [n_seg + 1]: first partial slot of segment r (segments of two or more chunks only)
    const void* perm;
    const V* a;              // (n, d1), rows through perm
    const V* g;              // (n, d2), rows through perm
    V* gb;                   // (n_seg, d1, d2) contiguous
    typename MfmaT<V>::Part* part;   // partial slots of d1 * d2 each
    int64_t lda, ldg;
    int64_t n_seg, d1, d2, chunk;
};

// One (segment, chunk, output tile): sum over the chunk's rows of a_iᵀ g_i, into grad_b directly when the segment has one
// chunk, else into its partial slot.  Rows are taken in order, KC at a time, each product an ordered fmaf chain (f32, f64).
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) imm_gradb_kernel(ImmGradB<V> p) {
    constexpr int KC = MfmaT<V>::KC, P = mfma_pitch<V>();
    constexpr int MT = kImmGT / 16 / (kBlock / kWave), NT = kImmGT / 16;
    __shared__ __attribute__((aligned(16))) V Xs[kImmGT * P];
    __shared__ __attribute__((aligned(16))) V Ys[kImmGT * P];
    __shared__ int64_t src_row[KC];

    const int64_t t = blockIdx.x;
    if (t >= ld_idx<I>(p.chunk_ptr, p.n_seg)) return;
    const int64_t r = upper_slot<I>(p.chunk_ptr, p.n_seg + 1, t);
    const int64_t c = t - ld_idx<I>(p.chunk_ptr, r);
    const int64_t nch = ld_idx<I>(p.chunk_ptr, r + 1) - ld_idx<I>(p.chunk_ptr, r);
    const int64_t seg_hi = ld_idx<I>(p.offsets, r + 2);
    const int64_t lo = ld_idx<I>(p.offsets, r + 1) + c * p.chunk;
    const int64_t hi = min(lo + p.chunk, seg_hi);
    const int64_t m0 = (int64_t)blockIdx.y * kImmGT, n0 = (int64_t)blockIdx.z * kImmGT;
    const int m_ok = (int)min((int64_t)kImmGT, p.d1 - m0), n_ok = (int)min((int64_t)kImmGT, p.d2 - n0);

    const int wave = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    const int mb = wave * MT * 16;
    typename MfmaT<V>::Acc acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = typename MfmaT<V>::Acc{};

    for (int64_t k0 = lo; k0 < hi; k0 += KC) {
        const int k_ok = (int)min((int64_t)KC, hi - k0);
        for (int i = threadIdx.x; i < KC; i += kBlock)
            src_row[i] = i < k_ok ? (p.perm ? ld_idx<I>(p.perm, k0 + i) : k0 + i) : -1;
        __syncthreads();
        stage_rmajor<V, kImmGT, KC, P>(Xs, p.a + m0, m_ok, k_ok, [&](int k) { return src_row[k] * p.lda; });
        stage_rmajor<V, kImmGT, KC, P>(Ys, p.g + n0, n_ok, k_ok, [&](int k) { return src_row[k] * p.ldg; });
        __syncthreads();
        mfma_stage<V, MT, NT, P>(Xs, Ys, mb, acc);
        __syncthreads();
    }

    const bool direct = nch == 1;
    using Part = typename MfmaT<V>::Part;
    Part* slot = direct ? nullptr : p.part + (ld_idx<I>(p.part_ptr, r) + c) * p.d1 * p.d2;
    V* dst = p.gb + r * p.d1 * p.d2;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int m = mb + 16 * mt + acc_row<V>(lane, reg);
            if (m >= m_ok) continue;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = 16 * nt + (lane & 15);
                if (n >= n_ok) continue;
                const int64_t at = (m0 + m) * p.d2 + n0 + n;
                if (direct) dst[at] = to_v<V>(acc[mt][nt][reg]);
                else slot[at] = acc[mt][nt][reg];
            }
        }
}

// grad_b[r] for segments without exactly one chunk: zeros (no rows) or the partials summed in chunk order.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) imm_gradb_reduce_kernel(ImmGradB<V> p) {
    const int64_t r = blockIdx.x;
    const int64_t nch = ld_idx<I>(p.chunk_ptr, r + 1) - ld_idx<I>(p.chunk_ptr, r);
    if (nch == 1) return;
    const int64_t per = p.d1 * p.d2;
    const int64_t at = (int64_t)blockIdx.y * kBlock + threadIdx.x;
    if (at >= per) return;
    using Part = typename MfmaT<V>::Part;
    Part s = 0;
    const Part* src = p.part + ld_idx<I>(p.part_ptr, r) * per + at;
    for (int64_t c = 0; c < nch; ++c) s += src[c * per];
    p.gb[r * per + at] = to_v<V>(s);
}

template <typename V, typename I>
int imm_fwd_launch(const ImmFwd<V>& P, int64_t max_tiles, hipStream_t s) {
    const bool wide = !std::is_same<V, double>::value && P.d2 > 64;
    const int bn = wide ? 128 : 64;
    const int64_t ny = (P.d2 + bn - 1) / bn;
    if (max_tiles > 0x7fffffffLL || ny > 65535) return TSGU_ERR_TOO_LARGE;
    const dim3 grid((unsigned)max_tiles, (unsigned)ny);
    if constexpr (std::is_same<V, double>::value) {
        hipLaunchKernelGGL((imm_fwd_kernel<V, I, 64>), grid, dim3(kBlock), 0, s, P);
    } else {
        if (wide) hipLaunchKernelGGL((imm_fwd_kernel<V, I, 128>), grid, dim3(kBlock), 0, s, P);
        else hipLaunchKernelGGL((imm_fwd_kernel<V, I, 64>), grid, dim3(kBlock), 0, s, P);
    }
    return check_launch();
}

template <typename V, typename I>
int imm_gradb_launch(const ImmGradB<V>& P, int64_t max_chunks, hipStream_t s) {
    const int64_t ny = (P.d1 + kImmGT - 1) / kImmGT, nz = (P.d2 + kImmGT - 1) / kImmGT;
    const int64_t per = P.d1 * P.d2, nx = (per + kBlock - 1) / kBlock;
    if (max_chunks > 0x7fffffffLL || ny > 65535 || nz > 65535 || P.n_seg > 0x7fffffffLL || nx > 65535) return TSGU_ERR_TOO_LARGE;
    if (max_chunks > 0) {
        hipLaunchKernelGGL((imm_gradb_kernel<V, I>), dim3((unsigned)max_chunks, (unsigned)ny, (unsigned)nz), dim3(kBlock), 0, s, P);
        if (const int rc = check_launch()) return rc;
    }
    hipLaunchKernelGGL((imm_gradb_reduce_kernel<V, I>), dim3((unsigned)P.n_seg, (unsigned)nx), dim3(kBlock), 0, s, P);
    return check_launch();
}

// One translation unit per value type (indexed_mm_f32 / _f64 / _bf16.hip) instantiates these, and with them the kernels of that type.
template <typename V>
int imm_fwd_dispatch(int itype, const ImmFwd<V>& P, int64_t max_tiles, hipStream_t s) {
    return with_index_type(itype, [&](auto i) { return imm_fwd_launch<V, decltype(i)>(P, max_tiles, s); });
}
template <typename V>
int imm_gradb_dispatch(int itype, const ImmGradB<V>& P, int64_t max_chunks, hipStream_t s) {
    return with_index_type(itype, [&](auto i) { return imm_gradb_launch<V, decltype(i)>(P, max_chunks, s); });
}
extern template int imm_fwd_dispatch<float>(int, const ImmFwd<float>&, int64_t, hipStream_t);
extern template int imm_fwd_dispatch<double>(int, const ImmFwd<double>&, int64_t, hipStream_t);
extern template int imm_fwd_dispatch<bf16_t>(int, const ImmFwd<bf16_t>&, int64_t, hipStream_t);
extern template int imm_gradb_dispatch<float>(int, const ImmGradB<float>&, int64_t, hipStream_t);
extern template int imm_gradb_dispatch<double>(int, const ImmGradB<double>&, int64_t, hipStream_t);
extern template int imm_gradb_dispatch<bf16_t>(int, const ImmGradB<bf16_t>&, int64_t, hipStream_t);

}  // namespace tsgu
