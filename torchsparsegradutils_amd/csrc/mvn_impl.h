// Reductions of the sparse multivariate normal's density (distributions/sparse_multivariate_normal.py): the log-determinant from the
// factor's stored diagonal, the Mahalanobis term from the solve's / product's result, and the variance from the factor's rows.
//
// Every sum over rows is two-stage and in a fixed order: a workgroup owns one contiguous chunk of rows of one batch item (each thread
// a strided subsequence, then a tree through the wave / LDS), writes ONE partial per (item, column), and a second kernel adds the
// partials of an output in order.  No float atomics: the same operands give the same bits.  fp32 inputs accumulate in fp32, fp64 in
// fp64 (bf16 is not offered by these entries).  All stores are ordinary vector stores.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int64_t kMvnChunkMin = 1024;    // rows of one item a workgroup sums at least
constexpr int64_t kMvnMaxBlocks = 1024;   // partials per output at most (the second stage is one wave per output)
constexpr int kMvnRowLanes = 8;           // lanes that share one sparse row (27-point rows: four passes)

inline int64_t mvn_chunk(int64_t rows_per_item) {
    const int64_t c = (rows_per_item + kMvnMaxBlocks - 1) / kMvnMaxBlocks;
    return c < kMvnChunkMin ? kMvnChunkMin : c;
}
inline int64_t mvn_blocks(int64_t rows_per_item) {
    const int64_t c = mvn_chunk(rows_per_item);
    return rows_per_item > 0 ? (rows_per_item + c - 1) / c : 1;
}

__device__ __forceinline__ float mvn_log(float x) { return logf(x); }
__device__ __forceinline__ double mvn_log(double x) { return log(x); }

// Sum over the workgroup's 256 threads in a fixed order (butterfly inside each wave, then the four wave totals in order).
// The total is returned to thread 0 only.
template <typename Acc>
__device__ __forceinline__ Acc block_total(Acc x, Acc* sm) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) x += shfl_xor_acc(x, m);
    if ((threadIdx.x & (kWave - 1)) == 0) sm[threadIdx.x / kWave] = x;
    __syncthreads();
    Acc t = 0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kBlock / kWave; ++i) t += sm[i];
    }
    return t;
}

// ---- once per pattern: where every row keeps its diagonal entry ---------------------------------------------------------------
template <typename I>
__global__ void __launch_bounds__(kBlock) diag_positions_kernel(int64_t n, int64_t nnz, const I* __restrict__ crow,
                                                                 const I* __restrict__ col, const I* __restrict__ perm,
                                                                 I* __restrict__ pos) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    int64_t e0 = (int64_t)crow[r], e1 = (int64_t)crow[r + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;
    I p = (I)-1;
    for (int64_t e = e0; e < e1; ++e) {
        if ((int64_t)col[e] == r) {
            p = perm ? perm[e] : (I)e;      // (the first occurrence: duplicates are outside the contract, as for the solve)
            break;
        }
    }
    pos[r] = p;
}

// ---- stage 1 of Σ_i log(val[pos[i]]) (pos == NULL: Σ_i log(val[i])) -----------------------------------------------------------
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) diag_logsum_partial_kernel(int64_t rows_per_item, int64_t chunk, int64_t n_val,
                                                                      const I* __restrict__ pos, const V* __restrict__ val,
                                                                      typename VT<V>::Acc* __restrict__ partial) {
    using Acc = typename VT<V>::Acc;
    __shared__ Acc sm[kBlock / kWave];
    const int64_t item = blockIdx.y, nb = gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t r1 = r0 + chunk < rows_per_item ? r0 + chunk : rows_per_item;
    Acc acc = 0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kBlock) {
        const int64_t gi = item * rows_per_item + i;
        Acc v;
        if (pos) {
            const int64_t p = (int64_t)pos[gi];
            v = (p >= 0 && p < n_val) ? VT<V>::up(val[p]) : Acc(0);     // no stored diagonal: log 0 = -inf, as the dense formula
        } else {
            v = VT<V>::up(val[gi]);
        }
        acc += mvn_log(v);
    }
    const Acc t = block_total<Acc>(acc, sm);
    if (threadIdx.x == 0) partial[item * nb + blockIdx.x] = t;
}

// ---- stage 2 of every reduction here: out[o] = Σ_b partial[o·nb + b], one wave per output, fixed order ---------------------------
template <typename V>
__global__ void __launch_bounds__(kBlock) mvn_finalize_kernel(const typename VT<V>::Acc* __restrict__ partial, int64_t nb,
                                                               int64_t n_out, V* __restrict__ out) {
    using Acc = typename VT<V>::Acc;
    const int64_t o = (int64_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (o >= n_out) return;      // (whole waves leave together)
    const int lane = threadIdx.x & (kWave - 1);
    Acc acc = 0;
    for (int64_t j = lane; j < nb; j += kWave) acc += partial[o * nb + j];
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) acc += shfl_xor_acc(acc, m);
    if (lane == 0) out[o] = VT<V>::down(acc);
}

// ---- gradient of the log-determinant in the value array ------------------------------------------------------------------------
// kMvnRowLanes lanes per row.  fill: every entry of the row is written — g/val at the diagonal position, zero elsewhere (the zero
// fill and the scatter are one pass; rows own disjoint entries).  Otherwise the diagonal entry alone is updated in place, on top of
// a gradient that is already there.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) diag_logsum_bwd_kernel(int64_t n, int64_t rows_per_item, int64_t nnz,
                                                                  const I* __restrict__ crow, const I* __restrict__ perm,
                                                                  const I* __restrict__ pos, const V* __restrict__ val,
                                                                  const V* __restrict__ g, V* __restrict__ grad, int fill) {
    using Acc = typename VT<V>::Acc;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t r = gid / kMvnRowLanes;
    const int l = threadIdx.x & (kMvnRowLanes - 1);
    if (r >= n) return;
    const int64_t p = (int64_t)pos[r];
    const Acc gv = VT<V>::up(g[r / rows_per_item]);
    if (fill) {
        int64_t e0 = (int64_t)crow[r], e1 = (int64_t)crow[r + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > nnz) e1 = nnz;
        for (int64_t e = e0 + l; e < e1; e += kMvnRowLanes) {
            const int64_t dst = perm ? (int64_t)perm[e] : e;
            if (dst < 0 || dst >= nnz) continue;
            grad[dst] = dst == p ? VT<V>::down(gv / VT<V>::up(val[dst])) : VT<V>::down(Acc(0));
        }
    } else if (l == 0 && p >= 0 && p < nnz) {
        grad[p] = VT<V>::down(VT<V>::up(grad[p]) + gv / VT<V>::up(val[p]));
    }
}

// the dense-vector variant: grad[i] = g[item] / val[i]
template <typename V>
__global__ void __launch_bounds__(kBlock) vec_logsum_bwd_kernel(int64_t n, int64_t rows_per_item, const V* __restrict__ val,
                                                                 const V* __restrict__ g, V* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    grad[i] = VT<V>::down(VT<V>::up(g[i / rows_per_item]) / VT<V>::up(val[i]));
}

// ---- the Mahalanobis term: out[item, c] = Σ_i w_i^{±1} (Y[i,c] + E[i,c])² ------------------------------------------------------
template <typename V>
struct QuadArgs {
    const V* Y;
    int64_t ldy, ycs;      // element (i, c) of Y at Y[i·ldy + c·ycs]
    const V* E;            // optional second term (the implicit unit diagonal's share), own strides
    int64_t lde, ecs;
    const V* w;            // optional per-row weight
    int w_mode;            // 0 none, 1 multiply, 2 divide
    int64_t k, rows_per_item, chunk;
};

template <typename V>
__device__ __forceinline__ typename VT<V>::Acc quad_term(const QuadArgs<V>& a, int64_t gi, int64_t c) {
    typename VT<V>::Acc t = VT<V>::up(a.Y[gi * a.ldy + c * a.ycs]);
    if (a.E) t += VT<V>::up(a.E[gi * a.lde + c * a.ecs]);
    return t;
}

// Stage 1.  A workgroup owns a chunk of rows of one item and a tile of up to 256 columns; its threads form (rows per pass) x
// (columns) with the fast thread index along the operand's unit stride: columns for a row-major Y (the solve's result), rows for a
// column-major one (the transposed views the products return), so that a wave reads whole lines either way.
template <typename V>
__global__ void __launch_bounds__(kBlock) quadform_partial_kernel(QuadArgs<V> a, int row_major,
                                                                   typename VT<V>::Acc* __restrict__ partial) {
    using Acc = typename VT<V>::Acc;
    __shared__ Acc sm[kBlock];
    const int64_t item = blockIdx.y, nb = gridDim.x;
    const int64_t c0 = (int64_t)blockIdx.z * kBlock;
    const int kt = (int)(a.k - c0 < kBlock ? a.k - c0 : kBlock);
    const int rp = kBlock / kt;
    const int tid = threadIdx.x;
    const bool active = tid < rp * kt;
    const int ri = row_major ? tid / kt : tid % rp;
    const int cj = row_major ? tid % kt : tid / rp;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = r0 + a.chunk < a.rows_per_item ? r0 + a.chunk : a.rows_per_item;
    Acc acc = 0;
    if (active) {
        const int64_t c = c0 + cj;
        for (int64_t i = r0 + ri; i < r1; i += rp) {
            const int64_t gi = item * a.rows_per_item + i;
            const Acc t = quad_term<V>(a, gi, c);
            Acc q = t * t;
            if (a.w_mode == 1) q *= VT<V>::up(a.w[gi]);
            else if (a.w_mode == 2) q /= VT<V>::up(a.w[gi]);
            acc += q;
        }
    }
    sm[active ? ri * kt + cj : tid] = acc;      // (inactive threads sit behind the rp·kt active slots)
    __syncthreads();
    int s = 1;
    while (s < rp) s <<= 1;
    for (s >>= 1; s >= 1; s >>= 1) {
        if (active && ri < s && ri + s < rp) sm[ri * kt + cj] += sm[(ri + s) * kt + cj];
        __syncthreads();
    }
    if (active && ri == 0) partial[(item * a.k + c0 + cj) * nb + blockIdx.x] = sm[cj];
}

// Backward, one thread per row: grad_Y[i,c] = 2 g[item,c] w_i^{±1} (Y+E)[i,c] (also the gradient of E) and the row's share of
// grad_w summed over the columns in the same pass: t² g (multiply), −t² g / w² (divide).
template <typename V>
__global__ void __launch_bounds__(kBlock) quadform_bwd_kernel(QuadArgs<V> a, int64_t n, const V* __restrict__ g,
                                                               V* __restrict__ gY, int64_t ldg, int64_t gcs,
                                                               V* __restrict__ gw) {
    using Acc = typename VT<V>::Acc;
    const int64_t gi = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n) return;
    const int64_t item = gi / a.rows_per_item;
    Acc s = 1;
    if (a.w_mode == 1) s = VT<V>::up(a.w[gi]);
    else if (a.w_mode == 2) s = Acc(1) / VT<V>::up(a.w[gi]);
    Acc acc = 0;
    for (int64_t c = 0; c < a.k; ++c) {
        const Acc t = quad_term<V>(a, gi, c);
        const Acc gc = VT<V>::up(g[item * a.k + c]);
        gY[gi * ldg + c * gcs] = VT<V>::down(Acc(2) * gc * (s * t));
        acc += gc * (t * t);
    }
    if (gw) gw[gi] = VT<V>::down(a.w_mode == 2 ? -(acc * (s * s)) : acc);
}

// ---- the variance: out[i] = add_i + Σ_k val[k]² w[col[k]] over row i -----------------------------------------------------------
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) row_sumsq_kernel(int64_t n, int64_t nnz, int64_t n_w, const I* __restrict__ crow,
                                                            const I* __restrict__ col, const I* __restrict__ perm,
                                                            const V* __restrict__ val, const V* __restrict__ w,
                                                            const V* __restrict__ add, V* __restrict__ out) {
    using Acc = typename VT<V>::Acc;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t r = gid / kMvnRowLanes;
    const int l = threadIdx.x & (kMvnRowLanes - 1);
    Acc acc = 0;
    if (r < n) {
        int64_t e0 = (int64_t)crow[r], e1 = (int64_t)crow[r + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > nnz) e1 = nnz;
        for (int64_t e = e0 + l; e < e1; e += kMvnRowLanes) {
            const int64_t src = perm ? (int64_t)perm[e] : e;
            const Acc v = (src >= 0 && src < nnz) ? VT<V>::up(val[src]) : Acc(0);
            Acc q = v * v;
            if (w) {
                const int64_t j = (int64_t)col[e];
                q *= (j >= 0 && j < n_w) ? VT<V>::up(w[j]) : Acc(0);
            }
            acc += q;
        }
    }
    acc = group_sum<Acc, kMvnRowLanes>(acc);      // (every lane of the wave takes part: rows past the end carry zeros)
    if (r < n && l == 0) out[r] = VT<V>::down(add ? acc + VT<V>::up(add[r]) : acc);
}

// grad_val[k] = 2 g[row(k)] val[k] w[col[k]], the same walk (rows own disjoint entries)
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) row_sumsq_bwd_kernel(int64_t n, int64_t nnz, int64_t n_w, const I* __restrict__ crow,
                                                                const I* __restrict__ col, const I* __restrict__ perm,
                                                                const V* __restrict__ val, const V* __restrict__ w,
                                                                const V* __restrict__ g, V* __restrict__ grad) {
    using Acc = typename VT<V>::Acc;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t r = gid / kMvnRowLanes;
    const int l = threadIdx.x & (kMvnRowLanes - 1);
    if (r >= n) return;
    const Acc gr = Acc(2) * VT<V>::up(g[r]);
    int64_t e0 = (int64_t)crow[r], e1 = (int64_t)crow[r + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > nnz) e1 = nnz;
    for (int64_t e = e0 + l; e < e1; e += kMvnRowLanes) {
        const int64_t dst = perm ? (int64_t)perm[e] : e;
        if (dst < 0 || dst >= nnz) continue;
        Acc q = gr * VT<V>::up(val[dst]);
        if (w) {
            const int64_t j = (int64_t)col[e];
            q *= (j >= 0 && j < n_w) ? VT<V>::up(w[j]) : Acc(0);
        }
        grad[dst] = VT<V>::down(q);
    }
}

}  // namespace tsgu
