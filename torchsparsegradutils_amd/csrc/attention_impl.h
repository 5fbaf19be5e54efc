// Attention over a sparse pattern: O[i,h,:] = Σ_j softmax_j(scale·<Q[i,h],K[j,h]> + bias[i,j]) · V[j,h,:] over the stored j of row i,
// and its gradients, without an nnz-sized intermediate: the logits live in registers, the forward keeps one log-sum-exp per
// (row, head) and the backward recomputes the probabilities from it.
//
// All three kernels walk (ptr, idx, perm-or-NULL) the way the plan-free SpMM walks a CSR matrix (spmm_impl.h): a workgroup owns
// RPB consecutive groups (rows; columns for the column pass), stages its contiguous slice of (idx, bias) in LDS with coalesced
// loads, kAttnStage entries at a time, and a group of CL×EP lanes owns one row.  The CL column lanes span the H·d elements of a
// dense row, VEC (16 bytes) each, so a gathered K[j] / V[j] is one contiguous run of 16-byte loads; the d/VEC lanes of one head
// reduce its dot product by DPP.  The EP entry lanes take the entries e ≡ ep (mod EP) of the row (e counted from the row's first
// entry, so the assignment does not depend on where the row lies) concurrently and are merged by an xor butterfly at the row's
// end: a fixed order, no atomics.  Rows wider than 64 accumulator lanes (256 fp32 / bf16 elements, 128 fp64) are walked as tiles
// of that width, one after the other: heads are independent, so a tile is a complete problem of its own.
//
//   forward          online softmax per entry lane (running maximum, sum, accumulator); writes O and lse[n, H]
//   backward, rows   walk 1: δ[i,h] = Σ_j P·dP (= <dO[i,h], O[i,h]> of the UNROUNDED O: bf16 gradients are those of the fp32
//                    path rounded once), walk 2: dS = P·(dP − δ), dQ[i,h] = scale·Σ_j dS·K[j,h], dA[i,j] = Σ_h dS
//   backward, cols   over the transposed pattern: column j keeps K[j], V[j] in registers, gathers Q[i], dO[i], lse[i], δ[i]:
//                    dK[j,h] = scale·Σ_i dS·Q[i,h], dV[j,h] = Σ_i P·dO[i,h]
// A row or hub column longer than one slice is walked by its one lane group, slice after slice: correct, not split.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kAttnStage = 1024;     // staged (idx, bias) entries per slice
constexpr int kAttnMaxHeadDim = 128;
constexpr int kAttnMaxWidth = 1024;  // H·d

enum AttnMode { kAttnFwd = 0, kAttnBwdRows = 1, kAttnBwdCols = 2 };

// Operands by role.  "own": rows of the walked groups (Q, dO for the row direction; K, V for the column pass); "far": the rows
// gathered through idx (K, V; Q, dO for the column pass).  Leading dimensions in elements.
struct AttnParams {
    int64_t n_groups;
    const void* ptr;
    const void* idx;
    const void* perm;   // position of entry k in the bias / dA arrays (NULL: k itself)
    const void* bias;   // V[nnz] or NULL
    const void* own0;   // Q  (cols: K)
    const void* own1;   // dO (cols: V); unused by the forward
    const void* far0;   // K  (cols: Q)
    const void* far1;   // V  (cols: dO)
    int64_t ld_own0, ld_own1, ld_far0, ld_far1;
    void* out0;         // O, dQ, dK
    void* out1;         // dV
    int64_t ld_out0, ld_out1;
    void* lse;          // Acc[n, H]: written by the forward, read by the backward
    void* delta;        // Acc[n, H]: written by the row pass, read by the column pass
    void* dA;           // Acc[nnz] or NULL (row pass)
    double scale;
    int heads, d, width;        // width = heads·d
    int cl, ep, dl, tiles;      // column lanes, entry lanes, lanes per head, tiles of cl column lanes
};

struct AttnGeom {
    int cl, ep, dl, tiles;
    int rows_per_block() const { return kBlock / (cl * ep); }
};

inline bool attn_supported(int heads, int d) {
    return heads >= 1 && (d == 8 || d == 16 || d == 32 || d == 64 || d == 128) && (int64_t)heads * d <= kAttnMaxWidth;
}

// The entry lanes are a function of the row's bytes in the ACCUMULATOR type, so that bf16 (8 elements per lane, fp32 sums) walks
// every row exactly as fp32 does: its results are the fp32 results rounded once.
template <typename V>
inline AttnGeom attn_geom(int heads, int d) {
    using Acc = typename VT<V>::Acc;
    constexpr int VEC = VT<V>::kWide;
    AttnGeom g;
    // a tile is 64 accumulator lanes wide (256 fp32 / bf16 elements, 128 fp64): bf16 keeps 32 column lanes of 8 when it tiles
    constexpr int max_cl = kWave * (16 / (int)sizeof(Acc)) / VEC;
    const int lanes = heads * d / VEC;
    g.dl = d / VEC;
    g.cl = lanes >= max_cl ? max_cl : next_pow2(lanes);
    g.tiles = (lanes + g.cl - 1) / g.cl;
    const int acc_lanes = next_pow2((int64_t)heads * d * (int)sizeof(Acc) / 16);
    g.ep = acc_lanes <= 16 ? 4 : acc_lanes == 32 ? 2 : 1;
    return g;
}

// Σ over the dl lanes of one head (an all-reduce: every lane of the head gets the total).  dl is uniform over the launch.
template <typename Acc>
__device__ __forceinline__ Acc attn_head_sum(Acc x, int dl) {
    switch (dl) {
        case 2: return group_sum<Acc, 2>(x);
        case 4: return group_sum<Acc, 4>(x);
        case 8: return group_sum<Acc, 8>(x);
        case 16: return group_sum<Acc, 16>(x);
        case 32: return group_sum<Acc, 32>(x);
        case 64: return group_sum<Acc, 64>(x);
    }
    return x;
}

// A lane's share of a dot product: runs of four elements summed in order, then the runs pairwise — what two fp32 lanes and the
// first butterfly step make of the same eight elements.
template <typename Acc, int VEC>
__device__ __forceinline__ Acc attn_dot(const Acc (&x)[VEC], const Acc (&y)[VEC]) {
    if constexpr (VEC == 8) {
        Acc a = x[0] * y[0], b = x[4] * y[4];
#pragma unroll
        for (int v = 1; v < 4; ++v) {
            a = fma(x[v], y[v], a);
            b = fma(x[4 + v], y[4 + v], b);
        }
        return a + b;
    } else {
        Acc a = x[0] * y[0];
#pragma unroll
        for (int v = 1; v < VEC; ++v) a = fma(x[v], y[v], a);
        return a;
    }
}

template <typename Acc>
__device__ __forceinline__ Acc attn_inf() {
    return (Acc)__builtin_huge_valf();
}

template <typename V, typename I, int MODE>
__global__ __launch_bounds__(kBlock) void attn_kernel(const AttnParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int VEC = VT<V>::kWide;
    constexpr bool FWD = MODE == kAttnFwd, ROWS = MODE == kAttnBwdRows, COLS = MODE == kAttnBwdCols;

    __shared__ int s_idx[kAttnStage];
    __shared__ Acc s_bias[kAttnStage];

    const int tid = threadIdx.x;
    const int CL = P.cl, EP = P.ep, GROUP = CL * EP, RPB = kBlock / GROUP;
    const int grp = tid / GROUP, gl = tid % GROUP, cl = gl % CL, ep = gl / CL;

    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const V* __restrict__ bias = static_cast<const V*>(P.bias);
    const V* __restrict__ own0 = static_cast<const V*>(P.own0);
    const V* __restrict__ own1 = static_cast<const V*>(P.own1);
    const V* __restrict__ far0 = static_cast<const V*>(P.far0);
    const V* __restrict__ far1 = static_cast<const V*>(P.far1);
    const uint32_t ld_far0 = (uint32_t)P.ld_far0, ld_far1 = (uint32_t)P.ld_far1;
    const Acc scale = (Acc)P.scale;
    const Acc ninf = -attn_inf<Acc>();

    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    const int64_t row1 = row0 + RPB < P.n_groups ? row0 + RPB : P.n_groups;
    const int64_t blk_begin = (int64_t)ptr[row0], blk_end = (int64_t)ptr[row1];
    const int64_t row = row0 + grp;
    const bool row_ok = row < row1;
    const int64_t start = row_ok ? (int64_t)ptr[row] : 0;
    const int64_t end = row_ok ? (int64_t)ptr[row + 1] : 0;
    const bool fits = blk_end - blk_begin <= kAttnStage;   // the common case: one slice, staged once for all walks
    bool staged = false;

    auto stage = [&](int64_t cs, int64_t ce) {
        for (int64_t k = cs + tid; k < ce; k += kBlock) {
            s_idx[k - cs] = (int)stream_load(idx + k);
            Acc b = 0;
            if (bias) b = VT<V>::up(bias[perm ? (int64_t)perm[k] : k]);
            s_bias[k - cs] = b;
        }
    };

    // body(i, k): entry k of this lane's row, staged at i.  Entry lanes by the position in the ROW.
    auto walk = [&](auto&& body) {
        if (fits) {
            if (!staged) {
                stage(blk_begin, blk_end);
                __syncthreads();
                staged = true;
            }
            for (int64_t k = start + ep; k < end; k += EP) body((int)(k - blk_begin), k);
        } else {
            for (int64_t cs = blk_begin; cs < blk_end; cs += kAttnStage) {
                const int64_t ce = cs + kAttnStage < blk_end ? cs + kAttnStage : blk_end;
                __syncthreads();
                stage(cs, ce);
                __syncthreads();
                const int64_t lo = start > cs ? start : cs, hi = end < ce ? end : ce;
                if (lo < hi) {
                    const int64_t first = lo + (ep - (lo - start) % EP + EP) % EP;
                    for (int64_t k = first; k < hi; k += EP) body((int)(k - cs), k);
                }
            }
        }
    };

    // Σ over the entry lanes of the group (all-reduce by xor butterfly: both partners add the same two numbers)
    auto ep_total = [&](Acc x) {
        for (int m = CL; m < GROUP; m <<= 1) x += shfl_xor_acc(x, m);
        return x;
    };

    for (int tile = 0; tile < P.tiles; ++tile) {
        const int e0 = (tile * CL + cl) * VEC;      // first element of this lane
        const bool act = e0 < P.width;
        const int h = act ? e0 / P.d : 0;
        const bool head_lane = act && e0 % P.d == 0;   // the lane that stores a head's scalars
        const bool mine = act && row_ok;

        Acc a0[VEC], a1[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) a0[v] = a1[v] = 0;
        if (mine) {
            load_vec<V, VEC>(own0 + row * P.ld_own0 + e0, a0);
            if constexpr (!FWD) load_vec<V, VEC>(own1 + row * P.ld_own1 + e0, a1);
        }

        auto gather = [&](int j, Acc(&x0)[VEC], Acc(&x1)[VEC]) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) x0[v] = x1[v] = 0;
            if (act) {
                load_vec<V, VEC>(far0 + row_off(j, ld_far0) + e0, x0);
                load_vec<V, VEC>(far1 + row_off(j, ld_far1) + e0, x1);
            }
        };

        if constexpr (FWD) {
            Acc m = ninf, s = 0, acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0;
            walk([&](int i, int64_t) {
                Acc kv[VEC], vv[VEC];
                gather(s_idx[i], kv, vv);
                const Acc t = fma(scale, attn_head_sum(attn_dot<Acc, VEC>(a0, kv), P.dl), s_bias[i]);
                if (t > m) {           // a new maximum: the state is rescaled (m = -inf: by exp(-inf) = 0)
                    const Acc r = exp(m - t);
                    s = s * r + (Acc)1;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * r + vv[v];
                    m = t;
                } else if (t != ninf) {  // (-inf: weight 0; NaN: falls through here and poisons s)
                    const Acc p = exp(t - m);
                    s += p;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fma(p, vv[v], acc[v]);
                }
            });
            // merge the entry lanes: state ⊕ state is symmetric, so both partners of a butterfly step hold the same bits
            for (int st = CL; st < GROUP; st <<= 1) {
                const Acc m2 = shfl_xor_acc(m, st), s2 = shfl_xor_acc(s, st);
                const Acc M = m2 > m ? m2 : m;
                const Acc f1 = m == ninf ? (Acc)0 : exp(m - M), f2 = m2 == ninf ? (Acc)0 : exp(m2 - M);
                s = s * f1 + s2 * f2;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const Acc o = shfl_xor_acc(acc[v], st);
                    acc[v] = acc[v] * f1 + o * f2;
                }
                m = M;
            }
            if (mine && ep == 0) {
                Acc o[VEC], l;
                if (end == start) {        // no stored entry: zeros, lse = -inf
                    l = ninf;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = 0;
                } else if (!(s > (Acc)0) || !(s < attn_inf<Acc>()) || m == attn_inf<Acc>()) {
                    // a NaN or +inf logit, or nothing but -inf: NaN for this head (torch.softmax on the row's values)
                    l = __builtin_nanf("");
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = l;
                } else {
                    l = m + log(s);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = acc[v] / s;
                }
                store_vec<V, VEC>(static_cast<V*>(P.out0) + row * P.ld_out0 + e0, o);
                if (head_lane) static_cast<Acc*>(P.lse)[row * P.heads + h] = l;
            }
        } else {
            // P and dS of one entry from the recomputed logit; rows: lse and δ are the row's own, cols: gathered with Q[i], dO[i]
            Acc lse_own = 0, delta_own = 0;
            if constexpr (ROWS) {
                if (mine) lse_own = static_cast<const Acc*>(P.lse)[row * P.heads + h];
                Acc dsum = 0;
                walk([&](int i, int64_t) {
                    Acc kv[VEC], vv[VEC];
                    gather(s_idx[i], kv, vv);
                    const Acc t = fma(scale, attn_head_sum(attn_dot<Acc, VEC>(a0, kv), P.dl), s_bias[i]);
                    const Acc dP = attn_head_sum(attn_dot<Acc, VEC>(a1, vv), P.dl);
                    dsum = fma(exp(t - lse_own), dP, dsum);
                });
                delta_own = ep_total(dsum);
                if (mine && ep == 0 && head_lane) static_cast<Acc*>(P.delta)[row * P.heads + h] = delta_own;
            }
            Acc acc0[VEC], acc1[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc0[v] = acc1[v] = 0;
            walk([&](int i, int64_t k) {
                const int j = s_idx[i];
                Acc x0[VEC], x1[VEC];
                gather(j, x0, x1);
                Acc l = lse_own, dl_ = delta_own;
                if constexpr (COLS) {
                    l = act ? static_cast<const Acc*>(P.lse)[(int64_t)j * P.heads + h] : (Acc)0;
                    dl_ = act ? static_cast<const Acc*>(P.delta)[(int64_t)j * P.heads + h] : (Acc)0;
                }
                // (x·y commutes: the logit has the same bits whichever side is gathered)
                const Acc t = fma(scale, attn_head_sum(attn_dot<Acc, VEC>(COLS ? x0 : a0, COLS ? a0 : x0), P.dl), s_bias[i]);
                const Acc dP = attn_head_sum(attn_dot<Acc, VEC>(COLS ? x1 : a1, COLS ? a1 : x1), P.dl);
                const Acc p = exp(t - l);
                const Acc dS = p * (dP - dl_);
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc0[v] = fma(dS, x0[v], acc0[v]);
                if constexpr (COLS) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc1[v] = fma(p, x1[v], acc1[v]);
                } else {
                    if (P.dA) {      // Σ over the heads of the tile (every lane of a head holds its dS), then over the tiles
                        Acc x = act ? dS : (Acc)0;
                        for (int m = P.dl; m < CL; m <<= 1) x += shfl_xor_acc(x, m);
                        if (cl == 0) {
                            Acc* dst = static_cast<Acc*>(P.dA) + (perm ? (int64_t)perm[k] : k);
                            *dst = tile ? *dst + x : x;
                        }
                    }
                }
            });
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                acc0[v] = ep_total(acc0[v]) * scale;
                if constexpr (COLS) acc1[v] = ep_total(acc1[v]);
            }
            if (mine && ep == 0) {
                store_vec<V, VEC>(static_cast<V*>(P.out0) + row * P.ld_out0 + e0, acc0);
                if constexpr (COLS) store_vec<V, VEC>(static_cast<V*>(P.out1) + row * P.ld_out1 + e0, acc1);
            }
        }
    }
}

}  // namespace tsgu
