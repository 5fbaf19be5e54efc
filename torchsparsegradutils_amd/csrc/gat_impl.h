// Graph attention (GAT / GATv2) over a sparse pattern, forward and gradients, without an nnz-sized intermediate.
//
//   GAT    e[i,j,h] = lrelu(s_dst[i,h] + s_src[j,h]) + bias[i,j]                    O[i,h,:] = Σ_j softmax_j(e)·V[j,h,:]
//   GATv2  e[i,j,h] = Σ_k att[h,k]·lrelu(X_dst[i,h,k] + X_src[j,h,k]) + bias[i,j]    O[i,h,:] = Σ_j softmax_j(e)·X_src[j,h,:]
//
// The walk is attention_impl.h's: a workgroup owns RPB consecutive groups (rows; columns for the column pass), a group of CL×EP
// lanes owns one row, the CL column lanes span a tile of the H·d elements in 16-byte runs, the EP entry lanes take the entries
// e ≡ ep (mod EP) counted from the row's first entry, and an xor butterfly merges them at the row's end.  Two forwards:
//
//   GAT forward (gat_fwd_kernel): the logit is two scalars per head, so exp is the cost.  The weights go through LDS and are
//   computed ONCE per (entry, head): a slice of (idx, bias, row) is staged, its entries × heads-of-the-tile work items are spread
//   over all 256 threads (A: logits into s_w[stage][HT]), every row group reduces its own entries' logits to a slice maximum per
//   head and rescales its (m, sum, acc) once per slice (B), the work items replace the logits by w = exp(logit − m_new) (C), and
//   the row's lanes run a pure gather-FMA loop acc += w·V[idx] with w a broadcast LDS read (D).  nnz·H exps plus one per
//   (row, slice, head), against nnz·H·d/VEC in the per-lane scheme.  The LDS weight array holds the heads of one tile (at most 32,
//   16 for fp64); the staged slice shrinks with them (gat_stage).
//
//   GATv2 forward (gat_pass_kernel, kGatFwd): register-resident.  The row's lanes hold X_dst[i], att and att·slope, gather X_src[j]
//   once, score it (the coefficient selected by the sign of z, partial sums as attn_dot, DPP head reduction) and feed the same
//   registers to the online-softmax accumulator.
//
//   backward, rows   walk 1: δ[i,h] = Σ_j P·dP; walk 2: dS = P·(dP − δ), ds_dst / dX_dst, dA[i,j] = Σ_h dS; GATv2 also sums its
//                    workgroup's share of datt in registers → LDS → partials[workgroup, H·d]
//   backward, cols   column j keeps V[j] / X_src[j] and s_src[j] in registers, gathers dO[i], lse[i], δ[i], s_dst[i] / X_dst[i],
//                    recomputes P and dS: dV + ds_src, or dX_src with both of its terms from the one gather
//   fold             datt = Σ partials over the workgroups: sixteen contiguous runs in order, then the sixteen totals in order
// No global atomics; every sum in a fixed order that depends on the row's (column's) own entries only.
#pragma once

#include "attention_impl.h"

namespace tsgu {

constexpr int kGatWeightBytes = 16384;   // the LDS weight array of the GAT forward: 4096 fp32 / 2048 fp64 weights
constexpr int kGatFoldCols = 16, kGatFoldSegs = kBlock / kGatFoldCols;

enum GatKind { kGatV1 = 0, kGatV2 = 1 };
enum GatMode { kGatFwd = 0, kGatBwdRows = 1, kGatBwdCols = 2 };

// Operands by role.  "own": rows of the walked groups; "far": the rows gathered through idx.  Leading dimensions in elements;
// the scalar arrays s_* are [groups, heads] without padding.
struct GatParams {
    int64_t n_groups;
    const void* ptr;
    const void* idx;
    const void* perm;    // position of entry k in the bias / dA arrays (NULL: k itself)
    const void* bias;    // V[nnz] or NULL
    const void* s_own;   // GAT: s_dst (cols: s_src)
    const void* s_far;   // GAT: s_src (cols: s_dst)
    const void* x_own;   // GATv2: X_dst (cols: X_src); GAT cols: V
    const void* x_far;   // GAT: V; GATv2: X_src (cols: X_dst)
    const void* g_own;   // dO (row pass)
    const void* g_far;   // dO (column pass)
    int64_t ld_x_own, ld_x_far, ld_g_own, ld_g_far;
    const void* att;     // GATv2: V[heads·d]
    void* out0;          // O; dX_dst; dV / dX_src
    int64_t ld_out0;
    void* out_s;         // GAT: ds_dst / ds_src, V[groups, heads]
    void* lse;           // Acc[n, H]
    void* delta;         // Acc[n, H]
    void* dA;            // Acc[nnz] or NULL (row pass)
    void* partials;      // Acc[workgroups, heads·d] (GATv2 row pass)
    double slope;
    int heads, d, width;
    int cl, ep, dl, tiles;
    int stage, ht;       // GAT forward: staged entries per slice, heads per tile
};

// heads one tile of cl column lanes covers, and the slice the LDS weight array leaves room for
template <typename V>
inline int gat_tile_heads(const AttnGeom& g, int heads) {
    const int cap = g.cl / g.dl;
    return heads < cap ? heads : cap;
}
template <typename V>
inline int gat_stage(const AttnGeom& g, int heads) {
    const int fit = kGatWeightBytes / (int)sizeof(typename VT<V>::Acc) / gat_tile_heads<V>(g, heads);
    return fit < kAttnStage ? fit : kAttnStage;
}

// A lane's share of Σ_k c_k·z_k with c_k = att_k (z_k > 0) or att_k·slope: the runs of attn_dot.
template <typename Acc, int VEC>
__device__ __forceinline__ Acc gat_score(const Acc (&z)[VEC], const Acc (&c0)[VEC], const Acc (&c1)[VEC]) {
    Acc c[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) c[v] = z[v] > (Acc)0 ? c1[v] : c0[v];
    return attn_dot<Acc, VEC>(c, z);
}

template <typename Acc>
__device__ __forceinline__ Acc gat_lrelu(Acc z, Acc slope) {
    return z > (Acc)0 ? z : slope * z;
}

// ------------------------------------------------------------------------------------------------------------ GAT forward
template <typename V, typename I>
__global__ __launch_bounds__(kBlock) void gat_fwd_kernel(const GatParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int VEC = VT<V>::kWide;
    constexpr int kWeights = kGatWeightBytes / (int)sizeof(Acc);

    __shared__ int s_idx[kAttnStage];
    __shared__ Acc s_bias[kAttnStage];
    __shared__ unsigned char s_row[kAttnStage];     // the row of a staged entry, counted from the workgroup's first
    __shared__ Acc s_w[kWeights];                   // [stage][HT]: logits, then weights
    __shared__ Acc s_m[kBlock];                     // [RPB][HT]: the running maximum after this slice
    __shared__ int64_t s_ptr[kWave + 1];

    const int tid = threadIdx.x;
    const int CL = P.cl, EP = P.ep, DL = P.dl, GROUP = CL * EP, RPB = kBlock / GROUP, S = P.stage, HT = P.ht, H = P.heads;
    const int grp = tid / GROUP, gl = tid % GROUP, cl = gl % CL, ep = gl / CL;

    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const V* __restrict__ bias = static_cast<const V*>(P.bias);
    const V* __restrict__ s_dst = static_cast<const V*>(P.s_own);
    const V* __restrict__ s_src = static_cast<const V*>(P.s_far);
    const V* __restrict__ far = static_cast<const V*>(P.x_far);
    const uint32_t ld_far = (uint32_t)P.ld_x_far;
    const Acc slope = (Acc)P.slope;
    const Acc ninf = -attn_inf<Acc>();

    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    const int64_t row1 = row0 + RPB < P.n_groups ? row0 + RPB : P.n_groups;
    if (tid <= RPB) s_ptr[tid] = (int64_t)ptr[row0 + tid < row1 ? row0 + tid : row1];
    __syncthreads();
    const int64_t blk_begin = s_ptr[0], blk_end = s_ptr[RPB];
    const int64_t row = row0 + grp;
    const bool row_ok = row < row1;
    const int64_t start = row_ok ? s_ptr[grp] : 0;
    const int64_t end = row_ok ? s_ptr[grp + 1] : 0;
    const bool fits = blk_end - blk_begin <= S;      // the common case: one slice, (idx, bias, row) staged once for all tiles
    bool staged = false;

    auto stage = [&](int64_t cs, int64_t ce) {
        for (int64_t k = cs + tid; k < ce; k += kBlock) {
            s_idx[k - cs] = (int)stream_load(idx + k);
            Acc b = 0;
            if (bias) b = VT<V>::up(bias[perm ? (int64_t)perm[k] : k]);
            s_bias[k - cs] = b;
            int lo = 0, hi = RPB;                    // the last row that starts at or before k
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_ptr[mid] <= k) lo = mid;
                else hi = mid;
            }
            s_row[k - cs] = (unsigned char)lo;
        }
    };

    for (int tile = 0; tile < P.tiles; ++tile) {
        const int e0 = (tile * CL + cl) * VEC;
        const bool act = e0 < P.width;
        const int h0 = tile * HT;                          // first head of the tile
        const int nh = H - h0 < HT ? H - h0 : HT;          // its heads
        const int hl = act ? cl / DL : 0;                  // this lane's head within the tile
        const int h = h0 + hl;
        const bool head_lane = act && e0 % P.d == 0;
        const bool mine = act && row_ok;
        const int ql = cl % DL + DL * ep, NQ = DL * EP;    // this lane among the lanes of (row, head)

        Acc m = ninf, s = 0, acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0;

        for (int64_t cs = blk_begin; cs < blk_end; cs += S) {
            const int64_t ce = cs + S < blk_end ? cs + S : blk_end;
            const int cnt = (int)(ce - cs);
            __syncthreads();                               // the previous slice's (tile's) weights are no longer read
            if (!staged) {
                stage(cs, ce);
                staged = fits;
                __syncthreads();
            }
            // A: the logits, one work item per (entry, head of the tile)
            for (int it = tid; it < cnt * nh; it += kBlock) {
                const int e = it / nh, q = it - e * nh;
                const Acc z = VT<V>::up(s_dst[(row0 + s_row[e]) * H + h0 + q]) + VT<V>::up(s_src[(int64_t)s_idx[e] * H + h0 + q]);
                s_w[e * HT + q] = gat_lrelu(z, slope) + s_bias[e];
            }
            __syncthreads();
            // B: the row's maximum over this slice per head (a NaN does not take part: it poisons the sum), one rescale
            const int lo = (int)((start > cs ? start : cs) - cs), hi = (int)((end < ce ? end : ce) - cs);
            Acc mx = ninf;
            for (int i = lo + ql; i < hi; i += NQ) {
                const Acc t = s_w[i * HT + hl];
                mx = t > mx ? t : mx;
            }
            for (int st = 1; st < DL; st <<= 1) {
                const Acc o = shfl_xor_acc(mx, st);
                mx = o > mx ? o : mx;
            }
            for (int st = CL; st < GROUP; st <<= 1) {
                const Acc o = shfl_xor_acc(mx, st);
                mx = o > mx ? o : mx;
            }
            if (mx > m) {
                const Acc r = m == ninf ? (Acc)0 : exp(m - mx);
                s *= r;
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] *= r;
                m = mx;
            }
            if (mine && head_lane && ep == 0) s_m[grp * HT + hl] = m;
            __syncthreads();
            // C: weights in place of the logits (-inf: weight 0, also when the maximum is -inf)
            for (int it = tid; it < cnt * nh; it += kBlock) {
                const int e = it / nh, q = it - e * nh;
                const Acc t = s_w[e * HT + q];
                s_w[e * HT + q] = t == ninf ? (Acc)0 : exp(t - s_m[s_row[e] * HT + q]);
            }
            __syncthreads();
            // D: gather-FMA; the entry lanes by the position in the ROW
            if (lo < hi) {
                const int64_t k0 = cs + lo;
                for (int64_t k = k0 + (ep - (k0 - start) % EP + EP) % EP; k < cs + hi; k += EP) {
                    const int i = (int)(k - cs);
                    const Acc w = s_w[i * HT + hl];
                    if (act && w != (Acc)0) {
                        Acc vv[VEC];
                        load_vec<V, VEC>(far + row_off(s_idx[i], ld_far) + e0, vv);
                        s += w;
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fma(w, vv[v], acc[v]);
                    }
                }
            }
        }
        // the entry lanes share m: their states merge by plain sums
        for (int st = CL; st < GROUP; st <<= 1) {
            s += shfl_xor_acc(s, st);
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] += shfl_xor_acc(acc[v], st);
        }
        if (mine && ep == 0) {
            Acc o[VEC], l;
            if (end == start) {
                l = ninf;
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[v] = 0;
            } else if (!(s > (Acc)0) || !(s < attn_inf<Acc>()) || m == attn_inf<Acc>()) {
                l = __builtin_nanf("");
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[v] = l;
            } else {
                l = m + log(s);
#pragma unroll
                for (int v = 0; v < VEC; ++v) o[v] = acc[v] / s;
            }
            store_vec<V, VEC>(static_cast<V*>(P.out0) + row * P.ld_out0 + e0, o);
            if (head_lane) static_cast<Acc*>(P.lse)[row * H + h] = l;
        }
    }
}

// --------------------------------------------------------------------------- GATv2 forward; both kinds' backward passes
template <typename V, typename I, int KIND, int MODE>
__global__ __launch_bounds__(kBlock) void gat_pass_kernel(const GatParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int VEC = VT<V>::kWide;
    constexpr bool FWD = MODE == kGatFwd, ROWS = MODE == kGatBwdRows, COLS = MODE == kGatBwdCols, V2 = KIND == kGatV2;
    constexpr bool FOLD = V2 && ROWS;

    __shared__ int s_idx[kAttnStage];
    __shared__ Acc s_bias[kAttnStage];
    __shared__ Acc s_part[FOLD ? kBlock * VEC : 1];     // [RPB][CL·VEC]: the groups' shares of datt

    const int tid = threadIdx.x;
    const int CL = P.cl, EP = P.ep, GROUP = CL * EP, RPB = kBlock / GROUP, H = P.heads;
    const int grp = tid / GROUP, gl = tid % GROUP, cl = gl % CL, ep = gl / CL;

    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const V* __restrict__ bias = static_cast<const V*>(P.bias);
    const V* __restrict__ s_own = static_cast<const V*>(P.s_own);
    const V* __restrict__ s_far = static_cast<const V*>(P.s_far);
    const V* __restrict__ x_own = static_cast<const V*>(P.x_own);
    const V* __restrict__ x_far = static_cast<const V*>(P.x_far);
    const V* __restrict__ g_own = static_cast<const V*>(P.g_own);
    const V* __restrict__ g_far = static_cast<const V*>(P.g_far);
    const uint32_t ld_x_far = (uint32_t)P.ld_x_far, ld_g_far = (uint32_t)P.ld_g_far;
    const Acc slope = (Acc)P.slope;
    const Acc ninf = -attn_inf<Acc>();

    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    const int64_t row1 = row0 + RPB < P.n_groups ? row0 + RPB : P.n_groups;
    const int64_t blk_begin = (int64_t)ptr[row0], blk_end = (int64_t)ptr[row1];
    const int64_t row = row0 + grp;
    const bool row_ok = row < row1;
    const int64_t start = row_ok ? (int64_t)ptr[row] : 0;
    const int64_t end = row_ok ? (int64_t)ptr[row + 1] : 0;
    const bool fits = blk_end - blk_begin <= kAttnStage;
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

    auto ep_total = [&](Acc x) {
        for (int m = CL; m < GROUP; m <<= 1) x += shfl_xor_acc(x, m);
        return x;
    };

    for (int tile = 0; tile < P.tiles; ++tile) {
        const int e0 = (tile * CL + cl) * VEC;
        const bool act = e0 < P.width;
        const int h = act ? e0 / P.d : 0;
        const bool head_lane = act && e0 % P.d == 0;
        const bool mine = act && row_ok;

        // own registers: a0 = X_dst[i] (cols: X_src[j]; GAT cols: V[j]), a1 = dO[i] (row pass), so = the own scalar (GAT),
        // c1 = att, c0 = att·slope (GATv2)
        Acc a0[VEC], a1[VEC], c0[VEC], c1[VEC], so = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) a0[v] = a1[v] = c0[v] = c1[v] = 0;
        if (mine) {
            if constexpr (V2 || COLS) load_vec<V, VEC>(x_own + row * P.ld_x_own + e0, a0);
            if constexpr (ROWS) load_vec<V, VEC>(g_own + row * P.ld_g_own + e0, a1);
            if constexpr (!V2) so = VT<V>::up(s_own[row * H + h]);
        }
        if constexpr (V2) {
            if (act) load_vec<V, VEC>(static_cast<const V*>(P.att) + e0, c1);
#pragma unroll
            for (int v = 0; v < VEC; ++v) c0[v] = c1[v] * slope;
        }

        // x0: the gathered feature row (GAT rows: V[j]; GATv2: X_src[j], cols: X_dst[i]); x1: the gathered dO[i] (cols)
        auto gather = [&](int j, Acc(&x0)[VEC], Acc(&x1)[VEC], Acc& sf) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) x0[v] = x1[v] = 0;
            sf = 0;
            if (act) {
                if constexpr (V2 || !COLS) load_vec<V, VEC>(x_far + row_off(j, ld_x_far) + e0, x0);
                if constexpr (COLS) load_vec<V, VEC>(g_far + row_off(j, ld_g_far) + e0, x1);
                if constexpr (!V2) sf = VT<V>::up(s_far[(int64_t)j * H + h]);
            }
        };
        // the logit of the staged entry i; z: the LeakyReLU's argument(s) (GAT: z[0])
        auto logit = [&](int i, const Acc(&x0)[VEC], Acc sf, Acc(&z)[VEC]) {
            if constexpr (V2) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) z[v] = a0[v] + x0[v];
                return attn_head_sum(gat_score<Acc, VEC>(z, c0, c1), P.dl) + s_bias[i];
            } else {
                z[0] = so + sf;
                return gat_lrelu(z[0], slope) + s_bias[i];
            }
        };

        if constexpr (FWD) {
            Acc m = ninf, s = 0, acc[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = 0;
            walk([&](int i, int64_t) {
                Acc xs[VEC], unused[VEC], z[VEC], sf;
                gather(s_idx[i], xs, unused, sf);
                const Acc t = logit(i, xs, sf, z);
                if (t > m) {
                    const Acc r = exp(m - t);
                    s = s * r + (Acc)1;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = acc[v] * r + xs[v];
                    m = t;
                } else if (t != ninf) {
                    const Acc p = exp(t - m);
                    s += p;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] = fma(p, xs[v], acc[v]);
                }
            });
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
                if (end == start) {
                    l = ninf;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = 0;
                } else if (!(s > (Acc)0) || !(s < attn_inf<Acc>()) || m == attn_inf<Acc>()) {
                    l = __builtin_nanf("");
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = l;
                } else {
                    l = m + log(s);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) o[v] = acc[v] / s;
                }
                store_vec<V, VEC>(static_cast<V*>(P.out0) + row * P.ld_out0 + e0, o);
                if (head_lane) static_cast<Acc*>(P.lse)[row * H + h] = l;
            }
        } else {
            Acc lse_own = 0, delta_own = 0;
            if constexpr (ROWS) {
                if (mine) lse_own = static_cast<const Acc*>(P.lse)[row * H + h];
                Acc dsum = 0;
                walk([&](int i, int64_t) {
                    Acc x0[VEC], unused[VEC], z[VEC], sf;
                    gather(s_idx[i], x0, unused, sf);
                    const Acc t = logit(i, x0, sf, z);
                    const Acc dP = attn_head_sum(attn_dot<Acc, VEC>(a1, x0), P.dl);
                    dsum = fma(exp(t - lse_own), dP, dsum);
                });
                delta_own = ep_total(dsum);
                if (mine && ep == 0 && head_lane) static_cast<Acc*>(P.delta)[row * H + h] = delta_own;
            }
            // acc0: dX_dst / dV / dX_src; gs: ds_dst / ds_src (GAT); dacc: this row's share of datt (GATv2 row pass)
            Acc acc0[VEC], dacc[VEC], gs = 0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc0[v] = dacc[v] = 0;
            walk([&](int i, int64_t k) {
                const int j = s_idx[i];
                Acc x0[VEC], x1[VEC], z[VEC], sf;
                gather(j, x0, x1, sf);
                Acc l = lse_own, dl_ = delta_own;
                if constexpr (COLS) {
                    l = act ? static_cast<const Acc*>(P.lse)[(int64_t)j * H + h] : (Acc)0;
                    dl_ = act ? static_cast<const Acc*>(P.delta)[(int64_t)j * H + h] : (Acc)0;
                }
                const Acc t = logit(i, x0, sf, z);
                // dP = <dO[i], V[j]> (GATv2: <dO[i], X_src[j]>): the products commute, the bits are the row pass's
                Acc dP;
                if constexpr (ROWS) dP = attn_head_sum(attn_dot<Acc, VEC>(a1, x0), P.dl);
                else dP = attn_head_sum(attn_dot<Acc, VEC>(x1, a0), P.dl);
                const Acc p = exp(t - l);
                const Acc dS = act ? p * (dP - dl_) : (Acc)0;
                if constexpr (V2) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        acc0[v] = fma(dS, z[v] > (Acc)0 ? c1[v] : c0[v], acc0[v]);
                        if constexpr (COLS) acc0[v] = fma(p, x1[v], acc0[v]);
                        else dacc[v] = fma(dS, gat_lrelu(z[v], slope), dacc[v]);
                    }
                } else {
                    gs = fma(dS, z[0] > (Acc)0 ? (Acc)1 : slope, gs);
                    if constexpr (COLS) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc0[v] = fma(p, x1[v], acc0[v]);
                    }
                }
                if constexpr (ROWS) {
                    if (P.dA) {      // Σ over the heads of the tile (every lane of a head holds its dS), then over the tiles
                        Acc x = dS;
                        for (int m = P.dl; m < CL; m <<= 1) x += shfl_xor_acc(x, m);
                        if (cl == 0) {
                            Acc* dst = static_cast<Acc*>(P.dA) + (perm ? (int64_t)perm[k] : k);
                            *dst = tile ? *dst + x : x;
                        }
                    }
                }
            });
            if constexpr (V2 || COLS) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc0[v] = ep_total(acc0[v]);
                if (mine && ep == 0) store_vec<V, VEC>(static_cast<V*>(P.out0) + row * P.ld_out0 + e0, acc0);
            }
            if constexpr (!V2) {
                gs = ep_total(gs);
                if (mine && ep == 0 && head_lane) static_cast<V*>(P.out_s)[row * H + h] = VT<V>::down(gs);
            }
            if constexpr (FOLD) {
                // the groups' shares in group order: rows (and lanes) that own nothing hold zeros
#pragma unroll
                for (int v = 0; v < VEC; ++v) dacc[v] = ep_total(dacc[v]);
                __syncthreads();
                if (ep == 0) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) s_part[(grp * CL + cl) * VEC + v] = dacc[v];
                }
                __syncthreads();
                if (grp == 0 && ep == 0 && act) {
                    Acc* dst = static_cast<Acc*>(P.partials) + (int64_t)blockIdx.x * P.width + e0;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        Acc t = s_part[cl * VEC + v];
                        for (int g = 1; g < RPB; ++g) t += s_part[(g * CL + cl) * VEC + v];
                        dst[v] = t;
                    }
                }
            }
        }
    }
}

// datt[c] = Σ_w partials[w, c]: thread (segment, column) sums its contiguous run of workgroups in order, the first segment's
// thread then adds the kGatFoldSegs totals in order.  The order depends on n_partials alone.
template <typename V>
__global__ __launch_bounds__(kBlock) void gat_fold_kernel(const typename VT<V>::Acc* __restrict__ partials, int64_t n_partials, int width,
                                                          V* __restrict__ datt) {
    using Acc = typename VT<V>::Acc;
    __shared__ Acc sh[kBlock];
    const int tid = threadIdx.x, lc = tid % kGatFoldCols, seg = tid / kGatFoldCols;
    const int col = blockIdx.x * kGatFoldCols + lc;
    const int64_t chunk = (n_partials + kGatFoldSegs - 1) / kGatFoldSegs;
    const int64_t w0 = seg * chunk, w1 = w0 + chunk < n_partials ? w0 + chunk : n_partials;
    Acc a = 0;
    if (col < width)
        for (int64_t w = w0; w < w1; ++w) a += partials[w * width + col];
    sh[tid] = a;
    __syncthreads();
    if (seg == 0 && col < width) {
        Acc t = sh[lc];
        for (int g = 1; g < kGatFoldSegs; ++g) t += sh[g * kGatFoldCols + lc];
        datt[col] = VT<V>::down(t);
    }
}

}  // namespace tsgu
