// CSR × dense in the semirings of log-domain code (sparse_semiring_mm):
//   log       C[i,c] = log Σ_e exp(val[e] + B[col[e],c])        e over the stored entries of row i
//   max_plus  C[i,c] = max_e (val[e] + B[col[e],c])             min_plus: min
// One template family in three kinds (forward, gradient of the values, gradient of B) with the semiring as a template tag: the
// tropical instantiations hold no exp.  The candidate t = val + B is ONE addition in the accumulator type and lives in a
// register from its gather to its use, in all three kinds: there is no nnz × p array anywhere.
//
// Forward: the row-group walk of spmm_impl.h (a group of CL×EP lanes owns a row, the workgroup's (col, val) slice staged in LDS in
// passes of kStageCap entries, 16-byte gathers of the dense rows, grid.z over column slices).  Lane state per column element:
//   log       (m, s) with s = Σ exp(t − m); one exp per element and entry: with d = t − m and e = exp(−|d|), a new maximum rescales
//             (s = s·e + 1, m = t) and anything else adds (s += e).  −inf candidates (absent entries), +inf and NaN go through
//             selects.  The EP partials of a row merge by the symmetric (max, sum) combine of logsumexp_impl.h.
//   tropical  (best, arg) with the winner rule and the merge of mm_reduce_impl.h.
// Gradients, with W[e,c] = exp(val[e] + B[col[e],c] − C[i,c]) (0 for a −inf candidate) or [arg[i,c] == e]:
//   dval[e] = Σ_c G[i,c]·W[e,c]    one pass over the rows; G and C (arg) of the lane's columns stay in registers
//   dB[j,c] = Σ_e G[i,c]·W[e,c]    the same walk over the transposed pattern; B[j,·] stays in registers
// No atomics, nothing waits for another workgroup, every sum in a fixed order.
#pragma once

#include "logsumexp_impl.h"
#include "mm_reduce_impl.h"

namespace tsgu {

enum { kSemiringLog = 0, kSemiringMax = 1, kSemiringMin = 2 };

struct SemiringParams {
    int64_t n_groups, p;   // rows (forward, values pass) or columns of A (dense pass)
    const void* ptr;       // crow / tptr
    const void* idx;       // col / tidx
    const void* perm;      // dense pass: position of every transposed entry in A's value array
    const void* val;
    const void* B;
    int64_t ldb;
    const void* G;
    int64_t ldg;
    void* out;             // forward: C; values pass: dval; dense pass: dB
    int64_t ldout;
    void* cacc;            // log: C in the accumulator type (forward: written when not NULL; backward: read)
    int64_t ldacc;
    int* arg;              // tropical: the winners
    int64_t ldarg;
    int64_t nblocks;
};

// ---- VEC consecutive accumulator values (VEC > 1: 16-byte aligned address) -----------------------------------------------------
template <typename Acc, int VEC>
__device__ __forceinline__ void load_acc(const Acc* __restrict__ ptr, Acc (&out)[VEC]) {
    constexpr int W = VT<Acc>::kWide;
    if constexpr (VEC == 1) {
        out[0] = *ptr;
    } else {
        static_assert(VEC % W == 0, "whole 16-byte accesses");
#pragma unroll
        for (int q = 0; q < VEC; q += W) {
            Acc part[W];
            load_vec<Acc, W>(ptr + q, part);
#pragma unroll
            for (int v = 0; v < W; ++v) out[q + v] = part[v];
        }
    }
}

template <typename Acc, int VEC>
__device__ __forceinline__ void store_acc(Acc* __restrict__ ptr, const Acc (&in)[VEC]) {
    constexpr int W = VT<Acc>::kWide;
    if constexpr (VEC == 1) {
        *ptr = in[0];
    } else {
#pragma unroll
        for (int q = 0; q < VEC; q += W) {
            Acc part[W];
#pragma unroll
            for (int v = 0; v < W; ++v) part[v] = in[q + v];
            store_vec<Acc, W, true>(ptr + q, part);
        }
    }
}

// One candidate t into (m, s): ONE exp.  d = t − m; a new maximum (d > 0, or a NaN candidate onto a number) rescales the sum, anything
// else adds exp(d).  t = −inf is an absent entry: its term is 0 also against m = −inf (where d would be NaN).  Once m is NaN it
// stays; once it is +inf the sum no longer matters (lse_finish).  Selects only.
template <typename Acc>
__device__ __forceinline__ void lse_take(Acc& m, Acc& s, Acc t) {
    const Acc d = t - m;
    const bool absent = t == -(Acc)INFINITY;
    const Acc e = absent ? Acc(0) : acc_exp(-fabs(d));
    const bool up = !(d <= Acc(0)) & (m == m) & !absent;
    const Acc grown = s * e + Acc(1);
    const Acc added = s + e;
    s = up ? grown : added;
    m = up ? t : m;
}

// A gradient term g·W with W = exp(t − C) the weight of candidate t against the row's stored C.  An absent entry (t = −inf) has no
// term: exactly 0 whatever g and C are (C = −inf in a row of nothing but absent entries).
template <typename Acc>
__device__ __forceinline__ Acc lse_term(Acc g, Acc t, Acc c) {
    const Acc x = g * acc_exp(t - c);
    return t == -(Acc)INFINITY ? Acc(0) : x;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <typename V, typename I, int VEC, int CL, int EP, int SR>
__global__ __launch_bounds__(kBlock) void csr_semiring_mm_kernel(const SemiringParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int U = 4;   // gathers issued back to back per lane
    constexpr int SU = 4;  // staging loads issued back to back per thread
    constexpr bool LOG = SR == kSemiringLog;
    constexpr bool MIN = SR == kSemiringMin;

    __shared__ __attribute__((aligned(16))) unsigned char smem[StageBytes<V>::value];
    const Staged<V> stage(smem);

    const int tid = threadIdx.x;
    const int grp = tid / GROUP;
    const int gl = tid % GROUP;
    const int cl = gl % CL;
    const int ep = gl / CL;

    const int64_t vb = xcd_chunked_block(blockIdx.x, P.nblocks);
    const int64_t cbase = ((int64_t)blockIdx.z * CL + cl) * VEC;  // first column of this lane
    const bool col_ok = cbase < P.p;

    const I* __restrict__ crow = static_cast<const I*>(P.ptr);
    const I* __restrict__ col = static_cast<const I*>(P.idx);
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* __restrict__ B = static_cast<const V*>(P.B) + cbase;
    const uint32_t ldb = (uint32_t)P.ldb;

    const int64_t row0 = vb * RPB;
    const int64_t row1 = row0 + RPB < P.n_groups ? row0 + RPB : P.n_groups;
    const int64_t blk_begin = (int64_t)crow[row0];
    const int64_t blk_end = (int64_t)crow[row1];
    const int64_t row = row0 + grp;
    const bool row_ok = row < row1;
    const int64_t start = row_ok ? (int64_t)crow[row] : 0;
    const int64_t end = row_ok ? (int64_t)crow[row + 1] : 0;

    // log: (m, s); tropical: (best, arg) — `x` is m or best
    Acc x[VEC], s[VEC];
    int arg[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) x[v] = MIN ? (Acc)INFINITY : -(Acc)INFINITY, s[v] = 0, arg[v] = -1;

    auto take = [&](int v, Acc t, int pos) {
        if constexpr (LOG) lse_take<Acc>(x[v], s[v], t);
        else reduce_take<MIN, Acc>(x[v], arg[v], t, pos);
    };

    // the workgroup's slice [blk_begin, blk_end) goes through the staging window in passes; a pass's loads are all issued before
    // its first LDS write.  Every pass visits a lane's entries in increasing position.
    for (int64_t cs = blk_begin; cs < blk_end; cs += kStageCap) {
        const int64_t ce = cs + kStageCap < blk_end ? cs + kStageCap : blk_end;
        if (cs != blk_begin) __syncthreads();
        for (int64_t base = cs + tid; base < ce; base += (int64_t)kBlock * SU) {
            I cj[SU];
            V vv[SU];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int64_t k = base + (int64_t)u * kBlock;
                const bool ok = k < ce;
                cj[u] = ok ? stream_load(col + k) : (I)0;
                vv[u] = stream_load(val + (ok ? k : cs));
            }
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int64_t k = base + (int64_t)u * kBlock;
                if (k < ce) stage.put((int)(k - cs), (int)cj[u], vv[u]);
            }
        }
        __syncthreads();

        const int64_t lo = start > cs ? start : cs, hi = end < ce ? end : ce;
        if (col_ok && lo < hi) {
            int i = (int)(lo - cs) + ep;
            const int iend = (int)(hi - cs);
            const int pos0 = (int)cs;        // (nnz < 2^31: the entry points refuse more)
            for (; i + (U - 1) * EP < iend; i += U * EP) {
                int j[U];
                Acc a[U];
                Acc b[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) stage.get(i + u * EP, j[u], a[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) load_vec<V, VEC>(B + row_off(j[u], ldb), b[u]);
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) take(v, a[u] + b[u][v], pos0 + i + u * EP);
                }
            }
            for (; i < iend; i += EP) {
                int j;
                Acc a;
                Acc b[VEC];
                stage.get(i, j, a);
                load_vec<V, VEC>(B + row_off(j, ldb), b);
#pragma unroll
                for (int v = 0; v < VEC; ++v) take(v, a + b[v], pos0 + i);
            }
        }
    }

    if constexpr (LOG) {
        if constexpr (EP > 1) {
#pragma unroll
            for (int m = CL; m < GROUP; m <<= 1) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const Acc m2 = shfl_xor_acc(x[v], m), s2 = shfl_xor_acc(s[v], m);
                    lse_combine<Acc>(x[v], s[v], m2, s2);
                }
            }
        }
        if (row_ok && col_ok && ep == 0) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) x[v] = lse_finish<Acc>(x[v], s[v], 0);
            store_vec<V, VEC, true>(static_cast<V*>(P.out) + row * P.ldout + cbase, x);
            if (P.cacc) store_acc<Acc, VEC>(static_cast<Acc*>(P.cacc) + row * P.ldacc + cbase, x);
        }
    } else {
        // a lane whose candidates all equal the identity took none of them: its first entry (position start + ep) is the winner
        if (col_ok && start + ep < end) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) arg[v] = arg[v] < 0 ? (int)(start + ep) : arg[v];
        }
        if constexpr (EP > 1) {
#pragma unroll
            for (int m = CL; m < GROUP; m <<= 1) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const Acc ob = shfl_xor_acc(x[v], m);
                    const int oa = __shfl_xor(arg[v], m, kWave);
                    reduce_merge<Acc>(x[v], arg[v], ob, oa, MIN);
                }
            }
        }
        if (row_ok && col_ok && ep == 0) {      // (a row without entries keeps the identity and arg = -1)
            store_vec<V, VEC, true>(static_cast<V*>(P.out) + row * P.ldout + cbase, x);
            store_arg<VEC>(P.arg + row * P.ldarg + cbase, arg);
        }
    }
}

// ---- gradient of the values -----------------------------------------------------------------------------------------------------
// dval[e] = Σ_c G[i,c]·W[e,c] for the entries e of row i.  A group of CL lanes × EP entry lanes owns the row; a lane owns the columns
// (t·CL + cl)·VEC .. +VEC of every column tile t and keeps G and C (arg) of its first tile in registers.  An entry's sum runs over
// the lane's columns in increasing order, tile after tile in place, then over the CL lanes in the butterfly of group_sum.
// log: U entries' gathers of B are in flight together.  Tropical: no gather of B, G selected where arg == e.
template <typename V, typename I, int VEC, int CL, int EP, int SR>
__global__ __launch_bounds__(kBlock) void csr_semiring_mm_bwd_values_kernel(const SemiringParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int TW = CL * VEC;
    constexpr int U = 2;

    const int tid = threadIdx.x;
    const int gl = tid % GROUP;
    const int cl = gl % CL;
    const int ep = gl / CL;
    const int64_t row = (int64_t)blockIdx.x * RPB + tid / GROUP;
    if (row >= P.n_groups) return;     // (a whole lane group leaves: the cross-lane sums below stay inside a group)

    const I* __restrict__ crow = static_cast<const I*>(P.ptr);
    const I* __restrict__ col = static_cast<const I*>(P.idx);
    const V* __restrict__ G = static_cast<const V*>(P.G) + row * P.ldg;
    V* __restrict__ dval = static_cast<V*>(P.out);
    const int64_t start = (int64_t)crow[row], end = (int64_t)crow[row + 1];
    if (start == end) return;
    const int64_t c0 = (int64_t)cl * VEC;

    if constexpr (SR == kSemiringLog) {
        const V* __restrict__ val = static_cast<const V*>(P.val);
        const V* __restrict__ B = static_cast<const V*>(P.B);
        const Acc* __restrict__ C = static_cast<const Acc*>(P.cacc) + row * P.ldacc;
        const uint32_t ldb = (uint32_t)P.ldb;
        Acc g0[VEC], k0[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) g0[v] = 0, k0[v] = 0;
        if (c0 < P.p) {
            load_vec<V, VEC>(G + c0, g0);
            load_acc<Acc, VEC>(C + c0, k0);
        }
        for (int64_t base = start; base < end; base += (int64_t)EP * U) {
            int64_t e[U];
            int j[U];
            Acc a[U], sum[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                e[u] = base + (int64_t)u * EP + ep;
                const bool in = e[u] < end;
                j[u] = in ? (int)col[e[u]] : (int)col[start];
                a[u] = in ? VT<V>::up(val[e[u]]) : -(Acc)INFINITY;      // (an entry past the row is an absent one: weight 0)
                sum[u] = 0;
            }
            for (int64_t c = c0; c < P.p; c += TW) {
                Acc g[VEC], k[VEC], b[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) load_vec<V, VEC>(B + row_off(j[u], ldb) + c, b[u]);
                if (c == c0) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) g[v] = g0[v], k[v] = k0[v];
                } else {
                    load_vec<V, VEC>(G + c, g);
                    load_acc<Acc, VEC>(C + c, k);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) sum[u] += lse_term<Acc>(g[v], a[u] + b[u][v], k[v]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Acc tot = group_sum<Acc, CL>(sum[u]);
                if (cl == 0 && e[u] < end) dval[e[u]] = VT<V>::down(tot);
            }
        }
    } else {
        const int* __restrict__ arg = P.arg + row * P.ldarg;
        Acc g0[VEC];
        int a0[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) g0[v] = 0, a0[v] = -1;
        if (c0 < P.p) {
            load_vec<V, VEC>(G + c0, g0);
            load_arg<VEC>(arg + c0, a0);
        }
        for (int64_t base = start; base < end; base += EP) {
            const int64_t e = base + ep;
            const int ei = e < end ? (int)e : -2;        // (-2 matches nothing)
            Acc sum = 0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) sum += a0[v] == ei ? g0[v] : (Acc)0;
            for (int64_t c = c0 + TW; c < P.p; c += TW) {
                int a[VEC];
                load_arg<VEC>(arg + c, a);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (a[v] == ei) sum += VT<V>::up(G[c + v]);
                }
            }
            sum = group_sum<Acc, CL>(sum);
            if (cl == 0 && e < end) dval[e] = VT<V>::down(sum);
        }
    }
}

// ---- gradient of B --------------------------------------------------------------------------------------------------------------
// dB[j,c] = Σ_{entries t of column j, in stored order} G[i,c]·W[e,c] with i = tidx[t], e = perm[t]: the forward's lane layout over
// the transposed pattern (grid.z slices the columns); B[j,·] of the lane's columns stays in registers.  log: every entry gathers
// G[i,·] and C[i,·] and recomputes the weight from val[e].  Tropical: 16 bytes of arg[i,·] per entry, G only where one matches.
template <typename V, typename I, int VEC, int CL, int EP, int SR>
__global__ __launch_bounds__(kBlock) void csr_semiring_mm_bwd_dense_kernel(const SemiringParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int U = SR == kSemiringLog ? 2 : 4;

    const int tid = threadIdx.x;
    const int gl = tid % GROUP;
    const int cl = gl % CL;
    const int ep = gl / CL;
    const int64_t j = xcd_chunked_block(blockIdx.x, P.nblocks) * RPB + tid / GROUP;
    const int64_t cbase = ((int64_t)blockIdx.z * CL + cl) * VEC;
    const bool ok = j < P.n_groups && cbase < P.p;

    const I* __restrict__ tptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ tidx = static_cast<const I*>(P.idx);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const V* __restrict__ G = static_cast<const V*>(P.G) + cbase;
    const uint32_t ldg = (uint32_t)P.ldg;

    Acc acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0;

    if (ok) {
        const int64_t end = (int64_t)tptr[j + 1];
        if constexpr (SR == kSemiringLog) {
            const V* __restrict__ val = static_cast<const V*>(P.val);
            const Acc* __restrict__ C = static_cast<const Acc*>(P.cacc) + cbase;
            const uint32_t ldacc = (uint32_t)P.ldacc;
            Acc b[VEC];
            load_vec<V, VEC>(static_cast<const V*>(P.B) + j * P.ldb + cbase, b);
            for (int64_t t = (int64_t)tptr[j] + ep; t < end; t += (int64_t)U * EP) {
                int i[U];
                Acc a[U], g[U][VEC], k[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t q = t + (int64_t)u * EP;
                    const bool in = q < end;
                    i[u] = (int)tidx[in ? q : t];
                    a[u] = in ? VT<V>::up(val[perm[q]]) : -(Acc)INFINITY;      // (past the column: an absent entry, weight 0)
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    load_vec<V, VEC>(G + row_off(i[u], ldg), g[u]);
                    load_acc<Acc, VEC>(C + row_off(i[u], ldacc), k[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) acc[v] += lse_term<Acc>(g[u][v], a[u] + b[v], k[u][v]);
                }
            }
        } else {
            const int* __restrict__ arg = P.arg + cbase;
            const uint32_t ldarg = (uint32_t)P.ldarg;
            for (int64_t t = (int64_t)tptr[j] + ep; t < end; t += (int64_t)U * EP) {
                int i[U], e[U];
                int a[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t q = t + (int64_t)u * EP;
                    const bool in = q < end;
                    i[u] = in ? (int)tidx[q] : -1;
                    e[u] = in ? (int)perm[q] : -2;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (i[u] >= 0) {
                        load_arg<VEC>(arg + row_off(i[u], ldarg), a[u]);
                    } else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) a[u][v] = -1;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bool any = false;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) any = any | (a[u][v] == e[u]);
                    if (any) {
                        Acc g[VEC];
                        load_vec<V, VEC>(G + row_off(i[u], ldg), g);
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] += a[u][v] == e[u] ? g[v] : (Acc)0;
                    }
                }
            }
        }
    }
    if constexpr (EP > 1) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = ep_sum<Acc, CL, EP>(acc[v]);
    }
    if (ok && ep == 0) store_vec<V, VEC, true>(static_cast<V*>(P.out) + j * P.ldout + cbase, acc);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
enum { kSemiringFwd = 0, kSemiringBwdValues = 1, kSemiringBwdDense = 2 };

template <typename V, typename I, int KIND>
int semiring_launch(SemiringParams P, int semiring, bool can_wide, hipStream_t stream) {
    const RowGeom g = mm_reduce_geom<V>(P.p, can_wide);
    const int64_t rpb = spmm_rows_per_block(g);
    P.nblocks = (P.n_groups + rpb - 1) / rpb;
    const int64_t tiles = KIND == kSemiringBwdValues ? 1 : g.col_tiles;
    if (P.nblocks > 0x7fffffffLL || tiles > 65535) return TSGU_ERR_TOO_LARGE;
    const dim3 grid((unsigned)P.nblocks, 1, (unsigned)tiles);
    return dispatch_geom(g, [&](auto cl, auto ep) -> int {
        constexpr int CL = decltype(cl)::value, EP = decltype(ep)::value;
        auto go = [&](auto vecw, auto sr) {
            constexpr int VECW = decltype(vecw)::value, SR = decltype(sr)::value;
            if constexpr (KIND == kSemiringFwd)
                hipLaunchKernelGGL((csr_semiring_mm_kernel<V, I, VECW, CL, EP, SR>), grid, dim3(kBlock), 0, stream, P);
            else if constexpr (KIND == kSemiringBwdValues)
                hipLaunchKernelGGL((csr_semiring_mm_bwd_values_kernel<V, I, VECW, CL, EP, SR>), grid, dim3(kBlock), 0, stream, P);
            else hipLaunchKernelGGL((csr_semiring_mm_bwd_dense_kernel<V, I, VECW, CL, EP, SR>), grid, dim3(kBlock), 0, stream, P);
        };
        auto with_sr = [&](auto vecw) {
            if (semiring == kSemiringLog) go(vecw, std::integral_constant<int, kSemiringLog>{});
            else if (semiring == kSemiringMax) go(vecw, std::integral_constant<int, kSemiringMax>{});
            else go(vecw, std::integral_constant<int, kSemiringMin>{});
        };
        if (g.vec == 1) with_sr(std::integral_constant<int, 1>{});
        else with_sr(std::integral_constant<int, VT<V>::kWide>{});
        return check_launch();
    });
}

}  // namespace tsgu
