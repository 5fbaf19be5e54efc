// CSR × dense with a max / min reduction over the stored entries of a row (torch.sparse.mm(A, B, "amax" / "amin")), and its two
// gradient kernels.  The forward keeps the row-group layout of spmm_impl.h — a group of CL×EP lanes owns a row, the workgroup's
// contiguous (col, val) slice is staged in LDS with coalesced loads in passes of kStageCap entries, the dense rows are gathered
// with 16-byte loads, grid.z slices the columns — but a lane carries (best, arg) per column instead of a sum:
//   * candidates are the products val[e]·B[col[e],k] of the STORED entries only, formed in the accumulator type;
//   * a candidate replaces the running one on a strict > / < only, so of equal candidates (+0.0 and -0.0 among them) the one at
//     the lowest stored position stays; a NaN replaces any number and then stays (compare-and-select: the hardware max / min
//     instructions order the zeros and drop NaNs);
//   * the EP partials of a row are merged by (value, then lower position), which is the same rule and does not depend on the
//     order of the merge;
//   * C and arg (int32 position in A's value order, -1 for a row without entries) are written together.
// Both gradients flow through the winner only.  No atomics, no cross-workgroup communication, every sum in a fixed order.
#pragma once

#include "spmm_impl.h"

namespace tsgu {

struct MmReduceParams {
    int64_t n_groups, p;   // rows (forward, values pass) or columns of A (dense pass)
    const void* ptr;       // crow / tptr
    const void* idx;       // col / tidx
    const void* perm;      // dense pass: position of every transposed entry in A's value array
    const void* val;
    const void* B;
    int64_t ldb;
    const void* G;
    int64_t ldg;
    void* C;               // forward: C; values pass: dval; dense pass: dB
    int64_t ldc;
    int* arg;
    int64_t ldarg;
    int64_t nblocks;
    int op;                // 0 = amax, 1 = amin
};

// ---- VEC consecutive int32 of an arg row (VEC > 1: the address is a multiple of 4·VEC bytes, at most 16-byte accesses) --------
template <int VEC>
__device__ __forceinline__ void load_arg(const int* __restrict__ ptr, int (&out)[VEC]) {
    if constexpr (VEC == 1) {
        out[0] = *ptr;
    } else if constexpr (VEC == 2) {
        const int2 r = *reinterpret_cast<const int2*>(ptr);
        out[0] = r.x, out[1] = r.y;
    } else {
#pragma unroll
        for (int q = 0; q < VEC; q += 4) {
            const int4 r = *reinterpret_cast<const int4*>(ptr + q);
            out[q] = r.x, out[q + 1] = r.y, out[q + 2] = r.z, out[q + 3] = r.w;
        }
    }
}

template <int VEC>
__device__ __forceinline__ void store_arg(int* __restrict__ ptr, const int (&in)[VEC]) {
    if constexpr (VEC == 1) {
        *ptr = in[0];
    } else if constexpr (VEC == 2) {
        *reinterpret_cast<int2*>(ptr) = make_int2(in[0], in[1]);
    } else {
#pragma unroll
        for (int q = 0; q < VEC; q += 4) *reinterpret_cast<int4*>(ptr + q) = make_int4(in[q], in[q + 1], in[q + 2], in[q + 3]);
    }
}

// One candidate x at stored position pos (positions arrive in increasing order): strict compare, first wins, NaN sticky.
// `best` starts at the identity (-inf for max, +inf for min), so no "is this the first candidate" test is needed here; candidates
// equal to the identity are never taken, which the kernel repairs after the walk (the lane's first entry is then the winner).
// !(x <= best) is true for x > best and for a NaN on either side; (best == best) keeps a NaN that is already there.  Two
// compares, one scalar and, two selects per element: the forward is otherwise bound by these instructions, not by memory.
template <bool MIN, typename Acc>
__device__ __forceinline__ void reduce_take(Acc& best, int& arg, Acc x, int pos) {
    const bool not_better = MIN ? (x >= best) : (x <= best);
    const bool take = !not_better & (best == best);
    best = take ? x : best;
    arg = take ? pos : arg;
}

// Merge of two partial results of one row in any order: the better value, of equal values (or two NaNs) the lower position.
template <typename Acc>
__device__ __forceinline__ void reduce_merge(Acc& best, int& arg, Acc ob, int oa, bool amin) {
    const bool a_nan = best != best, b_nan = ob != ob;
    const bool better = amin ? (ob < best) : (ob > best);              // (false when either is a NaN)
    const bool tie = (a_nan & b_nan) | (ob == best);
    const bool wins = (b_nan & !a_nan) | (!a_nan & better) | (tie & (oa < arg));
    const bool take = (oa >= 0) & ((arg < 0) | wins);
    best = take ? ob : best;
    arg = take ? oa : arg;
}

template <typename V, typename I, int VEC, int CL, int EP, bool MIN>
__global__ __launch_bounds__(kBlock) void csr_spmm_reduce_kernel(const MmReduceParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int U = 4;   // gathers issued back to back per lane
    constexpr int SU = 4;  // staging loads issued back to back per thread

    __shared__ __attribute__((aligned(16))) unsigned char smem[StageBytes<V>::value];
    const Staged<V> stage(smem);

    const int tid = threadIdx.x;
    const int grp = tid / GROUP;
    const int gl = tid % GROUP;
    const int cl = gl % CL;
    const int ep = gl / CL;
    constexpr bool amin = MIN;

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

    Acc best[VEC];
    int arg[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) best[v] = MIN ? (Acc)INFINITY : -(Acc)INFINITY, arg[v] = -1;

    // the workgroup's slice [blk_begin, blk_end) goes through the staging window in passes; a pass's loads are all issued before
    // its first LDS write.  Every pass visits a lane's entries in increasing position, so "first wins" holds across passes.
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
                    for (int v = 0; v < VEC; ++v) reduce_take<MIN, Acc>(best[v], arg[v], a[u] * b[u][v], pos0 + i + u * EP);
                }
            }
            for (; i < iend; i += EP) {
                int j;
                Acc a;
                Acc b[VEC];
                stage.get(i, j, a);
                load_vec<V, VEC>(B + row_off(j, ldb), b);
#pragma unroll
                for (int v = 0; v < VEC; ++v) reduce_take<MIN, Acc>(best[v], arg[v], a * b[v], pos0 + i);
            }
        }
    }

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
                const Acc ob = __shfl_xor(best[v], m, kWave);
                const int oa = __shfl_xor(arg[v], m, kWave);
                reduce_merge<Acc>(best[v], arg[v], ob, oa, amin);
            }
        }
    }
    if (row_ok && col_ok && ep == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) best[v] = arg[v] < 0 ? (Acc)0 : best[v];      // a row without entries
        store_vec<V, VEC, true>(static_cast<V*>(P.C) + row * P.ldc + cbase, best);
        store_arg<VEC>(P.arg + row * P.ldarg + cbase, arg);
    }
}

// dval[e] = Σ_{k: arg[i,k] = e} G[i,k]·B[col[e],k] for the entries e of row i.  A group of CL lanes × EP entry lanes owns the row;
// a lane owns the columns (t·CL + cl)·VEC .. +VEC of every column tile t and gathers B only where its column's winner is (p loads
// per row).  The first tile's contributions stay in registers; an entry's sum runs over the lane's columns in increasing order,
// then over the CL lanes in a fixed butterfly.  An entry that wins nothing sums zeros: exactly 0.
template <typename V, typename I, int VEC, int CL, int EP>
__global__ __launch_bounds__(kBlock) void csr_spmm_reduce_bwd_values_kernel(const MmReduceParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int TW = CL * VEC;

    const int tid = threadIdx.x;
    const int gl = tid % GROUP;
    const int cl = gl % CL;
    const int ep = gl / CL;
    const int64_t row = (int64_t)blockIdx.x * RPB + tid / GROUP;
    if (row >= P.n_groups) return;     // (a whole lane group leaves: the cross-lane sums below stay inside a group)

    const I* __restrict__ crow = static_cast<const I*>(P.ptr);
    const I* __restrict__ col = static_cast<const I*>(P.idx);
    const V* __restrict__ B = static_cast<const V*>(P.B);
    const V* __restrict__ G = static_cast<const V*>(P.G) + row * P.ldg;
    const int* __restrict__ arg = P.arg + row * P.ldarg;
    V* __restrict__ dval = static_cast<V*>(P.C);
    const uint32_t ldb = (uint32_t)P.ldb;
    const int64_t start = (int64_t)crow[row], end = (int64_t)crow[row + 1];
    if (start == end) return;

    auto contribution = [&](int64_t c, int e) -> Acc {   // column c, won by entry e
        return VT<V>::up(G[c]) * VT<V>::up(B[row_off((int)col[e], ldb) + c]);
    };

    const int64_t c0 = (int64_t)cl * VEC;
    Acc x0[VEC];
    int a0[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) x0[v] = 0, a0[v] = -1;
    if (c0 < P.p) {
        load_arg<VEC>(arg + c0, a0);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            // (a row with entries has a winner in every column; anything else in `arg` is not the forward's and matches no entry)
            if (a0[v] >= start && a0[v] < end) x0[v] = contribution(c0 + v, a0[v]);
        }
    }

    for (int64_t base = start; base < end; base += EP) {
        const int64_t e = base + ep;
        const int ei = e < end ? (int)e : -2;        // (-2 matches nothing)
        Acc s = 0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) s += a0[v] == ei ? x0[v] : (Acc)0;
        for (int64_t c = c0 + TW; c < P.p; c += TW) {
            int a[VEC];
            load_arg<VEC>(arg + c, a);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (a[v] == ei) s += contribution(c + v, ei);
            }
        }
        s = group_sum<Acc, CL>(s);
        if (cl == 0 && e < end) dval[e] = VT<V>::down(s);
    }
}

// dB[j,k] = Σ_{entries t of column j, in stored order: arg[i,k] = e} val[e]·G[i,k] with i = tidx[t], e = perm[t]: a gather over the
// transposed pattern in the forward's lane layout (grid.z slices the columns).  A lane reads the arg lanes of every entry of its
// column and G only where one of them points back at the entry.
template <typename V, typename I, int VEC, int CL, int EP>
__global__ __launch_bounds__(kBlock) void csr_spmm_reduce_bwd_dense_kernel(const MmReduceParams P) {
    using Acc = typename VT<V>::Acc;
    constexpr int GROUP = CL * EP;
    constexpr int RPB = kBlock / GROUP;
    constexpr int U = 4;

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
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* __restrict__ G = static_cast<const V*>(P.G) + cbase;
    const int* __restrict__ arg = P.arg + cbase;
    const uint32_t ldg = (uint32_t)P.ldg, ldarg = (uint32_t)P.ldarg;

    Acc acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0;

    if (ok) {
        const int64_t end = (int64_t)tptr[j + 1];
        for (int64_t t = (int64_t)tptr[j] + ep; t < end; t += (int64_t)U * EP) {
            int i[U], e[U];
            int a[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t k = t + (int64_t)u * EP;
                const bool in = k < end;
                i[u] = in ? (int)tidx[k] : -1;
                e[u] = in ? (int)perm[k] : -2;
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
                    const Acc w = VT<V>::up(val[e[u]]);
                    Acc g[VEC];
                    load_vec<V, VEC>(G + row_off(i[u], ldg), g);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        if (a[u][v] == e[u]) acc[v] = fma(w, g[v], acc[v]);
                    }
                }
            }
        }
    }
    if constexpr (EP > 1) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = ep_sum<Acc, CL, EP>(acc[v]);
    }
    if (ok && ep == 0) store_vec<V, VEC, true>(static_cast<V*>(P.C) + j * P.ldc + cbase, acc);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// The lane geometry of p columns of value type V; `can_wide`: every dense operand of the launch (arg included) is touched in
// aligned lanes of kWide elements.  Without it the lanes are scalar: no operand is refused for its alignment.
template <typename V>
inline RowGeom mm_reduce_geom(int64_t p, bool can_wide) {
    return pick_geom(VT<V>::kWide, can_wide && p % VT<V>::kWide == 0, p);
}

inline bool lanes_of(const void* ptr, int64_t ld, int wide) { return aligned16(ptr) && ld % wide == 0; }

enum { kMmReduceFwd = 0, kMmReduceBwdValues = 1, kMmReduceBwdDense = 2 };

template <typename V, typename I, int KIND>
int mm_reduce_launch(MmReduceParams P, bool can_wide, hipStream_t stream) {
    const RowGeom g = mm_reduce_geom<V>(P.p, can_wide);
    const int64_t rpb = spmm_rows_per_block(g);
    P.nblocks = (P.n_groups + rpb - 1) / rpb;
    const int64_t tiles = KIND == kMmReduceBwdValues ? 1 : g.col_tiles;
    if (P.nblocks > 0x7fffffffLL || tiles > 65535) return TSGU_ERR_TOO_LARGE;
    const dim3 grid((unsigned)P.nblocks, 1, (unsigned)tiles);
    return dispatch_geom(g, [&](auto cl, auto ep) -> int {
        constexpr int CL = decltype(cl)::value, EP = decltype(ep)::value;
        auto go = [&](auto vecw) {
            constexpr int VECW = decltype(vecw)::value;
            if constexpr (KIND == kMmReduceFwd) {
                if (P.op) hipLaunchKernelGGL((csr_spmm_reduce_kernel<V, I, VECW, CL, EP, true>), grid, dim3(kBlock), 0, stream, P);
                else hipLaunchKernelGGL((csr_spmm_reduce_kernel<V, I, VECW, CL, EP, false>), grid, dim3(kBlock), 0, stream, P);
            } else if constexpr (KIND == kMmReduceBwdValues)
                hipLaunchKernelGGL((csr_spmm_reduce_bwd_values_kernel<V, I, VECW, CL, EP>), grid, dim3(kBlock), 0, stream, P);
            else hipLaunchKernelGGL((csr_spmm_reduce_bwd_dense_kernel<V, I, VECW, CL, EP>), grid, dim3(kBlock), 0, stream, P);
        };
        if (g.vec == 1) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, VT<V>::kWide>{});
        return check_launch();
    });
}

}  // namespace tsgu
