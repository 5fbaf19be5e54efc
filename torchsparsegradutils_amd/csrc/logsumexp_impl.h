// Segmented reductions over a row-gather pattern: the range walk that sparse_logsumexp / sparse_bidir_logsumexp and sparse_softmax /
// sparse_log_softmax (softmax_impl.h) share, and the log-sum-exp kernels themselves.
//
// The walk.  The entries are cut into contiguous ranges of lse_range<Acc>() entries, one wave each (balanced by entries, not by
// groups: one group of 2^20 entries among short ones occupies 2^20 / range waves).  A wave stages its range in LDS as accumulator
// values (seg_stage: 16-byte loads, or through `perm` for the column direction), then seg_walk reduces every group it owns — the
// groups whose first entry lies in the range — lane per group for short ones and the whole wave for long ones.  A group that runs
// past the range leaves a partial in the wave's tail slot, and every later wave it reaches leaves one in its head slot;
// seg_merge_kernel merges those partials in a fixed order, and for operators with one value per entry seg_fix_kernel rewrites the
// entries of the crossing pieces.  No float atomics: the same inputs give the same bits.  What is reduced and what happens to a
// finished group comes from an operation object (MaxSumExp, LseOp here; SmFwdOp, SmBwdOp in softmax_impl.h).
//
// Log-sum-exp forward.  The (max, Σ exp) partial; a finished group is one value, written by one lane.  A direction computed alone
// or as half of the bidirectional call is the same kernel with the same operands.
//
// Log-sum-exp backward.  One streaming pass in the stored order: each entry finds its primary group from `ptr` (a search in the wave's
// window of ptr, staged in LDS), reads the secondary index only when that direction is present, and gathers g / lse of the
// groups it belongs to.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

// LDS bytes of one wave's staged range (as accumulator values)
constexpr int kLseStageBytes = 8192;
template <typename Acc>
constexpr int lse_range() { return kLseStageBytes / (int)sizeof(Acc); }
// owned groups up to this many entries are reduced by one lane each; longer ones by the whole wave
constexpr int kLseLaneMax = 48;
constexpr int kLseWavesPerBlock = kBlock / kWave;
// workspace words of one range: the head partial from word 0, the tail partial (after the merge: the group's result) from kSegTail
constexpr int kSegSlots = 4;
constexpr int kSegTail = 2;

// max that propagates NaN (a NaN value makes its group NaN)
template <typename Acc>
__device__ __forceinline__ Acc nanmax(Acc a, Acc b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ float acc_exp(float x) { return expf(x); }
__device__ __forceinline__ double acc_exp(double x) { return exp(x); }
__device__ __forceinline__ float acc_log(float x) { return logf(x); }
__device__ __forceinline__ double acc_log(double x) { return log(x); }

template <typename Acc>
__device__ __forceinline__ bool finite_acc(Acc x) { return __builtin_isfinite(x); }

// (m, s): m = max of the values (NaN if any is NaN), s = sum exp(v - m) when m is finite, else 0
template <typename Acc>
__device__ __forceinline__ void lse_combine(Acc& m, Acc& s, Acc m2, Acc s2) {
    const Acc mm = nanmax(m, m2);
    if (finite_acc(mm)) {
        const Acc a = finite_acc(m) ? s * acc_exp(m - mm) : Acc(0);
        const Acc b = finite_acc(m2) ? s2 * acc_exp(m2 - mm) : Acc(0);
        s = a + b;
    } else {
        s = Acc(0);
    }
    m = mm;
}

// The group's value from its (m, s) and its count of absent entries (each an exp(0) term).  Edge cases as the reference:
// NaN -> NaN, +inf -> +inf, nothing at all -> -inf; the shift is max(m, 0) when absent entries count.
template <typename Acc>
__device__ __forceinline__ Acc lse_finish(Acc m, Acc s, int64_t zeros) {
    if (m != m) return m;
    const Acc inf = (Acc)INFINITY;
    if (m == inf) return m;
    if (zeros > 0) {
        const Acc M = m > Acc(0) ? m : Acc(0);
        const Acc t = (m > -inf ? s * acc_exp(m - M) : Acc(0)) + (Acc)zeros * acc_exp(-M);
        return M + acc_log(t);
    }
    if (m == -inf) return -inf;
    return m + acc_log(s);
}

// first g in [0, n] with p[g] >= x (p non-decreasing, p[n] >= x), searched by the whole wave 64 probes at a time
template <typename I>
__device__ __forceinline__ int64_t wave_lower_bound(const I* __restrict__ p, int64_t n, int64_t x, int lane) {
    int64_t lo = -1, hi = n;  // p[lo] < x (lo = -1: virtual), p[hi] >= x
    while (hi - lo > 1) {
        const int64_t step = (hi - lo - 1 + kWave - 1) / kWave;
        const int64_t q = lo + (int64_t)(lane + 1) * step;
        const bool ge = q >= hi || (int64_t)p[q] >= x;
        const unsigned long long mask = __ballot(ge);
        if (mask == 0) {
            lo += (int64_t)kWave * step;
        } else {
            const int f = __builtin_ctzll(mask);
            const int64_t nh = lo + (int64_t)(f + 1) * step;
            hi = nh < hi ? nh : hi;
            lo += (int64_t)f * step;
        }
    }
    return hi;
}

// ---- the walk ------------------------------------------------------------------------------------------------------------
// An operation object `Op` supplies what differs between the operators:
//   Op::Acc, Op::Part, Op::Params      accumulator type, partial of a piece, the kernels' parameter block
//   identity(), combine(a, b), wave_combine(p), put(slot, p), get(slot)      partials: merging them, and their workspace form
//   lane_reduce(st, lo, hi), wave_reduce(st, lo, hi, lane)                   st[lo, hi) by one lane / by the whole wave (every lane: p)
//   lane_finish(st, lo, hi, g, count, p), wave_finish(..., p, lane)          group g of `count` entries ends in the range
// and, as static functions of the parameter block (the merge and fix-up kernels walk nothing and build no object):
//   merged_finish(P, slot, g, count, p)                                      a crossing group's merged partial, at its owner's tail slot
//   merged(slot), fix(P, at, t)                                              (one value per entry) entry `at` of a crossing group

// entries of range w
template <typename Acc>
__device__ __forceinline__ int seg_len(int64_t w, int64_t nnz) {
    constexpr int R = lse_range<Acc>();
    const int64_t s = w * R;
    return (int)((s + R < nnz ? s + R : nnz) - s);
}

// The wave's `len` entries from `s` of `src` (through perm when given) into LDS as accumulator values, f applied to each.
template <typename V, typename I, typename F>
__device__ __forceinline__ void seg_stage(typename VT<V>::Acc* st, const V* __restrict__ src, const I* __restrict__ perm, int64_t s,
                                          int len, bool vec, int lane, F f) {
    using Acc = typename VT<V>::Acc;
    constexpr int W = VT<V>::kWide;
    if (perm == nullptr && vec) {
        for (int i = lane * W; i < len; i += kWave * W) {
            if (i + W <= len) {
                Acc v[W];
                load_vec<V, W>(src + s + i, v);
#pragma unroll
                for (int j = 0; j < W; ++j) st[i + j] = f(v[j], i + j);
            } else {
                for (int j = i; j < len; ++j) st[j] = f(VT<V>::up(src[s + j]), j);
            }
        }
    } else if (perm == nullptr) {
        for (int i = lane; i < len; i += kWave) st[i] = f(VT<V>::up(src[s + i]), i);
    } else {
        for (int i = lane; i < len; i += kWave) st[i] = f(VT<V>::up(src[(int64_t)perm[s + i]]), i);
    }
}

// The head rule: entry s of the range that starts at s belongs to a group that started in an earlier range when ga — the first
// group that starts at or after s — starts after s.  The head piece then ends at ptr[ga] or at the range's end.
template <typename I>
__device__ __forceinline__ bool seg_has_head(const I* __restrict__ ptr, int64_t n_groups, int64_t nnz, int64_t s, int64_t ga) {
    return s < nnz && (ga == n_groups || (int64_t)ptr[ga] > s);
}

// One wave over its staged range w: the head piece, then the owned groups [ga, gb) — first entry in [s, e); the last range also
// owns the empty groups at the end.  `part`: the range's workspace slots, or null when the caller knows that no group crosses a
// range boundary; with it, tail[w] becomes the owned group that runs past the range, or -1.
template <typename Op, typename I>
__device__ __forceinline__ void seg_walk(typename Op::Acc* st, const I* __restrict__ ptr, int64_t n_groups, int64_t nnz, int64_t n_ranges,
                                         int64_t w, int lane, typename Op::Acc* part, int64_t* tail, const Op op) {
    using Part = typename Op::Part;
    constexpr int R = lse_range<typename Op::Acc>();
    const int64_t s = w * R, e = s + R < nnz ? s + R : nnz;
    const int64_t ga = wave_lower_bound(ptr, n_groups, s, lane);
    const int64_t gb = w == n_ranges - 1 ? n_groups : wave_lower_bound(ptr, n_groups, e, lane);

    const bool head = seg_has_head(ptr, n_groups, nnz, s, ga);
    if (head && part) {
        const int64_t hend = (int64_t)ptr[ga];
        const Part p = op.wave_reduce(st, 0, (int)((hend < e ? hend : e) - s), lane);
        if (lane == 0) Op::put(part, p);
    }
    int64_t tailg = -1;   // (wave-uniform)

    for (int64_t base = ga; base < gb; base += kWave) {
        const int64_t g = base + lane;
        const bool active = g < gb;
        const int64_t glo = active ? (int64_t)ptr[g] : s;
        const int64_t ghi = active ? (int64_t)ptr[g + 1] : s;
        const int lo = (int)(glo - s), hi = (int)((ghi < e ? ghi : e) - s);
        const bool wide = active && hi - lo > kLseLaneMax;
        if (active && !wide) {
            const Part p = op.lane_reduce(st, lo, hi);
            if (ghi <= e) op.lane_finish(st, lo, hi, g, ghi - glo, p);
            else if (part) Op::put(part + kSegTail, p);
        }
        const unsigned long long tmask = __ballot(active && !wide && ghi > e);
        if (tmask) tailg = base + __builtin_ctzll(tmask);
        unsigned long long mask = __ballot(wide);
        while (mask) {
            const int f = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int flo = __shfl(lo, f, kWave), fhi = __shfl(hi, f, kWave);
            const int64_t fglo = __shfl(glo, f, kWave), fghi = __shfl(ghi, f, kWave);
            const Part p = op.wave_reduce(st, flo, fhi, lane);
            if (fghi <= e) {
                op.wave_finish(st, flo, fhi, base + f, fghi - fglo, p, lane);
            } else {
                if (lane == 0 && part) Op::put(part + kSegTail, p);
                tailg = base + f;
            }
        }
    }
    if (lane == 0 && part) tail[w] = tailg;
}

// One wave per range: the range's tail group (if any) merges its partials — the range's tail slot, then the head slots of the
// later ranges it reaches — lane-strided and then across the wave in a fixed order; lane 0 finishes the group at that tail slot.
template <typename Op, typename I>
__global__ void __launch_bounds__(kBlock) seg_merge_kernel(typename Op::Params P) {
    using Acc = typename Op::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const int64_t g = P.tail[w];
    if (g < 0) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const int64_t glo = (int64_t)ptr[g], ghi = (int64_t)ptr[g + 1];
    const int64_t w1 = (ghi - 1) / R;
    Acc* part = static_cast<Acc*>(P.part);
    typename Op::Part p = Op::identity();
    for (int64_t j = lane; j <= w1 - w; j += kWave)
        Op::combine(p, Op::get(j == 0 ? part + w * kSegSlots + kSegTail : part + (w + j) * kSegSlots));
    p = Op::wave_combine(p);
    // (the only reader of this slot above is lane 0 itself)
    if (lane == 0) Op::merged_finish(P, part + w * kSegSlots + kSegTail, g, ghi - glo, p);
}

// One wave per range, for operators with one value per entry: the entries of its head piece (from the tail slot of the range that
// owns that group) and of its tail piece, read once more from global memory.
template <typename Op, typename I>
__global__ void __launch_bounds__(kBlock) seg_fix_kernel(typename Op::Params P) {
    using Acc = typename Op::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const Acc* part = static_cast<const Acc*>(P.part);
    const int64_t s = w * R, e = s + R < P.nnz ? s + R : P.nnz;
    auto piece = [&](int64_t lo, int64_t hi, int64_t owner) {
        const auto t = Op::merged(part + owner * kSegSlots + kSegTail);
        for (int64_t k = lo + lane; k < hi; k += kWave) Op::fix(P, perm ? (int64_t)perm[k] : k, t);
    };
    const int64_t tg = P.tail[w];
    if (w > 0) {   // (range 0 has no head; the search is skipped where the range starts on a group start)
        const int64_t ga = wave_lower_bound(ptr, P.n_groups, s, lane);
        if (seg_has_head(ptr, P.n_groups, P.nnz, s, ga)) {
            const int64_t hend = (int64_t)ptr[ga];
            piece(s, hend < e ? hend : e, (int64_t)ptr[ga - 1] / R);
        }
    }
    if (tg >= 0) piece((int64_t)ptr[tg], e, w);
}

// The (max, Σ exp) partial of log-sum-exp and of the softmax forward.  Max first and then the sum; across the wave the xor
// butterfly with nanmax, then group_sum.
template <typename A>
struct MaxSumExp {
    using Acc = A;
    struct Part {
        Acc m, s;
    };
    static __device__ __forceinline__ Part identity() { return {-(Acc)INFINITY, Acc(0)}; }
    static __device__ __forceinline__ void combine(Part& a, Part b) { lse_combine(a.m, a.s, b.m, b.s); }
    static __device__ __forceinline__ Part wave_combine(Part p) {
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const Acc m2 = shfl_xor_acc(p.m, o), s2 = shfl_xor_acc(p.s, o);
            lse_combine(p.m, p.s, m2, s2);
        }
        return p;
    }
    static __device__ __forceinline__ void put(Acc* slot, Part p) {
        slot[0] = p.m;
        slot[1] = p.s;
    }
    static __device__ __forceinline__ Part get(const Acc* slot) { return {slot[0], slot[1]}; }
    static __device__ __forceinline__ Part lane_reduce(const Acc* st, int lo, int hi) {
        Acc m = -(Acc)INFINITY;
        for (int i = lo; i < hi; ++i) m = nanmax(m, st[i]);
        Acc sum = Acc(0);
        if (finite_acc(m)) {
            for (int i = lo; i < hi; ++i) sum += acc_exp(st[i] - m);
        }
        return {m, sum};
    }
    static __device__ __forceinline__ Part wave_reduce(const Acc* st, int lo, int hi, int lane) {
        Acc m = -(Acc)INFINITY;
        for (int i = lo + lane; i < hi; i += kWave) m = nanmax(m, st[i]);
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) m = nanmax(m, shfl_xor_acc(m, o));
        Acc sum = Acc(0);
        if (finite_acc(m)) {
            for (int i = lo + lane; i < hi; i += kWave) sum += acc_exp(st[i] - m);
        }
        return {m, group_sum<Acc, kWave>(sum)};
    }
};

// ---- log-sum-exp forward -------------------------------------------------------------------------------------------------
template <typename V>
struct LseFwd {
    const void* ptr;     // [n_groups + 1]
    const void* perm;    // [nnz] or null: entry k is val[perm[k]]
    const V* val;
    V* out;
    void* part;          // Acc[n_ranges][kSegSlots]: head (m, s), tail (m, s)
    int64_t* tail;       // [n_ranges]: the owned group that runs past the range, or -1
    int64_t n_groups, nnz, n_ranges;
    int64_t axis_len;    // entries per group including the absent ones; < 0: absent entries do not count
    int64_t gpi, ostride;    // group g is written at out[(g / gpi) * ostride + g % gpi]; [gpi, ostride) of every item: -inf
    int vec_ok;          // val is 16-byte aligned (ranges start at multiples of the range length)
};

template <typename V>
__device__ __forceinline__ void lse_store(const LseFwd<V>& P, int64_t g, typename VT<V>::Acc r) {
    const int64_t o = P.ostride == P.gpi ? g : (g / P.gpi) * P.ostride + g % P.gpi;
    P.out[o] = VT<V>::down(r);
}

template <typename V>
__device__ __forceinline__ int64_t lse_zeros(const LseFwd<V>& P, int64_t count) {
    return P.axis_len < 0 ? 0 : P.axis_len - count;
}

// A finished group is one value, written by one lane.
template <typename V>
struct LseOp : MaxSumExp<typename VT<V>::Acc> {
    using Acc = typename VT<V>::Acc;
    using Part = typename MaxSumExp<Acc>::Part;
    using Params = LseFwd<V>;
    const Params& P;
    __device__ __forceinline__ explicit LseOp(const Params& p) : P(p) {}
    static __device__ __forceinline__ void store_group(const Params& P, int64_t g, int64_t count, Part p) {
        lse_store(P, g, lse_finish(p.m, p.s, lse_zeros(P, count)));
    }
    __device__ __forceinline__ void lane_finish(Acc*, int, int, int64_t g, int64_t count, Part p) const { store_group(P, g, count, p); }
    __device__ __forceinline__ void wave_finish(Acc*, int, int, int64_t g, int64_t count, Part p, int lane) const {
        if (lane == 0) store_group(P, g, count, p);
    }
    static __device__ __forceinline__ void merged_finish(const Params& P, Acc*, int64_t g, int64_t count, Part p) { store_group(P, g, count, p); }
};

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) lse_fwd_kernel(LseFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    __shared__ Acc stage[kLseWavesPerBlock][R];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);

    // the -inf tail of every output item (padded layout)
    if (P.ostride > P.gpi) {
        const int64_t per = P.ostride - P.gpi, total = (P.n_groups / P.gpi) * per;
        for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock)
            P.out[(i / per) * P.ostride + P.gpi + i % per] = VT<V>::down(-(Acc)INFINITY);
    }

    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    const bool live = w < P.n_ranges;   // (every wave reaches the barrier below)
    Acc* st = stage[wid];
    seg_stage<V, I>(st, P.val, perm, w * R, live ? seg_len<Acc>(w, P.nnz) : 0, P.vec_ok != 0, lane, [](Acc v, int) { return v; });
    __syncthreads();
    if (!live) return;
    seg_walk(st, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, static_cast<Acc*>(P.part) + w * kSegSlots, P.tail, LseOp<V>(P));
}

// ---- log-sum-exp backward ------------------------------------------------------------------------------------------------
template <typename V>
struct LseBwd {
    const void* ptr;      // [n1 + 1] primary groups in stored order, or null
    const V* g1;          // [n1]
    const V* lse1;        // [n1]
    const void* idx;      // [nnz] secondary group of every entry, or null
    const V* g2;          // [n2]
    const V* lse2;        // [n2]
    const V* val;
    V* grad;
    int64_t n1, nnz;
    int vec_ok;           // val and grad are 16-byte aligned
};

constexpr int kLseBwdWindow = 320;   // ptr entries of a wave's window staged in LDS (else: searched in global memory)

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) lse_bwd_kernel(LseBwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int W = VT<V>::kWide;
    constexpr int kPerWave = kWave * W;
    __shared__ int64_t win[kLseWavesPerBlock][kLseBwdWindow];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const int64_t s = ((int64_t)blockIdx.x * kLseWavesPerBlock + wid) * kPerWave;
    const bool live = s < P.nnz;   // (every wave reaches the barrier below)
    const int64_t e = !live ? s : s + kPerWave < P.nnz ? s + kPerWave : P.nnz;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);

    const int64_t k0 = s + (int64_t)lane * W;
    Acc v[W];
    if (P.vec_ok && k0 + W <= e) {
        load_vec<V, W>(P.val + k0, v);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = k0 + j < e ? VT<V>::up(P.val[k0 + j]) : Acc(0);
    }

    Acc out[W];
#pragma unroll
    for (int j = 0; j < W; ++j) out[j] = Acc(0);

    if (ptr != nullptr) {   // (block-uniform)
        // primary groups of the window: r0 holds entry s, r1 holds entry e - 1 (the last g with ptr[g] <= k)
        int64_t r0 = 0, r1 = 0;
        bool staged = false;
        if (live) {
            r0 = wave_lower_bound(ptr, P.n1, s + 1, lane) - 1;
            r1 = wave_lower_bound(ptr, P.n1, e, lane) - 1;
            const int64_t nw = r1 - r0 + 2;     // ptr[r0 .. r1 + 1]
            staged = nw <= kLseBwdWindow;
            if (staged)
                for (int64_t i = lane; i < nw; i += kWave) win[wid][i] = (int64_t)ptr[r0 + i];
        }
        __syncthreads();
        int64_t lo = r0;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t k = k0 + j;
            if (k < e) {
                // last g in [lo, r1] with ptr[g] <= k
                int64_t a = lo, b = r1;
                while (a < b) {
                    const int64_t mid = (a + b + 1) >> 1;
                    const int64_t pm = staged ? win[wid][mid - r0] : (int64_t)ptr[mid];
                    if (pm <= k) a = mid;
                    else b = mid - 1;
                }
                lo = a;
                out[j] += VT<V>::up(P.g1[a]) * acc_exp(v[j] - VT<V>::up(P.lse1[a]));
            }
        }
    }
    if (idx != nullptr) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t k = k0 + j;
            if (k < e) {
                const int64_t c = (int64_t)idx[k];
                out[j] += VT<V>::up(P.g2[c]) * acc_exp(v[j] - VT<V>::up(P.lse2[c]));
            }
        }
    }
    if (P.vec_ok && k0 + W <= e) {
        store_vec<V, W>(P.grad + k0, out);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (k0 + j < e) P.grad[k0 + j] = VT<V>::down(out[j]);
    }
}

// ---- host side: ranges and the workspace of the walk ----------------------------------------------------------------------
// entries per range of a value type; -1: not a value type of these kernels
inline int64_t seg_range_of(int vtype) {
    if (vtype == TSGU_F32 || vtype == TSGU_BF16) return lse_range<float>();
    if (vtype == TSGU_F64) return lse_range<double>();
    return -1;
}

inline int64_t seg_ranges(int64_t range, int64_t nnz) { return nnz > 0 ? (nnz + range - 1) / range : 1; }

// workgroups of a kernel with one wave per range
inline int64_t seg_blocks(int64_t n_ranges) { return (n_ranges + kLseWavesPerBlock - 1) / kLseWavesPerBlock; }

// Acc[n_ranges][kSegSlots] and the tail groups int64[n_ranges]; -1: not a value type
inline int64_t seg_ws_bytes(int vtype, int64_t nnz) {
    const int64_t range = seg_range_of(vtype);
    if (range < 0) return -1;
    return seg_ranges(range, nnz) * (int64_t)(kSegSlots * (kLseStageBytes / range) + sizeof(int64_t));
}

// point `part` and `tail` of a parameter block (n_ranges set) into the workspace; both null without one
template <typename Acc, typename Params>
inline void seg_set_workspace(Params& p, void* workspace) {
    p.part = workspace;
    p.tail = workspace ? reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + p.n_ranges * kSegSlots * sizeof(Acc)) : nullptr;
}

}  // namespace tsgu
