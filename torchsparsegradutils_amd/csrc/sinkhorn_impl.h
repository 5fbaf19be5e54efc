// The half steps of a Sinkhorn iteration over a sparse pattern, their adjoints and the transport plan (sparse_sinkhorn).
//
// A half step is the range walk of logsumexp_impl.h (seg_stage, seg_walk, seg_merge_kernel) with "add the other side's potential,
// gathered through the secondary index" as the staging functor, the (max, Σ exp) partial of MaxSumExp with the sums inside a piece
// compensated (MaxSumExpK below), and a finish that writes log_marginal − lse: one read of the value and of its secondary index per entry (plus the perm in the column direction), no
// per-entry output, so no fix-up launch.
//
// The adjoint of a half step is a walk in the direction of the sum it produces.  The softmax weight of an entry is recomputed from
// the potentials, exp(val + pot_group + pot_other − log_marg_other): its argument is ≤ 0 up to rounding because every potential
// is applied BEFORE the exponential, which needs the entry's own group while it is staged — the plan's expanded primary index
// (`grp`, cached with the pattern).  The staging functor subtracts the term from the gradient buffer (distinct positions: a plain
// read-modify-write) and stages it; the walk reduces the staged terms with a plain, compensated sum (PlainSum) and the finish writes the
// outgoing cotangent.  tsgu_segment_sum is the same walk over the values themselves.
//
// The walk, its operation interface and the merge are used as they are: the log-sum-exp and softmax kernels do not change.
// No float atomics anywhere: the same inputs give the same bits.
#pragma once

#include "logsumexp_impl.h"
#include "softmax_impl.h"   // sm_wave_sync

namespace tsgu {

// ---- forward half step -----------------------------------------------------------------------------------------------------
template <typename V>
struct SkHalf {
    using Acc = typename VT<V>::Acc;
    const void* ptr;        // [n_groups + 1]
    const void* perm;       // [nnz] or null: entry k is val[perm[k]]
    const void* idx;        // [nnz]: the other direction's group of entry k
    const V* val;
    const Acc* other;       // the other side's potential
    const Acc* log_marg;    // [n_groups] or null (zeros)
    Acc* out;               // [n_groups]
    void* part;             // Acc[n_ranges][kSegSlots], or null: no group crosses a range boundary
    int64_t* tail;          // [n_ranges]
    int64_t n_groups, nnz, n_ranges;
    int vec_ok;             // val is 16-byte aligned
};

// One step of a compensated (Kahan) sum: `c` carries what the addition lost.  The build keeps floating-point contraction off and
// has no fast-math, so the compiler does not reassociate it away.
template <typename Acc>
__device__ __forceinline__ void kahan_add(Acc& sum, Acc& c, Acc x) {
    const Acc y = x - c;
    const Acc t = sum + y;
    c = (t - sum) - y;
    sum = t;
}

// MaxSumExp with compensated sums inside a piece: the sum of a long group then carries a few roundings instead of one per term of
// the longest chain.  The reverse sweep divides every weight of a group by this sum, so its error is an error of the whole
// gradient.  (The log-sum-exp and softmax kernels keep MaxSumExp itself: their bits do not change.)
template <typename A>
struct MaxSumExpK : MaxSumExp<A> {
    using Acc = A;
    using Part = typename MaxSumExp<A>::Part;
    static __device__ __forceinline__ Part lane_reduce(const Acc* st, int lo, int hi) {
        Acc m = -(Acc)INFINITY;
        for (int i = lo; i < hi; ++i) m = nanmax(m, st[i]);
        Acc sum = Acc(0), c = Acc(0);
        if (finite_acc(m)) {
            for (int i = lo; i < hi; ++i) kahan_add(sum, c, acc_exp(st[i] - m));
        }
        return {m, sum};
    }
    static __device__ __forceinline__ Part wave_reduce(const Acc* st, int lo, int hi, int lane) {
        Acc m = -(Acc)INFINITY;
        for (int i = lo + lane; i < hi; i += kWave) m = nanmax(m, st[i]);
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) m = nanmax(m, shfl_xor_acc(m, o));
        Acc sum = Acc(0), c = Acc(0);
        if (finite_acc(m)) {
            for (int i = lo + lane; i < hi; i += kWave) kahan_add(sum, c, acc_exp(st[i] - m));
        }
        return {m, group_sum<Acc, kWave>(sum)};
    }
};

// A finished group is one potential, written by one lane.
template <typename V>
struct SkHalfOp : MaxSumExpK<typename VT<V>::Acc> {
    using Acc = typename VT<V>::Acc;
    using Part = typename MaxSumExp<Acc>::Part;
    using Params = SkHalf<V>;
    const Params& P;
    __device__ __forceinline__ explicit SkHalfOp(const Params& p) : P(p) {}
    static __device__ __forceinline__ void store_group(const Params& P, int64_t g, Part p) {
        const Acc lm = P.log_marg ? P.log_marg[g] : Acc(0);
        P.out[g] = lm - lse_finish(p.m, p.s, (int64_t)0);
    }
    __device__ __forceinline__ void lane_finish(Acc*, int, int, int64_t g, int64_t, Part p) const { store_group(P, g, p); }
    __device__ __forceinline__ void wave_finish(Acc*, int, int, int64_t g, int64_t, Part p, int lane) const {
        if (lane == 0) store_group(P, g, p);
    }
    static __device__ __forceinline__ void merged_finish(const Params& P, Acc*, int64_t g, int64_t, Part p) { store_group(P, g, p); }
};

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sk_half_kernel(SkHalf<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    __shared__ Acc stage[kLseWavesPerBlock][R];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const Acc* __restrict__ other = P.other;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    if (w >= P.n_ranges) return;   // (no workgroup barrier below: a wave only reads what it staged itself)
    Acc* st = stage[wid];
    const int64_t s = w * R;
    seg_stage<V, I>(st, P.val, perm, s, seg_len<Acc>(w, P.nnz), P.vec_ok != 0, lane,
                    // (a stored −inf is an absent entry, also beside the +inf potential of a group that holds nothing else)
                    // (the gather stays unconditional: a select, not a branch around the load)
                    [&](Acc v, int i) {
                        const Acc t = v + other[(int64_t)idx[s + i]];
                        return v == -(Acc)INFINITY ? v : t;
                    });
    sm_wave_sync();
    seg_walk(st, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, P.part ? static_cast<Acc*>(P.part) + w * kSegSlots : nullptr, P.tail,
             SkHalfOp<V>(P));
}

// ---- the plain-sum partial --------------------------------------------------------------------------------------------------
// Lane-strided with a compensated sum (the terms of a cotangent's sum cancel), then group_sum across the wave; partials of a
// crossing group merge in range order.
template <typename A>
struct PlainSum {
    using Acc = A;
    using Part = A;
    static __device__ __forceinline__ Part identity() { return Acc(0); }
    static __device__ __forceinline__ void combine(Part& a, Part b) { a += b; }
    static __device__ __forceinline__ Part wave_combine(Part p) { return group_sum<Acc, kWave>(p); }
    static __device__ __forceinline__ void put(Acc* slot, Part p) { slot[0] = p; }
    static __device__ __forceinline__ Part get(const Acc* slot) { return slot[0]; }
    static __device__ __forceinline__ Part lane_reduce(const Acc* st, int lo, int hi) {
        Acc sum = Acc(0), c = Acc(0);
        for (int i = lo; i < hi; ++i) kahan_add(sum, c, st[i]);
        return sum;
    }
    static __device__ __forceinline__ Part wave_reduce(const Acc* st, int lo, int hi, int lane) {
        Acc sum = Acc(0), c = Acc(0);
        for (int i = lo + lane; i < hi; i += kWave) kahan_add(sum, c, st[i]);
        return group_sum<Acc, kWave>(sum);
    }
};

// ---- backward half step -----------------------------------------------------------------------------------------------------
template <typename V>
struct SkBwd {
    using Acc = typename VT<V>::Acc;
    const void* ptr;
    const void* perm;
    const void* idx;
    const void* grp;             // [nnz]: the group of entry k (ptr expanded)
    const V* val;
    const Acc* pot_group;        // [n_groups]
    const Acc* pot_other;
    const Acc* log_marg_other;   // or null (zeros)
    const Acc* g_other;          // the cotangent that comes in, on the other direction's groups
    Acc* grad;                   // [nnz] in the values' own order: grad[k'] -= term
    Acc* g_out;                  // [n_groups]: the cotangent that goes out
    void* part;
    int64_t* tail;
    int64_t n_groups, nnz, n_ranges;
    int accumulate;
    int vec_ok;
};

template <typename V>
struct SkBwdOp : PlainSum<typename VT<V>::Acc> {
    using Acc = typename VT<V>::Acc;
    using Part = Acc;
    using Params = SkBwd<V>;
    const Params& P;
    __device__ __forceinline__ explicit SkBwdOp(const Params& p) : P(p) {}
    static __device__ __forceinline__ void store_group(const Params& P, int64_t g, Part sum) {
        P.g_out[g] = (P.accumulate ? P.g_out[g] : Acc(0)) - sum;
    }
    __device__ __forceinline__ void lane_finish(Acc*, int, int, int64_t g, int64_t, Part sum) const { store_group(P, g, sum); }
    __device__ __forceinline__ void wave_finish(Acc*, int, int, int64_t g, int64_t, Part sum, int lane) const {
        if (lane == 0) store_group(P, g, sum);
    }
    static __device__ __forceinline__ void merged_finish(const Params& P, Acc*, int64_t g, int64_t, Part sum) { store_group(P, g, sum); }
};

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sk_half_bwd_kernel(SkBwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    __shared__ Acc stage[kLseWavesPerBlock][R];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ grp = static_cast<const I*>(P.grp);
    const Acc* __restrict__ pg = P.pot_group;
    const Acc* __restrict__ po = P.pot_other;
    const Acc* __restrict__ lm = P.log_marg_other;
    const Acc* __restrict__ go = P.g_other;
    Acc* grad = P.grad;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    if (w >= P.n_ranges) return;
    Acc* st = stage[wid];
    const int64_t s = w * R;
    seg_stage<V, I>(st, P.val, perm, s, seg_len<Acc>(w, P.nnz), P.vec_ok != 0, lane, [&](Acc v, int i) {
        const int64_t k = s + i;
        const int64_t c = (int64_t)idx[k];
        const int64_t at = perm ? (int64_t)perm[k] : k;
        // (every potential inside the exponential: the argument is the logarithm of a softmax weight.  The group's potential is
        // added first: val + pot_group is the value the other direction's half step staged, and with pot_other = −lse of that
        // step the weights of one of ITS groups sum to one up to the rounding of the sum)
        const Acc x = ((v + pg[(int64_t)grp[k]]) + po[c]) - (lm ? lm[c] : Acc(0));
        // (a stored −inf is an absent entry: no weight, also where it is alone in its group and that group's −lse is +inf)
        const Acc term = v == -(Acc)INFINITY ? Acc(0) : go[c] * acc_exp(x);
        grad[at] -= term;
        return term;
    });
    sm_wave_sync();
    seg_walk(st, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, P.part ? static_cast<Acc*>(P.part) + w * kSegSlots : nullptr, P.tail,
             SkBwdOp<V>(P));
}

// ---- segmented sum ----------------------------------------------------------------------------------------------------------
template <typename A>
struct SegSum {
    const void* ptr;
    const void* perm;
    const A* val;
    const A* add;    // [n_groups] or null
    A* out;          // [n_groups]
    void* part;
    int64_t* tail;
    int64_t n_groups, nnz, n_ranges;
    int vec_ok;
};

template <typename A>
struct SegSumOp : PlainSum<A> {
    using Acc = A;
    using Part = A;
    using Params = SegSum<A>;
    const Params& P;
    __device__ __forceinline__ explicit SegSumOp(const Params& p) : P(p) {}
    static __device__ __forceinline__ void store_group(const Params& P, int64_t g, Part sum) {
        P.out[g] = (P.add ? P.add[g] : Acc(0)) + sum;
    }
    __device__ __forceinline__ void lane_finish(Acc*, int, int, int64_t g, int64_t, Part sum) const { store_group(P, g, sum); }
    __device__ __forceinline__ void wave_finish(Acc*, int, int, int64_t g, int64_t, Part sum, int lane) const {
        if (lane == 0) store_group(P, g, sum);
    }
    static __device__ __forceinline__ void merged_finish(const Params& P, Acc*, int64_t g, int64_t, Part sum) { store_group(P, g, sum); }
};

template <typename A, typename I>
__global__ void __launch_bounds__(kBlock) seg_sum_kernel(SegSum<A> P) {
    constexpr int R = lse_range<A>();
    __shared__ A stage[kLseWavesPerBlock][R];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    if (w >= P.n_ranges) return;
    A* st = stage[wid];
    seg_stage<A, I>(st, P.val, perm, w * R, seg_len<A>(w, P.nnz), P.vec_ok != 0, lane, [](A v, int) { return v; });
    sm_wave_sync();
    seg_walk(st, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, P.part ? static_cast<A*>(P.part) + w * kSegSlots : nullptr, P.tail,
             SegSumOp<A>(P));
}

// ---- the transport plan -----------------------------------------------------------------------------------------------------
template <typename V>
struct SkPlan {
    using Acc = typename VT<V>::Acc;
    const void* ptr;         // [n_groups + 1]: the groups of the stored order
    const void* idx;         // [nnz]
    const V* val;
    const Acc* pot_group;
    const Acc* pot_other;
    V* out;
    int64_t n_groups, nnz;
    int vec_ok;              // val and out are 16-byte aligned
};

// One streaming pass in the stored order: 64·kWide entries per wave, an entry's group searched in the wave's window of ptr (in
// LDS, as lse_bwd_kernel does; in global memory when more group starts fall inside the span).
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sk_plan_kernel(SkPlan<V> P) {
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

    int64_t r0 = 0, r1 = 0;
    bool staged = false;
    if (live) {
        r0 = wave_lower_bound(ptr, P.n_groups, s + 1, lane) - 1;
        r1 = wave_lower_bound(ptr, P.n_groups, e, lane) - 1;
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
            // (a stored −inf stays −inf, also beside the +inf potential of a group that holds nothing else)
            const Acc t = (v[j] + P.pot_group[a]) + P.pot_other[(int64_t)idx[k]];
            v[j] = v[j] == -(Acc)INFINITY ? v[j] : t;
        }
    }
    if (P.vec_ok && k0 + W <= e) {
        store_vec<V, W>(P.out + k0, v);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (k0 + j < e) P.out[k0 + j] = VT<V>::down(v[j]);
    }
}

}  // namespace tsgu
