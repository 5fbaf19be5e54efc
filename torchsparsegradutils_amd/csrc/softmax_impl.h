// Segmented softmax / log-softmax over a row-gather pattern and its gradient (sparse_softmax / sparse_log_softmax).
//
// Both kernels are the range walk of logsumexp_impl.h (seg_stage, seg_walk, seg_merge_kernel, seg_fix_kernel) with an operation
// object of their own.  Unlike a reduction, the result has one value per ENTRY, so a wave finishes every group that begins and
// ends inside its range in place: the normalised values overwrite the staged ones and the range leaves LDS with 16-byte stores.
// One read and one write per entry (forward), two reads and one write (backward), plus the wave's window of `ptr`.
//
// Forward (SmFwdOp): the (max, Σ exp) partial of log-sum-exp; the merge leaves (m, Σ) — (m, log Σ) in the log form — in the tail
// slot of the range that owns a crossing group, and the fix-up normalises the entries of its pieces from there.
// Backward (SmBwdOp): a plain segmented sum S = Σ g·y (log form: Σ g) over the group, gin = a − b·S with (a, b) = (g·y, y) or
// (g, exp y); a and b are staged, a is what the walk reduces and rewrites.
//
// Merge and fix-up are separate launches that the host omits when no group crosses a range boundary (the caller knows that from
// the pattern; the workspace is then null and the walk writes no partial): nothing in a kernel waits for another workgroup, and
// nothing is accumulated with atomics — the same inputs give the same bits.
#pragma once

#include "logsumexp_impl.h"

namespace tsgu {

template <typename V>
struct SmFwd {
    const void* ptr;     // [n_groups + 1]
    const void* perm;    // [nnz] or null: entry k is val[perm[k]] and goes to out[perm[k]]
    const V* val;
    V* out;
    void* part;          // Acc[n_ranges][kSegSlots], or null: no group crosses a range boundary
    int64_t* tail;       // [n_ranges]: the owned group that runs past the range, or -1
    int64_t n_groups, nnz, n_ranges;
    int log_form;
    int vec_ok;          // val and out are 16-byte aligned (ranges start at multiples of the range length)
};

template <typename V>
struct SmBwd {
    const void* ptr;
    const void* perm;
    const V* y;          // the forward's result
    const V* g;          // upstream gradient of y
    V* gin;
    void* part;          // Acc[n_ranges][kSegSlots] (word 0: head sum, kSegTail: tail sum, then the group's sum), or null
    int64_t* tail;
    int64_t n_groups, nnz, n_ranges;
    int log_form;
    int vec_ok;          // y, g and gin are 16-byte aligned
};

// One entry from its group's (m, t): t = Σ exp(v − m), or its logarithm in the log form.  A group whose maximum is not finite
// (a NaN, a +inf, or nothing but −inf) is NaN throughout, as torch.softmax gives on the group's values.
template <typename Acc>
__device__ __forceinline__ Acc sm_value(Acc v, Acc m, Acc t, int log_form) {
    if (!finite_acc(m)) return (Acc)NAN;
    return log_form ? (v - m) - t : acc_exp(v - m) / t;
}
template <typename Acc>
__device__ __forceinline__ Acc sm_scale(Acc sum, int log_form) { return log_form ? acc_log(sum) : sum; }
// ... and of the gradient, from (a, b) and the group's S
template <typename Acc>
__device__ __forceinline__ Acc sm_grad(Acc a, Acc b, Acc S) { return a - b * S; }

// The staged range back to dst (through perm when given), rounded once: seg_stage's way back.
template <typename V, typename I>
__device__ __forceinline__ void sm_unstage(const typename VT<V>::Acc* st, V* __restrict__ dst, const I* __restrict__ perm, int64_t s,
                                           int len, bool vec, int lane) {
    using Acc = typename VT<V>::Acc;
    constexpr int W = VT<V>::kWide;
    if (perm == nullptr && vec) {
        for (int i = lane * W; i < len; i += kWave * W) {
            if (i + W <= len) {
                Acc v[W];
#pragma unroll
                for (int j = 0; j < W; ++j) v[j] = st[i + j];
                store_vec<V, W>(dst + s + i, v);
            } else {
                for (int j = i; j < len; ++j) dst[s + j] = VT<V>::down(st[j]);
            }
        }
    } else if (perm == nullptr) {
        for (int i = lane; i < len; i += kWave) dst[s + i] = VT<V>::down(st[i]);
    } else {
        for (int i = lane; i < len; i += kWave) dst[(int64_t)perm[s + i]] = VT<V>::down(st[i]);
    }
}

// The staged values other lanes of the wave rewrote are read next: LDS serves a wave's accesses in order, the fence keeps the
// compiler from moving them.
__device__ __forceinline__ void sm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Forward: a finished group's staged values become their normalised values, by the lanes that reduced them.
template <typename V>
struct SmFwdOp : MaxSumExp<typename VT<V>::Acc> {
    using Acc = typename VT<V>::Acc;
    using Part = typename MaxSumExp<Acc>::Part;
    using Params = SmFwd<V>;
    const int lf;   // (a copy of log_form: the per-entry loops must not read it through the parameter block)
    __device__ __forceinline__ explicit SmFwdOp(const Params& P) : lf(P.log_form) {}
    __device__ __forceinline__ void lane_finish(Acc* st, int lo, int hi, int64_t, int64_t, Part p) const {
        const Acc t = sm_scale(p.s, lf);
        if (lf) {   // (the form is chosen once per group, not per entry)
            for (int i = lo; i < hi; ++i) st[i] = sm_value(st[i], p.m, t, 1);
        } else {
            for (int i = lo; i < hi; ++i) st[i] = sm_value(st[i], p.m, t, 0);
        }
    }
    __device__ __forceinline__ void wave_finish(Acc* st, int lo, int hi, int64_t, int64_t, Part p, int lane) const {
        const Acc t = sm_scale(p.s, lf);
        if (lf) {
            for (int i = lo + lane; i < hi; i += kWave) st[i] = sm_value(st[i], p.m, t, 1);
        } else {
            for (int i = lo + lane; i < hi; i += kWave) st[i] = sm_value(st[i], p.m, t, 0);
        }
    }
    static __device__ __forceinline__ void merged_finish(const Params& P, Acc* slot, int64_t, int64_t, Part p) {
        slot[0] = p.m;
        slot[1] = sm_scale(p.s, P.log_form);
    }
    static __device__ __forceinline__ Part merged(const Acc* slot) { return {slot[0], slot[1]}; }
    static __device__ __forceinline__ void fix(const Params& P, int64_t at, Part t) {
        P.out[at] = VT<V>::down(sm_value(VT<V>::up(P.val[at]), t.m, t.s, P.log_form));
    }
};

// Backward: the partial is the plain sum of the staged a; b is staged beside it (the fix-up reads both from global memory).
template <typename V>
struct SmBwdOp {
    using Acc = typename VT<V>::Acc;
    using Part = Acc;
    using Params = SmBwd<V>;
    const Acc* sb;   // the staged b of the wave's range
    __device__ __forceinline__ explicit SmBwdOp(const Acc* b) : sb(b) {}
    static __device__ __forceinline__ Part identity() { return Acc(0); }
    static __device__ __forceinline__ void combine(Part& a, Part b) { a += b; }
    static __device__ __forceinline__ Part wave_combine(Part p) { return group_sum<Acc, kWave>(p); }
    static __device__ __forceinline__ void put(Acc* slot, Part p) { slot[0] = p; }
    static __device__ __forceinline__ Part get(const Acc* slot) { return slot[0]; }
    static __device__ __forceinline__ Part lane_reduce(const Acc* sa, int lo, int hi) {
        Acc sum = Acc(0);
        for (int i = lo; i < hi; ++i) sum += sa[i];
        return sum;
    }
    static __device__ __forceinline__ Part wave_reduce(const Acc* sa, int lo, int hi, int lane) {
        Acc sum = Acc(0);
        for (int i = lo + lane; i < hi; i += kWave) sum += sa[i];
        return group_sum<Acc, kWave>(sum);
    }
    __device__ __forceinline__ void lane_finish(Acc* sa, int lo, int hi, int64_t, int64_t, Part sum) const {
        for (int i = lo; i < hi; ++i) sa[i] = sm_grad(sa[i], sb[i], sum);
    }
    __device__ __forceinline__ void wave_finish(Acc* sa, int lo, int hi, int64_t, int64_t, Part sum, int lane) const {
        for (int i = lo + lane; i < hi; i += kWave) sa[i] = sm_grad(sa[i], sb[i], sum);
    }
    static __device__ __forceinline__ void merged_finish(const Params&, Acc* slot, int64_t, int64_t, Part sum) { slot[1] = sum; }
    static __device__ __forceinline__ Part merged(const Acc* slot) { return slot[1]; }
    static __device__ __forceinline__ void fix(const Params& P, int64_t at, Part sum) {
        const Acc y = VT<V>::up(P.y[at]), g = VT<V>::up(P.g[at]);
        P.gin[at] = VT<V>::down(P.log_form ? sm_grad(g, acc_exp(y), sum) : sm_grad(g * y, y, sum));
    }
};

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_fwd_kernel(SmFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    __shared__ Acc stage[kLseWavesPerBlock][R];
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    if (w >= P.n_ranges) return;   // (no workgroup barrier below: a wave only reads what it staged itself)
    Acc* st = stage[wid];
    const int64_t s = w * R;
    const int len = seg_len<Acc>(w, P.nnz);
    const bool vec = P.vec_ok != 0;
    seg_stage<V, I>(st, P.val, perm, s, len, vec, lane, [](Acc v, int) { return v; });
    sm_wave_sync();
    seg_walk(st, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, P.part ? static_cast<Acc*>(P.part) + w * kSegSlots : nullptr, P.tail,
             SmFwdOp<V>(P));
    sm_wave_sync();
    // (the pieces of crossing groups leave as they came; seg_fix_kernel overwrites them)
    sm_unstage<V, I>(st, P.out, perm, s, len, vec, lane);
}

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_bwd_kernel(SmBwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    __shared__ Acc stage_a[kLseWavesPerBlock][R];   // g·y (log form: g), then gin
    __shared__ Acc stage_b[kLseWavesPerBlock][R];   // y (log form: exp y)
    const int lane = threadIdx.x % kWave, wid = threadIdx.x / kWave;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + wid;
    if (w >= P.n_ranges) return;
    Acc* sa = stage_a[wid];
    Acc* sb = stage_b[wid];
    const int64_t s = w * R;
    const int len = seg_len<Acc>(w, P.nnz);
    const int lf = P.log_form;
    const bool vec = P.vec_ok != 0;
    seg_stage<V, I>(sb, P.y, perm, s, len, vec, lane, [&](Acc v, int) { return lf ? acc_exp(v) : v; });
    // (each lane multiplies by the y it staged itself: the two passes walk the same indices)
    seg_stage<V, I>(sa, P.g, perm, s, len, vec, lane, [&](Acc v, int i) { return lf ? v : v * sb[i]; });
    sm_wave_sync();
    seg_walk(sa, ptr, P.n_groups, P.nnz, P.n_ranges, w, lane, P.part ? static_cast<Acc*>(P.part) + w * kSegSlots : nullptr, P.tail,
             SmBwdOp<V>(sb));
    sm_wave_sync();
    sm_unstage<V, I>(sa, P.gin, perm, s, len, vec, lane);
}

}  // namespace tsgu
