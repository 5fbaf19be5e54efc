// Segmented softmax / log-softmax over a row-gather pattern and its gradient (sparse_softmax / sparse_log_softmax).
//
// The cutting is the log-sum-exp forward's (logsumexp_impl.h): contiguous ranges of lse_range<Acc>() entries, one wave each, staged
// in LDS as accumulator values; a group of up to kLseLaneMax entries in the range is reduced by one lane, a longer one by the
// whole wave.  Unlike a reduction, the result has one value per ENTRY, so a wave finishes every group that begins and ends
// inside its range in place: the normalised values overwrite the staged ones and the range leaves LDS with 16-byte stores.  One
// read and one write per entry (forward), two reads and one write (backward), plus the wave's window of `ptr`.
//
// A group that crosses a range boundary leaves the (max, sum) partial of its first piece in the range's tail slot and of every
// later piece in that range's head slot; sm_merge_kernel combines them in a fixed order into the tail slot of the range that
// owns the group, and sm_fix_kernel normalises the entries of those pieces only (read once more from global memory).  Both are
// separate launches that the host omits when no group crosses (the caller knows that from the pattern): nothing in a kernel
// waits for another workgroup, and nothing is accumulated with atomics — the same inputs give the same bits.
//
// The backward has the same shape with a plain segmented sum: S = Σ g·y (log form: Σ g) over the group, gin = a − b·S with
// (a, b) = (g·y, y) or (g, exp y).
#pragma once

#include "logsumexp_impl.h"

namespace tsgu {

constexpr int kSmSlots = 4;   // workspace words of one range: head (m, s), tail (m, s) — the log-sum-exp forward's layout

template <typename V>
struct SmFwd {
    const void* ptr;     // [n_groups + 1]
    const void* perm;    // [nnz] or null: entry k is val[perm[k]] and goes to out[perm[k]]
    const V* val;
    V* out;
    void* part;          // Acc[n_ranges][kSmSlots], or null: no group crosses a range boundary
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
    void* part;          // Acc[n_ranges][kSmSlots] (slot 0: head sum, slot 2: tail sum, then the group's sum), or null
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

// The wave's range [s, e) of `src` (through perm when given) into LDS as accumulator values, f applied to each.
template <typename V, typename I, typename F>
__device__ __forceinline__ void sm_stage(typename VT<V>::Acc* st, const V* __restrict__ src, const I* __restrict__ perm, int64_t s,
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

// ... and back: the staged range to dst (through perm when given), rounded once.
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

// The wave's range and the groups it owns — the log-sum-exp forward's rule: [ga, gb) are the groups whose first entry lies in
// [s, e) (the last range also owns the empty groups at the end); `head`: entry s belongs to a group that started earlier.
template <typename I>
struct SmRange {
    int64_t s, e, ga, gb;
    bool head;
    __device__ __forceinline__ SmRange(const I* __restrict__ ptr, int64_t n_groups, int64_t nnz, int64_t n_ranges, int64_t w, int R,
                                       int lane) {
        s = w * R;
        e = s + R < nnz ? s + R : nnz;
        ga = wave_lower_bound(ptr, n_groups, s, lane);
        gb = w == n_ranges - 1 ? n_groups : wave_lower_bound(ptr, n_groups, e, lane);
        head = s < nnz && (ga == n_groups || (int64_t)ptr[ga] > s);
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
    const int64_t s0 = w * R;
    const int len = (int)((s0 + R < P.nnz ? s0 + R : P.nnz) - s0);
    sm_stage<V, I>(st, P.val, perm, s0, len, P.vec_ok != 0, lane, [](Acc v, int) { return v; });
    sm_wave_sync();

    const SmRange<I> rg(ptr, P.n_groups, P.nnz, P.n_ranges, w, R, lane);
    const int64_t s = rg.s, e = rg.e;
    Acc* part = P.part ? static_cast<Acc*>(P.part) + w * kSmSlots : nullptr;
    const Acc ninf = -(Acc)INFINITY;
    const int lf = P.log_form;

    // the whole wave over st[lo, hi): (m, sum) in every lane
    auto wave_reduce = [&](int lo, int hi, Acc& m, Acc& sum) {
        m = ninf;
        for (int i = lo + lane; i < hi; i += kWave) m = nanmax(m, st[i]);
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) m = nanmax(m, shfl_xor_acc(m, o));
        sum = Acc(0);
        if (finite_acc(m)) {
            for (int i = lo + lane; i < hi; i += kWave) sum += acc_exp(st[i] - m);
        }
        sum = group_sum<Acc, kWave>(sum);
    };

    if (rg.head && part) {
        const int64_t hend = (int64_t)ptr[rg.ga];
        Acc m, sum;
        wave_reduce(0, (int)((hend < e ? hend : e) - s), m, sum);
        if (lane == 0) {
            part[0] = m;
            part[1] = sum;
        }
    }
    int64_t tailg = -1;   // (wave-uniform)

    for (int64_t base = rg.ga; base < rg.gb; base += kWave) {
        const int64_t g = base + lane;
        const bool active = g < rg.gb;
        const int64_t glo = active ? (int64_t)ptr[g] : s;
        const int64_t ghi = active ? (int64_t)ptr[g + 1] : s;
        const int lo = (int)(glo - s), hi = (int)((ghi < e ? ghi : e) - s);
        const bool wide = active && hi - lo > kLseLaneMax;
        if (active && !wide) {
            Acc m = ninf;
            for (int i = lo; i < hi; ++i) m = nanmax(m, st[i]);
            Acc sum = Acc(0);
            if (finite_acc(m)) {
                for (int i = lo; i < hi; ++i) sum += acc_exp(st[i] - m);
            }
            if (ghi <= e) {
                const Acc t = sm_scale(sum, lf);
                for (int i = lo; i < hi; ++i) st[i] = sm_value(st[i], m, t, lf);
            } else if (part) {
                part[2] = m;
                part[3] = sum;
            }
        }
        const unsigned long long tmask = __ballot(active && !wide && ghi > e);
        if (tmask) tailg = base + __builtin_ctzll(tmask);
        unsigned long long mask = __ballot(wide);
        while (mask) {
            const int f = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int flo = __shfl(lo, f, kWave), fhi = __shfl(hi, f, kWave);
            const int64_t fghi = __shfl(ghi, f, kWave);
            Acc m, sum;
            wave_reduce(flo, fhi, m, sum);
            if (fghi <= e) {
                const Acc t = sm_scale(sum, lf);
                for (int i = flo + lane; i < fhi; i += kWave) st[i] = sm_value(st[i], m, t, lf);
            } else {
                if (lane == 0 && part) {
                    part[2] = m;
                    part[3] = sum;
                }
                tailg = base + f;
            }
        }
    }
    if (lane == 0 && part) P.tail[w] = tailg;
    sm_wave_sync();
    // (the pieces of crossing groups leave as they came; sm_fix_kernel overwrites them)
    sm_unstage<V, I>(st, P.out, perm, s, len, P.vec_ok != 0, lane);
}

// One wave per range: the range's tail group (if any) merges its partials — the range's tail slot, then the head slots of the
// later ranges it reaches — lane-strided and then by a fixed butterfly; lane 0 leaves (m, Σ or log Σ) in the tail slot.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_merge_kernel(SmFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const int64_t g = P.tail[w];
    if (g < 0) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const int64_t w1 = ((int64_t)ptr[g + 1] - 1) / R;
    Acc* part = static_cast<Acc*>(P.part);
    Acc m = -(Acc)INFINITY, sum = Acc(0);
    for (int64_t j = lane; j <= w1 - w; j += kWave) {
        const Acc* q = j == 0 ? part + w * kSmSlots + 2 : part + (w + j) * kSmSlots;
        lse_combine(m, sum, q[0], q[1]);
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const Acc m2 = shfl_xor_acc(m, o), s2 = shfl_xor_acc(sum, o);
        lse_combine(m, sum, m2, s2);
    }
    if (lane == 0) {   // (the only reader of this slot above is lane 0 itself)
        part[w * kSmSlots + 2] = m;
        part[w * kSmSlots + 3] = sm_scale(sum, P.log_form);
    }
}

// One wave per range: the entries of its head piece (from the tail slot of the range that owns that group) and of its tail piece.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_fix_kernel(SmFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const Acc* part = static_cast<const Acc*>(P.part);
    const int64_t s = w * R, e = s + R < P.nnz ? s + R : P.nnz;
    const int lf = P.log_form;
    auto piece = [&](int64_t lo, int64_t hi, int64_t owner) {
        const Acc m = part[owner * kSmSlots + 2], t = part[owner * kSmSlots + 3];
        for (int64_t k = lo + lane; k < hi; k += kWave) {
            const int64_t at = perm ? (int64_t)perm[k] : k;
            P.out[at] = VT<V>::down(sm_value(VT<V>::up(P.val[at]), m, t, lf));
        }
    };
    const int64_t tg = P.tail[w];
    if (w > 0) {   // (range 0 has no head; the search is skipped where the range starts on a group start)
        const int64_t ga = wave_lower_bound(ptr, P.n_groups, s, lane);
        if (s < P.nnz && (ga == P.n_groups || (int64_t)ptr[ga] > s)) {
            const int64_t hend = (int64_t)ptr[ga];
            piece(s, hend < e ? hend : e, (int64_t)ptr[ga - 1] / R);
        }
    }
    if (tg >= 0) piece((int64_t)ptr[tg], e, w);
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
    const int64_t s0 = w * R;
    const int len = (int)((s0 + R < P.nnz ? s0 + R : P.nnz) - s0);
    const int lf = P.log_form;
    const bool vec = P.vec_ok != 0;
    sm_stage<V, I>(sb, P.y, perm, s0, len, vec, lane, [&](Acc v, int) { return lf ? acc_exp(v) : v; });
    // (each lane multiplies by the y it staged itself: the two passes walk the same indices)
    sm_stage<V, I>(sa, P.g, perm, s0, len, vec, lane, [&](Acc v, int i) { return lf ? v : v * sb[i]; });
    sm_wave_sync();

    const SmRange<I> rg(ptr, P.n_groups, P.nnz, P.n_ranges, w, R, lane);
    const int64_t s = rg.s, e = rg.e;
    Acc* part = P.part ? static_cast<Acc*>(P.part) + w * kSmSlots : nullptr;

    auto wave_sum = [&](int lo, int hi) {
        Acc sum = Acc(0);
        for (int i = lo + lane; i < hi; i += kWave) sum += sa[i];
        return group_sum<Acc, kWave>(sum);
    };

    if (rg.head && part) {
        const int64_t hend = (int64_t)ptr[rg.ga];
        const Acc sum = wave_sum(0, (int)((hend < e ? hend : e) - s));
        if (lane == 0) part[0] = sum;
    }
    int64_t tailg = -1;

    for (int64_t base = rg.ga; base < rg.gb; base += kWave) {
        const int64_t g = base + lane;
        const bool active = g < rg.gb;
        const int64_t glo = active ? (int64_t)ptr[g] : s;
        const int64_t ghi = active ? (int64_t)ptr[g + 1] : s;
        const int lo = (int)(glo - s), hi = (int)((ghi < e ? ghi : e) - s);
        const bool wide = active && hi - lo > kLseLaneMax;
        if (active && !wide) {
            Acc sum = Acc(0);
            for (int i = lo; i < hi; ++i) sum += sa[i];
            if (ghi <= e) {
                for (int i = lo; i < hi; ++i) sa[i] = sa[i] - sb[i] * sum;
            } else if (part) {
                part[2] = sum;
            }
        }
        const unsigned long long tmask = __ballot(active && !wide && ghi > e);
        if (tmask) tailg = base + __builtin_ctzll(tmask);
        unsigned long long mask = __ballot(wide);
        while (mask) {
            const int f = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int flo = __shfl(lo, f, kWave), fhi = __shfl(hi, f, kWave);
            const int64_t fghi = __shfl(ghi, f, kWave);
            const Acc sum = wave_sum(flo, fhi);
            if (fghi <= e) {
                for (int i = flo + lane; i < fhi; i += kWave) sa[i] = sa[i] - sb[i] * sum;
            } else {
                if (lane == 0 && part) part[2] = sum;
                tailg = base + f;
            }
        }
    }
    if (lane == 0 && part) P.tail[w] = tailg;
    sm_wave_sync();
    sm_unstage<V, I>(sa, P.gin, perm, s, len, vec, lane);
}

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_bwd_merge_kernel(SmBwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const int64_t g = P.tail[w];
    if (g < 0) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const int64_t w1 = ((int64_t)ptr[g + 1] - 1) / R;
    Acc* part = static_cast<Acc*>(P.part);
    Acc sum = Acc(0);
    for (int64_t j = lane; j <= w1 - w; j += kWave) sum += j == 0 ? part[w * kSmSlots + 2] : part[(w + j) * kSmSlots];
    sum = group_sum<Acc, kWave>(sum);
    if (lane == 0) part[w * kSmSlots + 3] = sum;
}

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) sm_bwd_fix_kernel(SmBwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ perm = static_cast<const I*>(P.perm);
    const Acc* part = static_cast<const Acc*>(P.part);
    const int64_t s = w * R, e = s + R < P.nnz ? s + R : P.nnz;
    const int lf = P.log_form;
    auto piece = [&](int64_t lo, int64_t hi, int64_t owner) {
        const Acc sum = part[owner * kSmSlots + 3];
        for (int64_t k = lo + lane; k < hi; k += kWave) {
            const int64_t at = perm ? (int64_t)perm[k] : k;
            const Acc y = VT<V>::up(P.y[at]), g = VT<V>::up(P.g[at]);
            const Acc a = lf ? g : g * y, b = lf ? acc_exp(y) : y;
            P.gin[at] = VT<V>::down(a - b * sum);
        }
    };
    const int64_t tg = P.tail[w];
    if (w > 0) {
        const int64_t ga = wave_lower_bound(ptr, P.n_groups, s, lane);
        if (s < P.nnz && (ga == P.n_groups || (int64_t)ptr[ga] > s)) {
            const int64_t hend = (int64_t)ptr[ga];
            piece(s, hend < e ? hend : e, (int64_t)ptr[ga - 1] / R);
        }
    }
    if (tg >= 0) piece((int64_t)ptr[tg], e, w);
}

}  // namespace tsgu
