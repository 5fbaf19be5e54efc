// Segmented log-sum-exp over a row-gather pattern and its gradient (sparse_logsumexp / sparse_bidir_logsumexp).
//
// Forward.  The entries are cut into contiguous ranges of kLseRange entries, one wave each (balanced by entries, not by
// groups: one group of 2^20 entries among short ones occupies 2^20 / kLseRange waves).  A wave loads its range with 16-byte
// loads (or through `perm`, for the column direction) into LDS, then reduces every group it owns — the groups whose first
// entry lies in the range — lane per group for short ones and the whole wave for long ones.  A group that runs past the range
// leaves a (max, sum) partial in the wave's tail slot, and every later wave it reaches leaves one in its head slot; a second
// kernel merges those partials in a fixed order.  No float atomics: the same inputs give the same bits, and a direction
// computed alone or as half of the bidirectional call is the same kernel with the same operands.
//
// Backward.  One streaming pass in the stored order: each entry finds its primary group from `ptr` (a search in the wave's
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

template <typename V>
struct LseFwd {
    const void* ptr;     // [n_groups + 1]
    const void* perm;    // [nnz] or null: entry k is val[perm[k]]
    const V* val;
    V* out;
    void* part;          // Acc[n_ranges][4]: head (m, s), tail (m, s)
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

template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) lse_fwd_kernel(LseFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    constexpr int W = VT<V>::kWide;
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
    const int64_t s = w * R;
    const int64_t e = !live ? s : s + R < P.nnz ? s + R : P.nnz;
    const int len = (int)(e - s);
    const bool last = w == P.n_ranges - 1;
    Acc* st = stage[wid];

    // stage the range
    if (perm == nullptr && P.vec_ok) {
        const V* src = P.val + s;
        for (int i = lane * W; i < len; i += kWave * W) {
            if (i + W <= len) {
                Acc v[W];
                load_vec<V, W>(src + i, v);
#pragma unroll
                for (int j = 0; j < W; ++j) st[i + j] = v[j];
            } else {
                for (int j = i; j < len; ++j) st[j] = VT<V>::up(src[j]);
            }
        }
    } else if (perm == nullptr) {
        for (int i = lane; i < len; i += kWave) st[i] = VT<V>::up(P.val[s + i]);
    } else {
        for (int i = lane; i < len; i += kWave) st[i] = VT<V>::up(P.val[(int64_t)perm[s + i]]);
    }

    __syncthreads();
    if (!live) return;
    // owned groups [ga, gb): first entry in [s, e) (the last range also owns the empty groups at the end)
    const int64_t ga = wave_lower_bound(ptr, P.n_groups, s, lane);
    const int64_t gb = last ? P.n_groups : wave_lower_bound(ptr, P.n_groups, e, lane);

    Acc* part = static_cast<Acc*>(P.part) + w * 4;
    const Acc ninf = -(Acc)INFINITY;

    // the whole wave over st[lo, hi): (m, s) in every lane
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

    // head: the group entry s belongs to started in an earlier range
    if (s < P.nnz && (ga == P.n_groups || (int64_t)ptr[ga] > s)) {
        const int64_t hend = (int64_t)ptr[ga];
        Acc m, sum;
        wave_reduce(0, (int)((hend < e ? hend : e) - s), m, sum);
        if (lane == 0) {
            part[0] = m;
            part[1] = sum;
        }
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
            Acc m = ninf;
            for (int i = lo; i < hi; ++i) m = nanmax(m, st[i]);
            Acc sum = Acc(0);
            if (finite_acc(m)) {
                for (int i = lo; i < hi; ++i) sum += acc_exp(st[i] - m);
            }
            if (ghi <= e) {
                lse_store(P, g, lse_finish(m, sum, lse_zeros(P, ghi - glo)));
            } else {
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
            const int64_t fglo = __shfl(glo, f, kWave), fghi = __shfl(ghi, f, kWave);
            Acc m, sum;
            wave_reduce(flo, fhi, m, sum);
            if (lane == 0) {
                if (fghi <= e) {
                    lse_store(P, base + f, lse_finish(m, sum, lse_zeros(P, fghi - fglo)));
                } else {
                    part[2] = m;
                    part[3] = sum;
                }
            }
            if (fghi > e) tailg = base + f;
        }
    }
    if (lane == 0) P.tail[w] = tailg;
}

// One wave per range: the range's tail group (if any) merges its partials — the range's tail slot, then the head slots of the
// later ranges it reaches — lane-strided and then by a fixed butterfly; lane 0 writes the group.
template <typename V, typename I>
__global__ void __launch_bounds__(kBlock) lse_merge_kernel(LseFwd<V> P) {
    using Acc = typename VT<V>::Acc;
    constexpr int R = lse_range<Acc>();
    const int lane = threadIdx.x % kWave;
    const int64_t w = (int64_t)blockIdx.x * kLseWavesPerBlock + threadIdx.x / kWave;
    if (w >= P.n_ranges) return;
    const int64_t g = P.tail[w];
    if (g < 0) return;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const int64_t glo = (int64_t)ptr[g], ghi = (int64_t)ptr[g + 1];
    const int64_t w1 = (ghi - 1) / R;
    const Acc* part = static_cast<const Acc*>(P.part);
    Acc m = -(Acc)INFINITY, sum = Acc(0);
    for (int64_t j = lane; j <= w1 - w; j += kWave) {
        const Acc* q = j == 0 ? part + w * 4 + 2 : part + (w + j) * 4;
        lse_combine(m, sum, q[0], q[1]);
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const Acc m2 = shfl_xor_acc(m, o), s2 = shfl_xor_acc(sum, o);
        lse_combine(m, sum, m2, s2);
    }
    if (lane == 0) lse_store(P, g, lse_finish(m, sum, lse_zeros(P, ghi - glo)));
}

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

}  // namespace tsgu
