// Sparse × sparse products C = A·B over CSR arrays, in two phases.
//
// Symbolic (once per pair of patterns): a group of lanes owns a row of C.  It copies the column indices of every B row that the
// row of A meets into a buffer of at least ub = Σ_k nnz(B[k,:]) slots, pads the buffer with a sentinel, sorts it with a bitonic
// network and keeps the first of every run of equal columns: exact, ascending, and without a probe loop — the buffer is sized
// by the row's upper bound, every loop runs over the buffer.  The launch either counts (cnt[row]) or, with C's row pointer
// known, writes the columns.  Rows are binned by ub: 8 lanes and 32 slots, a wave and 512 slots, a workgroup and 4096 slots, all
// in LDS; longer rows sort a power-of-two slice of a global scratch array with one workgroup each (the same code on another
// pointer).  No workgroup reads what another wrote.
//
// Numeric (every call): the same groups, binned by the row's length in C.  The row's sorted columns and its accumulators sit in
// LDS (the last bin: the columns are C's own, the accumulators a global array).  The entries of A[i,:] are taken one after the
// other in stored order; for each, the lanes run over the entries of B[k,:] — distinct columns, so distinct slots — find the
// column by bisection and add a·b to its slot.  Every output entry is therefore summed in A's stored order by plain adds: no
// float atomics, the same bits on every run.  bf16 accumulates in fp32 and is rounded once.
//
// The two gradients are gathers over C's pattern (one thread per stored entry of the operand, bisection in C's row):
//   gradA[i,k] = Σ_{t ∈ B[k,:]} g[pos_C(i, col_t)]·b_t          in B's stored order
//   gradB[k,j] = Σ_{i ∈ column k of A} a_ik·g[pos_C(i, j)]       in the order of A's transposed pattern
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kSpgemmBins = 4;                        // three LDS bins and the global one
constexpr int kSpgemmLimit[3] = {32, 512, 4096};      // largest ub (symbolic) / row length of C (numeric) of the LDS bins
constexpr int kSpgemmGroup[kSpgemmBins] = {8, 64, 256, 256};
constexpr int kSpgemmEmpty = 0x7fffffff;              // above every column index: n_cols < 2^31

struct SpgemmParams {
    int64_t n_bin;             // rows of this launch
    const int* rows;           // their indices
    int64_t n_rows, n_inner, n_cols;
    const void *a_ptr, *a_idx, *a_val;
    const void *b_ptr, *b_idx, *b_val;
    void *c_ptr, *c_idx, *c_val;
    int* scratch;              // symbolic, global bin: the sort buffers, row g of the launch at sptr[g] .. sptr[g + 1] (a power of two)
    const int64_t* sptr;
    int64_t* cnt;              // symbolic, counting launch: distinct columns of every row
    int fill;                  // symbolic: 0 = count, 1 = write c_idx
    void* acc;                 // numeric, global bin: nnz(C) accumulators
};

struct SpgemmGradParams {
    int64_t n_entries;         // stored entries of the operand whose gradient is computed
    int64_t n_rows, n_inner, n_cols;
    const void* row;           // row index of every such entry
    const void* idx;           // its column index
    const void *w_ptr, *w_idx, *w_perm, *w_val;      // the walked side: B's rows (gradA), A's transposed pattern and values (gradB)
    const void *c_ptr, *c_idx;
    const void* g;             // upstream gradient on C's pattern
    void* out;
};

// Lanes of one group meet: a workgroup barrier when the group is the workgroup, else the lanes share a wave, whose LDS accesses
// execute in program order — only the compiler has to be kept from moving them.
template <int GROUP>
__device__ __forceinline__ void spgemm_group_sync() {
    if constexpr (GROUP == kBlock) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
}

// First position of `len` ascending columns that is not below j.
template <typename C>
__device__ __forceinline__ int spgemm_lower_bound(const C* cols, int len, int64_t j) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)cols[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename I, int GROUP, int CAP, bool GLOBAL>
__global__ __launch_bounds__(kBlock) void spgemm_symbolic_kernel(SpgemmParams P) {
    constexpr int GPB = kBlock / GROUP;
    __shared__ int lds_buf[GLOBAL ? 1 : GPB * CAP];
    __shared__ int scan[kBlock];
    const int lane = threadIdx.x % GROUP, slot = threadIdx.x / GROUP;
    const int64_t g = (int64_t)blockIdx.x * GPB + slot;
    if (g >= P.n_bin) return;      // (a whole group, and with GROUP = kBlock the whole workgroup)
    const int64_t row = P.rows[g];
    int* buf;
    int cap;
    if constexpr (GLOBAL) {
        buf = P.scratch + P.sptr[g];
        cap = (int)(P.sptr[g + 1] - P.sptr[g]);
    } else {
        buf = lds_buf + slot * CAP;
        cap = CAP;
    }
    const I* ap = static_cast<const I*>(P.a_ptr);
    const I* ai = static_cast<const I*>(P.a_idx);
    const I* bp = static_cast<const I*>(P.b_ptr);
    const I* bi = static_cast<const I*>(P.b_idx);

    const int64_t a0 = ap[row], a1 = ap[row + 1];
    int64_t off = 0;
    for (int64_t e = a0; e < a1; ++e) {
        const int64_t k = ai[e];
        if ((uint64_t)k >= (uint64_t)P.n_inner) continue;
        const int64_t b0 = bp[k], len = bp[k + 1] - b0;
        if (len <= 0) continue;
        for (int64_t t = lane; t < len; t += GROUP)
            if (off + t < cap) buf[off + t] = (int)bi[b0 + t];
        off += len;
    }
    if constexpr (!GLOBAL) {      // sort no more than the row needs: the power of two at or above its candidates (and the group's lanes)
        int need = GROUP;
        while (need < off && need < cap) need <<= 1;
        cap = need;
    }
    for (int64_t t = (off < cap ? off : cap) + lane; t < cap; t += GROUP) buf[t] = kSpgemmEmpty;
    spgemm_group_sync<GROUP>();

    for (int k = 2; k <= cap; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < cap; i += GROUP) {
                const int o = i ^ j;
                if (o > i) {
                    const int x = buf[i], y = buf[o];
                    if ((x > y) == ((i & k) == 0)) buf[i] = y, buf[o] = x;
                }
            }
            spgemm_group_sync<GROUP>();
        }
    }

    // the first of every run of equal columns, each lane over its own contiguous piece
    const int piece = cap / GROUP, lo = lane * piece;
    int mine = 0;
    for (int i = lo; i < lo + piece; ++i) {
        const int v = buf[i];
        mine += (v != kSpgemmEmpty && (i == 0 || buf[i - 1] != v)) ? 1 : 0;
    }
    scan[threadIdx.x] = mine;
    spgemm_group_sync<GROUP>();
    int before = 0, total = 0;
    for (int l = 0; l < GROUP; ++l) {
        const int s = scan[slot * GROUP + l];
        total += s;
        before += l < lane ? s : 0;
    }
    if (!P.fill) {
        if (lane == 0) P.cnt[row] = total;
        return;
    }
    const I* cp = static_cast<const I*>(P.c_ptr);
    I* ci = static_cast<I*>(P.c_idx);
    const int64_t c0 = cp[row], clen = cp[row + 1] - c0;
    int64_t w = before;
    for (int i = lo; i < lo + piece; ++i) {
        const int v = buf[i];
        if (v != kSpgemmEmpty && (i == 0 || buf[i - 1] != v)) {
            if (w < clen) ci[c0 + w] = (I)v;
            ++w;
        }
    }
}

// ub[i] = Σ_{k ∈ A[i,:]} nnz(B[k,:]): one thread per row.
template <typename I>
__global__ __launch_bounds__(kBlock) void spgemm_row_bound_kernel(int64_t n_rows, int64_t n_inner, const I* __restrict__ ap,
                                                                  const I* __restrict__ ai, const I* __restrict__ bp,
                                                                  int64_t* __restrict__ ub) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    int64_t s = 0;
    for (int64_t e = ap[row]; e < ap[row + 1]; ++e) {
        const int64_t k = ai[e];
        if ((uint64_t)k >= (uint64_t)n_inner) continue;
        const int64_t len = bp[k + 1] - bp[k];
        s += len > 0 ? len : 0;
    }
    ub[row] = s;
}

template <typename V, typename I, int GROUP, int CAP, bool GLOBAL>
__global__ __launch_bounds__(kBlock) void spgemm_numeric_kernel(SpgemmParams P) {
    using Acc = typename VT<V>::Acc;
    using Col = typename std::conditional<GLOBAL, I, int>::type;
    constexpr int GPB = kBlock / GROUP;
    __shared__ int lds_col[GLOBAL ? 1 : GPB * CAP];
    __shared__ Acc lds_acc[GLOBAL ? 1 : GPB * CAP];
    __shared__ Acc st_a[kBlock];          // one pass of the row of A: value, first entry and length of the row of B it meets
    __shared__ int64_t st_b0[kBlock];
    __shared__ int st_len[kBlock];
    const int lane = threadIdx.x % GROUP, slot = threadIdx.x / GROUP;
    const int64_t g = (int64_t)blockIdx.x * GPB + slot;
    if (g >= P.n_bin) return;
    const int64_t row = P.rows[g];
    const I* ap = static_cast<const I*>(P.a_ptr);
    const I* ai = static_cast<const I*>(P.a_idx);
    const V* av = static_cast<const V*>(P.a_val);
    const I* bp = static_cast<const I*>(P.b_ptr);
    const I* bi = static_cast<const I*>(P.b_idx);
    const V* bv = static_cast<const V*>(P.b_val);
    const I* cp = static_cast<const I*>(P.c_ptr);
    const I* ci = static_cast<const I*>(P.c_idx);
    V* cv = static_cast<V*>(P.c_val);

    const int64_t c0 = cp[row];
    int64_t clen64 = cp[row + 1] - c0;
    const Col* cols;
    Acc* acc;
    if constexpr (GLOBAL) {
        cols = ci + c0;
        acc = static_cast<Acc*>(P.acc) + c0;
        if (clen64 > 0x7fffffffLL) clen64 = 0x7fffffffLL;
    } else {
        cols = lds_col + slot * CAP;
        acc = lds_acc + slot * CAP;
        if (clen64 > CAP) clen64 = CAP;      // (never: the row lists are binned by this length)
    }
    const int clen = clen64 > 0 ? (int)clen64 : 0;
    for (int i = lane; i < clen; i += GROUP) {
        if constexpr (!GLOBAL) lds_col[slot * CAP + i] = (int)ci[c0 + i];
        acc[i] = Acc(0);
    }
    spgemm_group_sync<GROUP>();

    const int64_t a0 = ap[row], a1 = ap[row + 1];
    for (int64_t base = a0; base < a1; base += GROUP) {
        const int64_t e = base + lane;
        Acc a = Acc(0);
        int64_t b0 = 0;
        int len = 0;
        if (e < a1) {
            const int64_t k = ai[e];
            if ((uint64_t)k < (uint64_t)P.n_inner) {
                a = VT<V>::up(av[e]);
                b0 = bp[k];
                const int64_t l = bp[k + 1] - b0;
                len = l > 0 ? (int)l : 0;
            }
        }
        st_a[threadIdx.x] = a, st_b0[threadIdx.x] = b0, st_len[threadIdx.x] = len;
        spgemm_group_sync<GROUP>();
        const int here = a1 - base < GROUP ? (int)(a1 - base) : GROUP;
        for (int q = 0; q < here; ++q) {      // A's stored order
            const Acc aq = st_a[slot * GROUP + q];
            const int64_t bq = st_b0[slot * GROUP + q];
            const int lq = st_len[slot * GROUP + q];
            for (int t = lane; t < lq; t += GROUP) {
                const int64_t j = bi[bq + t];
                const Acc b = VT<V>::up(bv[bq + t]);
                const int pos = spgemm_lower_bound(cols, clen, j);
                if (pos < clen && (int64_t)cols[pos] == j) acc[pos] += aq * b;
            }
            spgemm_group_sync<GROUP>();
        }
    }
    for (int i = lane; i < clen; i += GROUP) cv[c0 + i] = VT<V>::down(acc[i]);
}

// gradA: one thread per stored entry of A.
template <typename V, typename I>
__global__ __launch_bounds__(kBlock) void spgemm_grad_a_kernel(SpgemmGradParams P) {
    using Acc = typename VT<V>::Acc;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= P.n_entries) return;
    const int64_t i = static_cast<const I*>(P.row)[e], k = static_cast<const I*>(P.idx)[e];
    const I* bp = static_cast<const I*>(P.w_ptr);
    const I* bi = static_cast<const I*>(P.w_idx);
    const V* bv = static_cast<const V*>(P.w_val);
    const I* cp = static_cast<const I*>(P.c_ptr);
    const V* gv = static_cast<const V*>(P.g);
    Acc s = Acc(0);
    if ((uint64_t)i < (uint64_t)P.n_rows && (uint64_t)k < (uint64_t)P.n_inner) {
        const int64_t c0 = cp[i];
        const int64_t cl = cp[i + 1] - c0;
        const int clen = cl > 0 ? (int)(cl < 0x7fffffffLL ? cl : 0x7fffffffLL) : 0;
        const I* cols = static_cast<const I*>(P.c_idx) + c0;
        for (int64_t t = bp[k]; t < bp[k + 1]; ++t) {      // B's stored order
            const int64_t j = bi[t];
            const int pos = spgemm_lower_bound(cols, clen, j);
            if (pos < clen && (int64_t)cols[pos] == j) s += VT<V>::up(gv[c0 + pos]) * VT<V>::up(bv[t]);
        }
    }
    static_cast<V*>(P.out)[e] = VT<V>::down(s);
}

// gradB: one thread per stored entry (k, j) of B, over column k of A in the order of A's transposed pattern.
template <typename V, typename I>
__global__ __launch_bounds__(kBlock) void spgemm_grad_b_kernel(SpgemmGradParams P) {
    using Acc = typename VT<V>::Acc;
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= P.n_entries) return;
    const int64_t k = static_cast<const I*>(P.row)[e], j = static_cast<const I*>(P.idx)[e];
    const I* tp = static_cast<const I*>(P.w_ptr);
    const I* ti = static_cast<const I*>(P.w_idx);
    const I* tperm = static_cast<const I*>(P.w_perm);
    const V* av = static_cast<const V*>(P.w_val);
    const I* cp = static_cast<const I*>(P.c_ptr);
    const I* ci = static_cast<const I*>(P.c_idx);
    const V* gv = static_cast<const V*>(P.g);
    Acc s = Acc(0);
    if ((uint64_t)k < (uint64_t)P.n_inner) {
        for (int64_t u = tp[k]; u < tp[k + 1]; ++u) {
            const int64_t i = ti[u];
            if ((uint64_t)i >= (uint64_t)P.n_rows) continue;
            const int64_t c0 = cp[i];
            const int64_t cl = cp[i + 1] - c0;
            const int clen = cl > 0 ? (int)(cl < 0x7fffffffLL ? cl : 0x7fffffffLL) : 0;
            const int pos = spgemm_lower_bound(ci + c0, clen, j);
            if (pos < clen && (int64_t)ci[c0 + pos] == j) s += VT<V>::up(av[tperm[u]]) * VT<V>::up(gv[c0 + pos]);
        }
    }
    static_cast<V*>(P.out)[e] = VT<V>::down(s);
}

template <typename F>
inline int spgemm_dispatch_bin(int bin, F&& f) {
    // f(GROUP, CAP, GLOBAL)
    switch (bin) {
        case 0: return f(std::integral_constant<int, kSpgemmGroup[0]>{}, std::integral_constant<int, kSpgemmLimit[0]>{}, std::false_type{});
        case 1: return f(std::integral_constant<int, kSpgemmGroup[1]>{}, std::integral_constant<int, kSpgemmLimit[1]>{}, std::false_type{});
        case 2: return f(std::integral_constant<int, kSpgemmGroup[2]>{}, std::integral_constant<int, kSpgemmLimit[2]>{}, std::false_type{});
        case 3: return f(std::integral_constant<int, kSpgemmGroup[3]>{}, std::integral_constant<int, 0>{}, std::true_type{});
    }
    return TSGU_ERR_BAD_ARG;
}

}  // namespace tsgu
