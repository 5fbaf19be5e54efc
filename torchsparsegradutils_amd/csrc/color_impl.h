// The kernels of the multicolour ordering (tsgu_hip_color.h): one round of the greedy colouring, the check of a colouring, and the
// sweep of one colour class of a triangular solve.
//
// round    A group of W = 4 … 64 lanes owns a node, as in the hop of amg_impl.h.  It walks row i of A and, when given, row i of Aᵀ
//          (one list of len(A_i) + len(Aᵀ_i) entries, lane t takes the entries t, t + W, …).  An uncoloured node with no uncoloured
//          neighbour of greater key (lowbias32(j), j) takes the smallest colour no neighbour holds, found in windows of 64 colours
//          (one 64-bit mask per lane, folded by an OR butterfly; the row is walked again for the next window when all 64 are
//          taken).  Every decision reads the colours of the round's start (`in`) and writes `out`: no in-round visibility is
//          relied on, and an OR is exact and order-free, so the result does not depend on W or on the grid.  No atomics but the
//          relaxed OR into the `undecided` word.
// check    per node: its colour is inside [0, n_colors) and no neighbour holds it; the lowest offending row + 1 by an atomic min.
// sweep    x[i] = (b[bmap(i)] − Σ_e val[vmap(e)]·x[idx[e]]) / val[vmap(diag[i])] for the rows [row0, row1) of one colour class — the
//          rows of a class read rows of other classes only, so the update is in place and wait-free.  The row walk and the column
//          tiling are those of amg_affine_kernel: 8 lanes own a row and a tile of CL columns, EP = 8 / CL lanes along the entries,
//          folded by the fixed tree of `ep_sum`.  A group of 8·m lanes covers m column tiles of its row: the order in which an
//          element is summed depends on its row and on p alone.
//
// The trip counts of the entry loops are wave-uniform scalars that only predicate lanes off.  Every index read from memory is
// checked against its array before it is used: no kernel depends on values to stay in bounds.
#pragma once

#include "amg_impl.h"

namespace tsgu {

constexpr int kColorWindow = 64;       // colours one pass over a row looks at
constexpr int kSweepGroupMin = 8;      // the narrowest and the widest lane group of the sweep (powers of two in between)
constexpr int kSweepGroupMax = 64;

struct ColorParams {
    int64_t n, nnz, nnz_t, n_colors;
    const void* ptr;
    const void* idx;
    const void* tptr;      // may be null: the pattern is structurally symmetric
    const void* tidx;
    const int* in;
    int* out;
    unsigned long long* word;      // round: the `undecided` word.  check: the lowest offending row + 1
};

// (lowbias32(a), a) > (lowbias32(b), b)
__device__ __forceinline__ bool color_key_greater(int64_t a, int64_t b) {
    const unsigned ha = amg_lowbias32((unsigned)a), hb = amg_lowbias32((unsigned)b);
    return ha != hb ? ha > hb : a > b;
}

// entry k of the list "row i of A, then row i of Aᵀ"
template <typename I>
__device__ __forceinline__ int64_t color_neighbour(const I* __restrict__ idx, const I* __restrict__ tidx, int64_t s, int64_t len_a,
                                                   int64_t ts, int64_t k) {
    return k < len_a ? (int64_t)idx[s + k] : (int64_t)tidx[ts + (k - len_a)];
}

template <int W>
__device__ __forceinline__ unsigned long long color_fold_or(unsigned long long m) {
#pragma unroll
    for (int k = W / 2; k >= 1; k >>= 1) m |= __shfl_xor(m, k, W);
    return m;
}

template <typename I, int W>
__global__ __launch_bounds__(kBlock) void color_round_kernel(const ColorParams P) {
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ tptr = static_cast<const I*>(P.tptr);
    const I* __restrict__ tidx = static_cast<const I*>(P.tidx);
    const int* __restrict__ in = P.in;
    const int t = threadIdx.x % W;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W;
    int64_t s, e, ts = 0, te = 0;
    amg_extent<I>(ptr, row, P.n, P.nnz, s, e);
    if (tptr) amg_extent<I>(tptr, row, P.n, P.nnz_t, ts, te);
    const int own = row < P.n ? in[row] : 0;
    const bool active = row < P.n && own < 0;
    const int64_t len_a = e - s, len = active ? len_a + (te - ts) : 0;
    const int64_t steps = (amg_wave_max(len) + W - 1) / W;

    // first pass: is a neighbour of greater key still uncoloured, and which of the colours 0 … 63 are taken
    unsigned long long mask = 0ull, blocked = 0ull;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t k = it * W + t;
        if (k < len) {
            const int64_t j = color_neighbour<I>(idx, tidx, s, len_a, ts, k);
            if (j >= 0 && j < P.n && j != row) {
                const int c = in[j];
                if (c < 0) blocked |= color_key_greater(j, row) ? 1ull : 0ull;
                else if (c < kColorWindow) mask |= 1ull << c;
            }
        }
    }
    mask = color_fold_or<W>(mask);
    blocked = color_fold_or<W>(blocked);
    const bool decide = active && !blocked;
    int color = -1;
    if (decide && mask != ~0ull) color = __builtin_ctzll(~mask);

    // further windows: len neighbours hold at most len colours, so a window that starts at or below len has a free one
    int64_t base = kColorWindow;
    while (__any(decide && color < 0 && base <= len)) {
        const bool need = decide && color < 0 && base <= len;
        mask = 0ull;
        for (int64_t it = 0; it < steps; ++it) {
            const int64_t k = it * W + t;
            if (need && k < len) {
                const int64_t j = color_neighbour<I>(idx, tidx, s, len_a, ts, k);
                if (j >= 0 && j < P.n && j != row) {
                    const int64_t c = (int64_t)in[j] - base;
                    if (c >= 0 && c < kColorWindow) mask |= 1ull << c;
                }
            }
        }
        mask = color_fold_or<W>(mask);
        if (need && mask != ~0ull) color = (int)(base + __builtin_ctzll(~mask));
        base += kColorWindow;
    }
    if (t == 0 && row < P.n) {
        P.out[row] = decide ? color : own;
        if (active && !decide) __hip_atomic_fetch_or(P.word, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename I, int W>
__global__ __launch_bounds__(kBlock) void color_check_kernel(const ColorParams P) {
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ tptr = static_cast<const I*>(P.tptr);
    const I* __restrict__ tidx = static_cast<const I*>(P.tidx);
    const int* __restrict__ in = P.in;
    const int t = threadIdx.x % W;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W;
    int64_t s, e, ts = 0, te = 0;
    amg_extent<I>(ptr, row, P.n, P.nnz, s, e);
    if (tptr) amg_extent<I>(tptr, row, P.n, P.nnz_t, ts, te);
    const int own = row < P.n ? in[row] : 0;
    const int64_t len_a = e - s, len = len_a + (te - ts);
    const int64_t steps = (amg_wave_max(len) + W - 1) / W;
    unsigned long long bad = row < P.n && (own < 0 || (int64_t)own >= P.n_colors) ? 1ull : 0ull;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t k = it * W + t;
        if (k < len) {
            const int64_t j = color_neighbour<I>(idx, tidx, s, len_a, ts, k);
            if (j >= 0 && j < P.n && j != row && in[j] == own) bad = 1ull;
        }
    }
    bad = color_fold_or<W>(bad);
    if (t == 0 && row < P.n && bad) __hip_atomic_fetch_min(P.word, (unsigned long long)row + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the word of the check starts at all ones (no offender): that becomes 0
__global__ void color_check_finish_kernel(unsigned long long* word) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && *word == ~0ull) *word = 0ull;
}

constexpr int kSweepDivide = 0;        // x = s / d
constexpr int kSweepUnit = 1;          // x = s
constexpr int kSweepScaled = 2;        // x = b − Σ / d

struct ColorSweepParams {
    int64_t n, nnz, n_val, row0, row1, p;
    const void* begin;
    const void* end;
    const void* idx;
    const void* diag;          // may be null (unit mode)
    const void* vmap;          // may be null: identity
    const void* val;
    const void* b;
    const void* bmap;          // may be null: identity
    void* x;
    void* out;                 // may be null
    const void* out_rows;      // may be null: identity
    int64_t ldb, ldx, ldo;
    int mode, group;
};

template <typename V, typename I, int CL>
__global__ __launch_bounds__(kBlock) void color_sweep_kernel(const ColorSweepParams P) {
    constexpr int EP = kAmgGroup / CL;
    const I* __restrict__ begin = static_cast<const I*>(P.begin);
    const I* __restrict__ end = static_cast<const I*>(P.end);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const I* __restrict__ diag = static_cast<const I*>(P.diag);
    const I* __restrict__ vmap = static_cast<const I*>(P.vmap);
    const I* __restrict__ bmap = static_cast<const I*>(P.bmap);
    const I* __restrict__ out_rows = static_cast<const I*>(P.out_rows);
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* B = static_cast<const V*>(P.b);
    V* X = static_cast<V*>(P.x);
    V* Out = static_cast<V*>(P.out);

    const int W = P.group;
    const int gl = threadIdx.x % W;
    const int l8 = gl % kAmgGroup, sub = gl / kAmgGroup;
    const int cl = l8 % CL, ep = l8 / CL;
    const int64_t row = P.row0 + (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W;
    const int64_t col = ((int64_t)blockIdx.y * (W / kAmgGroup) + sub) * CL + cl;
    const bool row_ok = row < P.row1;
    const bool col_ok = col < P.p;

    int64_t s = 0, e = 0;
    if (row_ok) {
        s = (int64_t)begin[row];
        e = (int64_t)end[row];
        if (s < 0) s = 0;
        if (e > P.nnz) e = P.nnz;
        if (e < s) e = s;
    }
    const int64_t steps = (amg_wave_max(e - s) + EP - 1) / EP;
    V acc = (V)0;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t k = s + it * EP + ep;
        if (k < e && col_ok) {
            const int64_t j = (int64_t)idx[k];
            const int64_t q = vmap ? (int64_t)vmap[k] : k;
            if (j >= 0 && j < P.n && q >= 0 && q < P.n_val) {
                const V prod = val[q] * X[j * P.ldx + col];
                acc = acc + prod;
            }
        }
    }
    acc = ep_sum<V, CL, EP>(acc);
    if (ep == 0 && col_ok && row_ok) {
        const int64_t br = bmap ? (int64_t)bmap[row] : row;
        const int64_t orow = out_rows ? (int64_t)out_rows[row] : row;
        int64_t dq = 0;
        if (P.mode != kSweepUnit) {
            dq = (int64_t)diag[row];
            if (vmap && dq >= 0 && dq < P.nnz) dq = (int64_t)vmap[dq];
            else if (vmap) dq = -1;
        }
        const bool d_ok = P.mode == kSweepUnit || (dq >= 0 && dq < P.n_val);
        if (br >= 0 && br < P.n && d_ok && (!Out || (orow >= 0 && orow < P.n))) {
            const V rhs = B[br * P.ldb + col];
            V r;
            if (P.mode == kSweepUnit) r = rhs - acc;
            else if (P.mode == kSweepDivide) r = (rhs - acc) / val[dq];
            else r = rhs - acc / val[dq];
            X[row * P.ldx + col] = r;
            if (Out) Out[orow * P.ldo + col] = r;
        }
    }
}

}  // namespace tsgu
