// The kernels of the aggregation multigrid preconditioner (tsgu_hip_amg.h): the key hop and the node update of the MIS-2
// aggregation, and the affine product every step of the V-cycle is one launch of.
//
// hop      out[i] = max(in[i], max_{j in row i} in[col_j]) over unsigned 64-bit keys.  Pull-style: a group of W = 4 … 64 lanes owns
//          a row, lane t gathers the keys of the entries t, t + W, … with 8-byte loads, and the group folds with a fixed xor
//          butterfly — a max is exact and order-free, so the result does not depend on W or on the grid.  No atomics.
// update   per node: the MIS-2 state machine on (key, t = hop(hop(key))), the initial keys, or the root keys of the assignment.
// affine   Out = C + alpha·w∘(B − A·X), row-major (n, p) operands.  A group of 8 lanes owns a row: CL = 1, 2, 4 or 8 lanes along
//          a tile of CL columns, EP = 8 / CL lanes along the entries.  Entry lane e sums the entries e, e + EP, … in ascending
//          order and the EP partial sums are folded by the fixed tree of `ep_sum`: the bits of an element depend on its row and on
//          p alone.  The epilogue is row-local (each element of Out is written by the lane that read the same element of C and B),
//          so Out may be C or B.
//
// The trip counts of the entry loops are wave-uniform scalars (the longest row of the wave, through `readfirstlane`) that only
// predicate lanes off: no loop ends in a tail that part of a wave walks alone.  Every index read from memory is checked against its
// array before it is used: no kernel depends on values to stay in bounds.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kAmgGroupMin = 4;        // the narrowest and the widest lane group of the hop (powers of two in between)
constexpr int kAmgGroupMax = 64;
constexpr int kAmgColumnTile = 8;      // columns of a tile of the affine product (= lanes of a row group)
constexpr int kAmgGroup = 8;           // lanes of a row group of the affine product

constexpr unsigned long long kAmgLow = (1ull << 62) - 1;      // priority and index of a key
constexpr unsigned long long kAmgRoot = 2ull << 62;
constexpr unsigned long long kAmgUndecided = 1ull << 62;

struct AmgHopParams {
    int64_t n, nnz;
    const void* ptr;
    const void* idx;
    const unsigned long long* in;
    unsigned long long* out;
};

// the longest extent of the wave as a scalar
__device__ __forceinline__ int64_t amg_wave_max(int64_t len) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const int64_t other = __shfl_xor(len, m, kWave);
        len = other > len ? other : len;
    }
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)len & 0xffffffffull));
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)len >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// the extent [s, e) of row `row` in an array of nnz entries, clamped to it; empty for a row beyond n
template <typename I>
__device__ __forceinline__ void amg_extent(const I* ptr, int64_t row, int64_t n, int64_t nnz, int64_t& s, int64_t& e) {
    s = e = 0;
    if (row >= n) return;
    s = (int64_t)ptr[row];
    e = (int64_t)ptr[row + 1];
    if (s < 0) s = 0;
    if (e > nnz) e = nnz;
    if (e < s) e = s;
}

template <typename I, int W>
__global__ __launch_bounds__(kBlock) void amg_hop_kernel(const AmgHopParams P) {
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const int t = threadIdx.x % W;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W;
    int64_t s, e;
    amg_extent<I>(ptr, row, P.n, P.nnz, s, e);
    const int64_t steps = (amg_wave_max(e - s) + W - 1) / W;
    unsigned long long best = row < P.n ? P.in[row] : 0ull;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t k = s + it * W + t;
        if (k < e) {
            const int64_t c = (int64_t)idx[k];
            if (c >= 0 && c < P.n) {
                const unsigned long long v = P.in[c];
                best = v > best ? v : best;
            }
        }
    }
#pragma unroll
    for (int m = W / 2; m >= 1; m >>= 1) {
        const unsigned long long other = __shfl_xor(best, m, W);
        best = other > best ? other : best;
    }
    if (t == 0 && row < P.n) P.out[row] = best;
}

__device__ __forceinline__ unsigned amg_lowbias32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// mode 0: the initial keys.  mode 1: one round's decision, and `undecided` != 0 when a node is still undecided after it.
// mode 2: the root's own key for roots, 0 otherwise.  (Internal linkage: color_impl.h includes this header for the row walk and the hash.)
static __global__ __launch_bounds__(kBlock) void amg_mis2_kernel(int mode, int64_t n, const unsigned long long* key, const unsigned long long* t,
                                                          unsigned long long* out, unsigned long long* undecided) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) {
        const unsigned prio = amg_lowbias32((unsigned)i) >> 2;
        out[i] = kAmgUndecided | ((unsigned long long)prio << 32) | (unsigned long long)(unsigned)i;
        return;
    }
    const unsigned long long k = key[i];
    const unsigned state = (unsigned)(k >> 62);
    if (mode == 2) {
        out[i] = state == 2u ? k : 0ull;
        return;
    }
    unsigned long long next = k;
    if (state == 1u) {
        const unsigned long long far = t[i];
        if ((unsigned)(far & 0xffffffffull) == (unsigned)i) next = kAmgRoot | (k & kAmgLow);
        else if ((far >> 62) == 2ull) next = k & kAmgLow;
        else __hip_atomic_fetch_or(undecided, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    out[i] = next;
}

struct AmgAffineParams {
    int64_t n_rows, n_cols, nnz, p;
    const void* ptr;
    const void* idx;
    const void* val;
    const void* x;
    const void* c;        // may be null: 0
    const void* b;        // may be null: 0
    const void* w;        // may be null: 1
    void* out;
    int64_t ldx, ldc, ldb, ldo;
    double alpha;
};

template <typename V, typename I, int CL>
__global__ __launch_bounds__(kBlock) void amg_affine_kernel(const AmgAffineParams P) {
    constexpr int EP = kAmgGroup / CL;
    const I* __restrict__ ptr = static_cast<const I*>(P.ptr);
    const I* __restrict__ idx = static_cast<const I*>(P.idx);
    const V* __restrict__ val = static_cast<const V*>(P.val);
    const V* __restrict__ X = static_cast<const V*>(P.x);
    const V* C = static_cast<const V*>(P.c);
    const V* B = static_cast<const V*>(P.b);
    const V* __restrict__ Wt = static_cast<const V*>(P.w);
    V* Out = static_cast<V*>(P.out);

    const int gl = threadIdx.x % kAmgGroup;
    const int cl = gl % CL, ep = gl / CL;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kAmgGroup) + threadIdx.x / kAmgGroup;
    const int64_t col = (int64_t)blockIdx.y * CL + cl;
    const bool col_ok = col < P.p;

    int64_t s, e;
    amg_extent<I>(ptr, row, P.n_rows, P.nnz, s, e);
    const int64_t steps = (amg_wave_max(e - s) + EP - 1) / EP;
    V acc = (V)0;
    for (int64_t it = 0; it < steps; ++it) {
        const int64_t k = s + it * EP + ep;
        if (k < e && col_ok) {
            const int64_t j = (int64_t)idx[k];
            if (j >= 0 && j < P.n_cols) {
                const V prod = val[k] * X[j * P.ldx + col];
                acc = acc + prod;
            }
        }
    }
    acc = ep_sum<V, CL, EP>(acc);
    if (ep == 0 && col_ok && row < P.n_rows) {
        V r = (B ? B[row * P.ldb + col] : (V)0) - acc;
        if (Wt) r = Wt[row] * r;
        r = (V)P.alpha * r;
        Out[row * P.ldo + col] = C ? C[row * P.ldc + col] + r : r;
    }
}

}  // namespace tsgu
