// What the two kernel families of the triangular solve share (csrc/sptrsm.hip: the sync-free CSR sweep; csrc/sptrsm_lattice.hip:
// the line sweep on stencil factors): the work buffer with its tickets and error word, the "not ready" tag of every value type,
// the kernel that pre-fills X with it, and the sum over a column's entry lanes.  The ordered row tickets, the time bound of every spin
// and the size of the persistent grid are shared with the incomplete factorisations as well (csrc/ilu_impl.h), whose rows depend
// on one another exactly as the rows of a lower solve do.
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kTrsmWaves = kBlock / kWave;   // waves of a workgroup = row classes (below)

struct TrsmWork {
    unsigned long long ticket[64];  // (kept for the layout: the error word stays at byte 512)
    int error;
    int pad[15];
    // Row tickets: rows are dealt to CLASSES, class c draws the rows ≡ c (mod classes) in order from its own counter (128 bytes
    // apart).  A class is (wave slot of a workgroup, workgroup index mod `wgc`) — up to 4 x 64 classes; with several column tiles
    // (p > 64) it is (wave slot, tile) as before.  ONE counter serves ~80 M same-address atomics per second: with one counter for
    // all rows that was the solve time of C3 (262144 rows: 3.2 ms whatever the pollers did), with four it still is the solve time
    // of a SHALLOW pattern (the reference's published shape, one off-diagonal entry per row: 65536 atomics per counter = 0.84 ms
    // whatever the number of waves).  Forward progress, per class: a counter hands its rows out in order, so every row of the class
    // below the lowest unfinished one is finished and the waves that held them are free to take it; every class has a resident wave
    // (the grid is persistent and never smaller than `wgc` workgroups).
    unsigned long long class_ticket[kTrsmWaves * 64 * 16];   // (= kTicketWords, below)
};

// ---- ordered row tickets, bounded spins, persistent grid (sptrsm.hip, ilu_impl.h) ----------------------------------------------
constexpr int kTicketStride = 16;                         // counters 128 bytes apart
constexpr int kTicketWords = kTrsmWaves * 64 * kTicketStride;
constexpr long long kSpinTimeoutTicks = 400000000LL;      // 4 s at the 100 MHz wall clock

// The next row of class `cls` out of `ncls` (rows ≡ cls mod ncls, in order), drawn by lane 0 for its wave.  The caller stops at
// the first ticket >= n.
__device__ __forceinline__ unsigned long long next_row_ticket(unsigned long long* counter, int lane, int ncls, int cls) {
    unsigned long long t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add(counter, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __shfl(t, 0, kWave) * ncls + cls;
}

// Workgroups of the persistent grid: `wg_per_cu` (1 … 8) per compute unit, never more waves than rows.
inline int64_t persistent_blocks(int n_cu, int wg_per_cu, int64_t n_rows) {
    if (wg_per_cu < 1) wg_per_cu = 1;
    if (wg_per_cu > 8) wg_per_cu = 8;
    int64_t blocks = (int64_t)n_cu * wg_per_cu;
    const int64_t need = (n_rows + kTrsmWaves - 1) / kTrsmWaves;
    return blocks > need ? need : blocks;
}

template <typename V>
struct Sentinel;
template <>
struct Sentinel<float> {
    using Bits = unsigned int;
    static constexpr Bits kTag = 0x7fc5a5a5u;    // quiet NaN, private payload
    static constexpr Bits kCanon = 0x7fc00000u;  // what a genuine NaN result is stored as
    __device__ static __forceinline__ Bits bits(float v) { return __float_as_uint(v); }
    __device__ static __forceinline__ float val(Bits b) { return __uint_as_float(b); }
};
template <>
struct Sentinel<double> {
    using Bits = unsigned long long;
    static constexpr Bits kTag = 0x7ff8a5a5a5a5a5a5ull;
    static constexpr Bits kCanon = 0x7ff8000000000000ull;
    __device__ static __forceinline__ Bits bits(double v) { return (Bits)__double_as_longlong(v); }
    __device__ static __forceinline__ double val(Bits b) { return __longlong_as_double((long long)b); }
};

template <>
struct Sentinel<bf16_t> {   // bf16 elements, fp32 arithmetic: x is rounded once, when it is published
    using Bits = unsigned short;
    static constexpr Bits kTag = 0x7fc5u;
    static constexpr Bits kCanon = 0x7fc0u;
    __device__ static __forceinline__ Bits bits(float v) { return VT<bf16_t>::down(v).bits; }
    __device__ static __forceinline__ float val(Bits b) { return __uint_as_float((unsigned int)b << 16); }
};

template <typename V>
__global__ __launch_bounds__(kBlock) void sptrsm_fill_kernel(void* X, int64_t ldx, int64_t n, int64_t p, TrsmWork* work) {
    using S = Sentinel<V>;
    using Bits = typename S::Bits;
    Bits* x = static_cast<Bits*>(X);
    const int64_t total = n * p;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / p, c = i - r * p;
        __hip_atomic_store(x + r * ldx + c, S::kTag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i < kTrsmWaves * 64; i += kBlock)
            __hip_atomic_store(&work->class_ticket[i * 16], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        __hip_atomic_store(&work->ticket[threadIdx.x], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0) __hip_atomic_store(&work->error, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Sum over the EP consecutive lanes of a group (every lane gets the total): DPP for groups up to a row of 16, wave shuffles beyond
template <typename A, int EP>
__device__ __forceinline__ A entry_sum(A x) {
    if constexpr (EP <= 16) {
        return group_sum<A, EP>(x);
    } else {
        x = group_sum<A, 16>(x);
#pragma unroll
        for (int m = 16; m < EP; m <<= 1) x += shfl_xor_acc(x, m);
        return x;
    }
}

}  // namespace tsgu
