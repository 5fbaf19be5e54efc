// Zero-fill incomplete factorisations, ILU(0) and IC(0), as ONE persistent, dependency-driven launch (include/tsgu_hip_factor.h).
//
// Row i of either factor needs the FINISHED rows k < i whose columns it stores — the dependency structure of a lower triangular
// solve on the same pattern.  So the rows are dealt exactly as csrc/sptrsm.hip deals them (sptrsm_common.h: ascending tickets per
// class, one wave per row, a persistent grid that never has more waves than rows), and its forward-progress argument holds word
// for word: a ticket is only drawn by a wave that is running, a wave owns one row at a time, and a wave waits on rows BELOW its
// own only — whatever the index arrays contain (an entry with a column >= i is never waited on, and never read).
//
// Hand-off: a row is tens to hundreds of bytes, so it is published with a flag (`done[row]`), not as tagged granules:
//   producer   the row's values with agent-scope relaxed atomic stores (write-through), s_waitcnt vmcnt(0), then ONE store of the
//              flag word with an agent-scope atomic (issued wave-wide with one value: see the end of the kernel's loop);
//   consumer   polls the flags of its dependencies with relaxed agent-scope loads, issues ONE agent-scope acquire, then reads the
//              rows with plain vector loads (never through the scalar cache: every load of `out` has a lane-dependent address).
// A row waits in two rounds — all dependencies but the nearest, which are folded in while the nearest (as a rule row i-1, the
// critical path) is still being computed, then the nearest — so it pays two acquires, not one per dependency.
//
// The row under construction (columns + working values) is staged in the wave's LDS slice; membership (i, j) is a binary search
// over its ascending columns.  A row longer than the slice works in `out` itself with write-through accesses (its entries are
// private to the wave until the flag is stored) and searches `idx` in global memory.
//
// Arithmetic: one IEEE division, multiplication and subtraction per update in the value type, no contraction (the build has
// -ffp-contract=off), every w_j updated serially in ascending k: ILU(0) is bit-identical to the sequential IKJ loop.  IC(0) sums
// each dot product per lane in ascending order of row k's entries and then over the lanes by a fixed butterfly: the order depends
// on the two rows only.  A breakdown (ILU: a zero pivot; IC: a radicand that is not positive) never stalls anything: the row is
// finished with IEEE arithmetic and published, and the lowest such row is recorded (`bad` = max of ~row: zero means clean).
#pragma once

#include "sptrsm_common.h"

namespace tsgu {

// The re-initialised block at the start of the work buffer: one hipMemsetAsync of factor_zero_bytes(n) per call.
struct FactorWork {
    int error;                 // byte 0: set by a wave whose wait expired; every other wave leaves when it sees it
    int pad;
    unsigned long long bad;    // max over the rows that broke down of ~row (0: none): the lowest such row wins
    unsigned long long class_ticket[kTicketWords];
    // unsigned int done[n] follows
};

inline int64_t factor_zero_bytes(int64_t n) { return ((int64_t)sizeof(FactorWork) + 4 * n + 15) / 16 * 16; }

template <typename V>
struct FactorGeom;
template <>
struct FactorGeom<float> {
    static constexpr int kCap = 512;   // entries of a row staged in LDS: 4 waves x 512 x (4 + 4) bytes = 16 KiB per workgroup
};
template <>
struct FactorGeom<double> {
    static constexpr int kCap = 384;   // 4 x 384 x (4 + 8) = 18 KiB: eight workgroups per CU still fit the 160 KiB
};

struct FactorParams {
    int64_t n, nnz;
    const void* ptr;
    const void* idx;
    const void* diag_pos;
    const void* val;
    void* out;
    FactorWork* work;
    double diag_scale;        // 1 + shift
    int wgc;                  // workgroup classes (1 … 64)
    long long timeout_ticks;
};

// A value that is the same in every lane, as a scalar.  The row a wave owns, the dependency it folds in and every extent derived
// from them are wave-uniform by construction, but they come out of `__shfl` / LDS / vector loads, which the compiler takes for
// lane-dependent: it would then structurise the loops around them per lane (lanes that "leave later" iterate without lane 0's
// ticket draw, and the cross-lane operations inside stop being wave-wide).  Saying so keeps all control flow scalar.
__device__ __forceinline__ int64_t uniform(int64_t x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// ---- the row under construction ----------------------------------------------------------------------------------------------
template <typename V, typename I>
struct LdsRow {
    int* cols;
    V* w;
    __device__ __forceinline__ int64_t col(int64_t m) const { return cols[m]; }
    __device__ __forceinline__ V get(int64_t m) const { return w[m]; }
    __device__ __forceinline__ void put(int64_t m, V v) const { w[m] = v; }
    // LDS operations of one wave complete in issue order; this only keeps the compiler from moving them across a pass
    __device__ __forceinline__ void pass_done() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
};

template <typename V, typename I>
struct GlobalRow {
    using Bits = typename Sentinel<V>::Bits;
    const I* idx;   // + row start
    Bits* w;        // out + row start
    __device__ __forceinline__ int64_t col(int64_t m) const { return (int64_t)idx[m]; }
    __device__ __forceinline__ V get(int64_t m) const {
        return Sentinel<V>::val(__hip_atomic_load(w + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __device__ __forceinline__ void put(int64_t m, V v) const {
        __hip_atomic_store(w + m, Sentinel<V>::bits(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // another lane reads what this lane wrote in the next pass: the stores are drained first
    __device__ __forceinline__ void pass_done() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// position of column j among the ascending columns [lo, hi) of the row, or -1
template <typename Row>
__device__ __forceinline__ int64_t find_col(const Row& r, int64_t lo, int64_t hi, int64_t j) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t c = r.col(mid);
        if (c == j) return mid;
        if (c < j) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// Wait for the rows that the entries [qa, qb) of row i name (only those below i), then ONE acquire.  False: the wait expired or
// another wave gave up.
template <typename Row>
__device__ __forceinline__ bool wait_rows(const Row& r, int64_t qa, int64_t qb, int64_t i, const unsigned int* done, int lane,
                                          const FactorParams& P) {
    if (qa >= qb) return true;
    long long t0 = 0;
    for (int64_t base = qa; base < qb; base += kWave) {
        const int64_t q = base + lane;
        int64_t k = -1;
        if (q < qb) k = r.col(q);
        const bool need = k >= 0 && k < i;
        unsigned int flag = 0;
        for (unsigned spin = 0;; ++spin) {
            if (need && flag == 0) flag = __hip_atomic_load(done + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!__any(need && flag == 0)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((spin & 255u) == 255u) {      // the wall clock and the error word, as the triangular solve consults them
                const long long now = wall_clock64();
                if (t0 == 0) t0 = now;
                if (__any(now - t0 > P.timeout_ticks || __hip_atomic_load(&P.work->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0))
                    return false;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return true;
}

// The (clamped) extent of a finished row k and its diagonal position; false when the arrays do not describe one.
template <typename I>
__device__ __forceinline__ bool row_extent(const I* ptr, const I* dpos, int64_t k, int64_t nnz, int64_t& s, int64_t& e, int64_t& d) {
    s = uniform((int64_t)ptr[k]);
    e = uniform((int64_t)ptr[k + 1]);
    d = uniform((int64_t)dpos[k]);
    return s >= 0 && e <= nnz && d >= s && d < e;
}

// ---- ILU(0): fold the finished rows named by the entries [qa, qb) of row i into it, in ascending order -------------------------
template <typename V, typename I, typename Row>
__device__ __forceinline__ void ilu_fold(const Row& r, int64_t qa, int64_t qb, int64_t len, int64_t i, const I* ptr, const I* idx,
                                         const I* dpos, const V* out, int64_t nnz, int lane) {
    for (int64_t q = qa; q < qb; ++q) {
        const int64_t k = uniform(r.col(q));
        if (k < 0 || k >= i) continue;
        int64_t sk, ek, dk;
        const bool ok = row_extent(ptr, dpos, k, nnz, sk, ek, dk);
        if (!ok) {
            sk = ek = dk = 0;
        }
        // lane 0 of the first pass holds the pivot out[k,k], the other lanes row k's upper entries
        V wk = 0;
        for (int64_t base = dk; base < ek || base == dk; base += kWave) {
            const int64_t p = base + lane;
            V u = 0;
            int64_t j = -1;
            if (ok && p < ek) {
                u = out[p];
                j = (int64_t)idx[p];
            }
            if (base == dk) {
                const V piv = __shfl(u, 0, kWave);
                wk = r.get(q) / piv;
                r.pass_done();
                r.put(q, wk);              // every lane, the same value: nothing in these loops is one lane's business (below)
                if (lane == 0) j = -1;
            }
            if (j > k) {
                const int64_t m = find_col(r, q + 1, len, j);
                if (m >= 0) {
                    const V prod = wk * u;
                    r.put(m, r.get(m) - prod);
                }
            }
            r.pass_done();
        }
    }
}

// ---- IC(0): l_ik for the entries [qa, qb) of row i, in ascending order ------------------------------------------------------------
template <typename V, typename I, typename Row>
__device__ __forceinline__ void ic_fold(const Row& r, int64_t qa, int64_t qb, int64_t i, const I* ptr, const I* idx, const I* dpos,
                                        const V* out, int64_t nnz, int lane) {
    for (int64_t q = qa; q < qb; ++q) {
        const int64_t k = uniform(r.col(q));
        if (k < 0 || k >= i) continue;
        int64_t sk, ek, dk;
        const bool ok = row_extent(ptr, dpos, k, nnz, sk, ek, dk);
        if (!ok) {
            sk = ek = dk = 0;
        }
        // the lanes stride over row k's strictly lower part and its diagonal [sk, dk]; each keeps its partial sum in ascending order
        V acc = 0;
        V piv = 0;
        for (int64_t base = sk; base <= dk; base += kWave) {
            const int64_t p = base + lane;
            V l = 0;
            int64_t j = -1;
            if (ok && p <= dk) {
                l = out[p];
                j = (int64_t)idx[p];
            }
            if (dk - base < kWave) piv = __shfl(l, (int)(dk - base), kWave);
            if (p < dk && j >= 0 && j < k) {
                const int64_t m = find_col(r, 0, q, j);
                if (m >= 0) {
                    const V prod = r.get(m) * l;
                    acc = acc + prod;
                }
            }
        }
        const V total = entry_sum<V, kWave>(acc);
        const V lik = (r.get(q) - total) / piv;
        r.pass_done();
        r.put(q, lik);
        r.pass_done();
    }
}

// One row, staged (LdsRow) or in place (GlobalRow).  False: a wait expired.
template <typename V, typename I, bool IC, typename Row>
__device__ __forceinline__ bool factor_row(const Row& r, int64_t i, int64_t s, int64_t len, int64_t nlow, int64_t dq,
                                           const FactorParams& P, unsigned int* done, int lane) {
    const I* ptr = static_cast<const I*>(P.ptr);
    const I* idx = static_cast<const I*>(P.idx);
    const I* dpos = static_cast<const I*>(P.diag_pos);
    const V* out = static_cast<const V*>(P.out);
    // two rounds: everything but the nearest dependency, then the nearest
    const int64_t split = nlow > 1 ? nlow - 1 : 0;
    for (int round = 0; round < 2; ++round) {
        const int64_t qa = round == 0 ? 0 : split;
        const int64_t qb = round == 0 ? split : nlow;
        if (qa >= qb) continue;
        if (!wait_rows(r, qa, qb, i, done, lane, P)) return false;
        if constexpr (IC) ic_fold<V, I>(r, qa, qb, i, ptr, idx, dpos, out, P.nnz, lane);
        else ilu_fold<V, I>(r, qa, qb, len, i, ptr, idx, dpos, out, P.nnz, lane);
    }
    bool broke = false;
    if constexpr (IC) {
        // l_ii = sqrt(a_ii − Σ l_ij²) over the strictly lower entries
        V acc = 0;
        for (int64_t base = 0; base < nlow; base += kWave) {
            const int64_t m = base + lane;
            if (m < nlow) {
                const V l = r.get(m);
                const V sq = l * l;
                acc = acc + sq;
            }
        }
        const V total = entry_sum<V, kWave>(acc);
        if (dq >= 0) {
            const V rad = r.get(dq) - total;
            broke = !(rad > (V)0);
            r.pass_done();
            r.put(dq, sqrt(rad));
            r.pass_done();
        }
    } else {
        if (dq >= 0) broke = r.get(dq) == (V)0;
    }
    if (__any(broke)) __hip_atomic_fetch_max(&P.work->bad, ~(unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

template <typename V, typename I, bool IC>
__global__ __launch_bounds__(kBlock) void factor_syncfree_kernel(const FactorParams P) {
    using S = Sentinel<V>;
    using Bits = typename S::Bits;
    constexpr int kCap = FactorGeom<V>::kCap;
    __shared__ int s_cols[kTrsmWaves][kCap];
    __shared__ V s_w[kTrsmWaves][kCap];

    const int lane = threadIdx.x & (kWave - 1);
    const int slot = threadIdx.x / kWave;
    const int wg = (int)(blockIdx.x % (unsigned)P.wgc);
    const int cls = wg * kTrsmWaves + slot;
    const int ncls = P.wgc * kTrsmWaves;
    const I* ptr = static_cast<const I*>(P.ptr);
    const I* idx = static_cast<const I*>(P.idx);
    const I* dpos = static_cast<const I*>(P.diag_pos);
    const V* val = static_cast<const V*>(P.val);
    Bits* out = static_cast<Bits*>(P.out);
    FactorWork* work = P.work;
    unsigned int* done = reinterpret_cast<unsigned int*>(work + 1);
    unsigned long long* const counter = &work->class_ticket[(slot * 64 + wg) * kTicketStride];
    const V scale = (V)P.diag_scale;
    // (columns are staged as 32-bit words: a matrix with more columns than that works in place)
    const int64_t cap = P.n > 0x7fffffffLL ? 0 : kCap;

    for (;;) {
        const unsigned long long t = (unsigned long long)uniform((int64_t)next_row_ticket(counter, lane, ncls, cls));
        if (t >= (unsigned long long)P.n) break;
        const int64_t i = (int64_t)t;
        int64_t s = uniform((int64_t)ptr[i]);
        int64_t e = uniform((int64_t)ptr[i + 1]);
        if (s < 0) s = 0;
        if (e > P.nnz) e = P.nnz;
        if (e < s) e = s;
        const int64_t len = e - s;
        int64_t dq = uniform((int64_t)dpos[i]) - s;          // the diagonal's place in the row (-1: the arrays name none)
        if (dq < 0 || dq >= len) dq = -1;
        // the entries in front of the diagonal are the dependencies (IC: the diagonal closes the row)
        const int64_t nlow = dq >= 0 ? dq : (IC ? len : 0);
        bool alive;
        if (len <= cap) {
            for (int64_t m = lane; m < len; m += kWave) {
                s_cols[slot][m] = (int)idx[s + m];
                V a = val[s + m];
                if (m == dq) a = a * scale;
                s_w[slot][m] = a;
            }
            const LdsRow<V, I> r{s_cols[slot], s_w[slot]};
            r.pass_done();
            alive = factor_row<V, I, IC>(r, i, s, len, nlow, dq, P, done, lane);
            if (alive) {
                for (int64_t m = lane; m < len; m += kWave)
                    __hip_atomic_store(out + s + m, S::bits(s_w[slot][m]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            const GlobalRow<V, I> r{idx + s, out + s};
            for (int64_t m = lane; m < len; m += kWave) {
                V a = val[s + m];
                if (m == dq) a = a * scale;
                r.put(m, a);
            }
            r.pass_done();
            alive = factor_row<V, I, IC>(r, i, s, len, nlow, dq, P, done, lane);
        }
        if (!alive) {
            __hip_atomic_store(&work->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        // publish: every store of the row has reached the L2 before the flag is raised.  The flag is ONE word and one store
        // instruction, issued by the whole wave with the same value (one write of one dword), not under `if (lane == 0)`: a
        // one-lane tail in front of the loop's back edge let the compiler send the other 63 lanes round the loop ahead of lane 0
        // — past its ticket draw, into the `__shfl` that hands the ticket out — and the wave then took row `cls` for ever.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(done + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// info = 1 + the lowest row that broke down, 0 when none did (behind the factorisation on its stream)
__global__ void factor_info_kernel(const FactorWork* work, int64_t* info) {
    const unsigned long long b = work->bad;
    *info = b ? (int64_t)(~b) + 1 : 0;
}

}  // namespace tsgu
