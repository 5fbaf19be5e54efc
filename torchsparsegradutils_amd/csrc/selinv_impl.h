// Takahashi selected inversion as ONE persistent, dependency-driven launch (include/tsgu_hip_selinv.h).
//
// Given the lower factor L of Q = L·Lᵀ (or the unit factor and D of Q = (L+I)·D·(L+I)ᵀ) by its COLUMNS (CSC: ascending rows, the
// diagonal first), the entries of Σ = Q⁻¹ on the pattern of L follow column by column from the right.  With s(i) = s_0 < s_1 < … the
// rows stored below the diagonal of column i and l_a = L[s_a, i]:
//     acc[a]   = Σ_b l_b · Σ[max(s_a, s_b), min(s_a, s_b)]         Σ[s_a, i] = −(1/L_ii) · acc[a]
//     Σ[i, i]  = 1/L_ii² − (1/L_ii) · Σ_a l_a · Σ[s_a, i]           (LDLᵀ: L_ii = 1, and 1/D_i for 1/L_ii²)
// Every Σ on the right-hand side lies in a FINISHED column s_a > i, at a stored position if the pattern is closed under elimination.
//
// Dependencies and forward progress.  Column i needs the finished columns k > i whose rows it stores — the mirror image of the
// factorisations (ilu_impl.h).  The columns are dealt by the same ordered tickets (sptrsm_common.h) in DESCENDING order: ticket t
// is column n − 1 − t.  The argument of ilu_impl.h holds mirrored: a ticket is only drawn by a wave that is running, a wave owns one
// column at a time, and a wave waits only on columns ABOVE its own — whatever the index arrays contain (an entry with a row <= i
// or >= n is never waited on and never read through) —, that is on tickets drawn before its own, whose waves are running or done;
// the column with the lowest unfinished ticket waits on nothing unfinished.  Every wait is bounded by the same timeout and error
// word as there.
//
// The lookup phase.  For a target a, the entries Σ[s_b, s_a] with b >= a all lie in ONE finished column, s_a, whose rows ascend as
// s(i) does.  So the wave SWEEPS that column once, 64 consecutive entries per step (coalesced loads of its rows and values), and
// each lane places its row in s(i): the matches ascend with the lanes, so the search window of a step starts at a cursor behind the
// last match of the step before (a merge at the granularity of a step, a bisection of the remaining window inside it), and the
// sweep ends as soon as the cursor reaches the end of s(i).  One visit (a, b, x = Σ[s_b, s_a]) serves both sums, by symmetry:
//     u      += l_b · x    in the lane's register: its partial of acc[a]
//     acc[b] += l_a · x    in the staged column (the rows of a column are distinct: no two lanes meet in one b)
// Targets are taken in DESCENDING order, the nearest dependency s_0 (as a rule column i+1, the critical path) last and after a wait
// of its own, as the factorisations wait in two rounds.  So acc[a] is first written when target a is swept —
// acc[a] = l_a·Σ[s_a,s_a] + (the lanes' partials folded by the fixed butterfly) — and then receives l_(a−1)·x, l_(a−2)·x, … in that
// order: the order of every sum depends on the pattern only, never on the grid or on timing.  No floating-point atomics;
// -ffp-contract=off; two calls give the same bits.  The number of matches of a sweep must be |s(i)| − 1 − a: fewer is a lookup that
// missed, i.e. a pattern that is not closed; the term is a zero, the sweep goes on, and the lowest such column is recorded
// (`open` = max of ~column).
//
// Staging: the column's rows, its values l and acc live in the wave's LDS slice (SelinvGeom: 4 waves x cap x (4 + 2·sizeof V)
// bytes, eight workgroups per CU fit the 160 KiB).  A longer column reads rows and l from the CSC arrays and keeps acc in the Σ
// array itself with write-through accesses (its entries are private to the wave until the flag is stored).
//
// Hand-off, as ilu_impl.h publishes a row: the column's Σ values go to the CSC-ordered working array `sig` (and, in the order of
// L's own value array, to `out`) with agent-scope relaxed stores, s_waitcnt vmcnt(0), then ONE wave-wide store of done[i].
// Consumers poll the flags relaxed, issue ONE acquire per round, and read `sig` with plain vector loads (the one wave-uniform
// address, a column's diagonal, with an agent-scope atomic load: never through the scalar cache).
//
// A zero or non-finite pivot (L_ii, or D_i) finishes the column with IEEE arithmetic, never stalls a dependant, and the lowest such
// column is recorded (`bad`).  One wave per column at every length: the columns of a banded factor form one dependency chain, so
// sub-wave groups (fsai_impl.h) would add lanes to columns that wait on each other, not throughput — not built.
#pragma once

#include "sptrsm_common.h"

namespace tsgu {

// A value that is the same in every lane, as a scalar (the column a wave owns, the dependency it sweeps and every extent derived
// from them come out of `__shfl` / LDS / vector loads, which the compiler takes for lane-dependent): keeps all control flow around
// the cross-lane operations scalar, as ilu_impl.h explains for its `uniform`.
__device__ __forceinline__ int64_t wave_uniform(int64_t x) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)x);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)x >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// The re-initialised block at the start of the work buffer: one hipMemsetAsync of selinv_zero_bytes(n) per call.
struct SelinvWork {
    int error;                 // byte 0: set by a wave whose wait expired; every other wave leaves when it sees it
    int pad;
    unsigned long long bad;    // max over the columns with a zero / non-finite pivot of ~column (0: none)
    unsigned long long open;   // max over the columns with a lookup that missed of ~column (0: the pattern is closed)
    unsigned long long pad2;
    unsigned long long class_ticket[kTicketWords];
    // unsigned int done[n] follows, then (16-byte aligned, not re-initialised) V sig[nnz]: Σ in CSC order
};

inline int64_t selinv_zero_bytes(int64_t n) { return ((int64_t)sizeof(SelinvWork) + 4 * n + 15) / 16 * 16; }
inline int64_t selinv_work_bytes(int64_t n, int64_t nnz, int64_t vsize) { return selinv_zero_bytes(n) + (nnz * vsize + 15) / 16 * 16; }

template <typename V>
struct SelinvGeom;
template <>
struct SelinvGeom<float> {
    static constexpr int kCap = 384;   // sub-diagonal entries of a column staged in LDS: 4 waves x 384 x (4 + 4 + 4) bytes = 18 KiB
};
template <>
struct SelinvGeom<double> {
    static constexpr int kCap = 224;   // 4 x 224 x (4 + 8 + 8) = 17.5 KiB: eight workgroups per CU still fit the 160 KiB
};

struct SelinvParams {
    int64_t n, nnz;
    const void* ptr;          // CSC of L: column pointers, ascending row indices,
    const void* idx;
    const void* perm;         // position of every CSC entry in L's value array (NULL: identity),
    const void* diag_pos;     // CSC position of every column's diagonal (NULL with D: L is stored strictly lower)
    const void* val;
    const void* D;            // NULL: Q = L·Lᵀ
    void* out;                // Σ at L's stored positions, in the order of `val`
    void* diag_out;           // with D: diag Σ (also the consumers' source of Σ[k,k])
    void* sig;                // Σ in CSC order (inside `work`)
    SelinvWork* work;
    int wgc;
    long long timeout_ticks;
};

template <typename I>
__device__ __forceinline__ int64_t value_pos(const I* perm, int64_t p, int64_t nnz) {
    const int64_t q = perm ? (int64_t)perm[p] : p;
    return (unsigned long long)q < (unsigned long long)nnz ? q : 0;     // (a plan's perm is a permutation; never index past the array)
}

// ---- the column under construction: rows s_a, values l_a, sums acc[a] for a in [0, m) -------------------------------------------
template <typename V>
struct LdsCol {
    const int* rows;
    const V* l;
    V* acc;
    __device__ __forceinline__ int64_t row(int64_t a) const { return rows[a]; }
    __device__ __forceinline__ V lv(int64_t a) const { return l[a]; }
    __device__ __forceinline__ V get(int64_t a) const { return acc[a]; }
    __device__ __forceinline__ void put(int64_t a, V v) const { acc[a] = v; }
    __device__ __forceinline__ void pass_done() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
};

template <typename V, typename I>
struct GlobalCol {
    using Bits = typename Sentinel<V>::Bits;
    const I* idx;     // + the column's first sub-diagonal position p0
    const I* perm;    // whole array (or NULL)
    const V* val;
    Bits* w;          // sig + p0
    int64_t p0, nnz;
    __device__ __forceinline__ int64_t row(int64_t a) const { return (int64_t)idx[a]; }
    __device__ __forceinline__ V lv(int64_t a) const { return val[value_pos(perm, p0 + a, nnz)]; }
    __device__ __forceinline__ V get(int64_t a) const {
        return Sentinel<V>::val(__hip_atomic_load(w + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __device__ __forceinline__ void put(int64_t a, V v) const {
        __hip_atomic_store(w + a, Sentinel<V>::bits(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void pass_done() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// position of row r among the ascending rows [lo, hi) of the column, or -1
template <typename Col>
__device__ __forceinline__ int64_t find_row(const Col& c, int64_t lo, int64_t hi, int64_t r) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const int64_t x = c.row(mid);
        if (x == r) return mid;
        if (x < r) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// Wait for the columns that the entries [qa, qb) of column i name (only those above i), then ONE acquire.  False: the wait expired
// or another wave gave up.
template <typename Col>
__device__ __forceinline__ bool wait_cols(const Col& c, int64_t qa, int64_t qb, int64_t i, const unsigned int* done, int lane,
                                          const SelinvParams& P) {
    if (qa >= qb) return true;
    long long t0 = 0;
    for (int64_t base = qa; base < qb; base += kWave) {
        const int64_t q = base + lane;
        int64_t k = -1;
        if (q < qb) k = c.row(q);
        const bool need = k > i && k < P.n;
        unsigned int flag = 0;
        for (unsigned spin = 0;; ++spin) {
            if (need && flag == 0) flag = __hip_atomic_load(done + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!__any(need && flag == 0)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((spin & 255u) == 255u) {      // the wall clock and the error word, as the factorisations consult them
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

// Sweep the finished column s_a for target a of column i (header comment).  True: a lookup missed.
template <typename V, typename I, bool LDLT, typename Col>
__device__ __forceinline__ bool sweep_target(const Col& c, int64_t a, int64_t m, int64_t i, const SelinvParams& P, int lane) {
    using S = Sentinel<V>;
    using Bits = typename S::Bits;
    const I* ptr = static_cast<const I*>(P.ptr);
    const I* idx = static_cast<const I*>(P.idx);
    const V* sig = static_cast<const V*>(P.sig);
    const int64_t k = wave_uniform(c.row(a));
    int64_t sb = 0, se = 0;          // the sub-diagonal entries of column k
    V xd = 0;                        // Σ[k, k]
    if (k > i && k < P.n) {
        const int64_t s = wave_uniform((int64_t)ptr[k]);
        const int64_t e = wave_uniform((int64_t)ptr[k + 1]);
        if constexpr (LDLT) {
            if (s >= 0 && s <= e && e <= P.nnz) {
                sb = s;
                se = e;
                xd = S::val(__hip_atomic_load(static_cast<const Bits*>(P.diag_out) + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        } else {
            const int64_t d = wave_uniform((int64_t) static_cast<const I*>(P.diag_pos)[k]);
            if (s >= 0 && d >= s && d < e && e <= P.nnz) {
                sb = d + 1;
                se = e;
                xd = S::val(__hip_atomic_load(static_cast<const Bits*>(P.sig) + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            }
        }
    }
    const V la = c.lv(a);
    V u = 0;
    int64_t cursor = a + 1;          // every match of this sweep lies in [cursor, m)
    int64_t hits = 0;
    for (int64_t base = sb; base < se && cursor < m; base += kWave) {
        const int64_t p = base + lane;
        int64_t b = -1;
        if (p < se) {
            const int64_t r = (int64_t)idx[p];
            b = find_row(c, cursor, m, r);
            if (b >= 0) {
                const V x = sig[p];
                const V mine = c.lv(b) * x;
                u = u + mine;
                const V theirs = la * x;
                c.put(b, c.get(b) + theirs);
            }
        }
        const unsigned long long mask = __ballot(b >= 0);
        if (mask) {                  // the rows ascend with the lanes, and so do the matches: the highest lane holds the last one
            const int top = 63 - __builtin_clzll(mask);
            cursor = wave_uniform((int64_t)__shfl((long long)b, top, kWave)) + 1;
            hits += __popcll(mask);
        }
    }
    const V total = entry_sum<V, kWave>(u);
    V t = la * xd;
    t = t + total;
    c.pass_done();
    c.put(a, t);                     // every lane, the same value (acc[a] is first written here: targets descend)
    c.pass_done();
    return hits != m - 1 - a;
}

// One column, staged (LdsCol) or in place (GlobalCol): acc[], then Σ[s_a, i] in its place, and Σ[i, i] (returned in `sii`).
// False: a wait expired.
template <typename V, typename I, bool LDLT, typename Col>
__device__ __forceinline__ bool selinv_column(const Col& c, int64_t i, int64_t m, V pivot, bool pivot_ok, const SelinvParams& P,
                                              unsigned int* done, int lane, V& sii) {
    bool missed = false;
    // two rounds: every dependency but the nearest, then the nearest
    if (m > 1) {
        if (!wait_cols(c, 1, m, i, done, lane, P)) return false;
        for (int64_t a = m - 1; a >= 1; --a) missed |= sweep_target<V, I, LDLT>(c, a, m, i, P, lane);
    }
    if (m > 0) {
        if (!wait_cols(c, 0, 1, i, done, lane, P)) return false;
        missed |= sweep_target<V, I, LDLT>(c, 0, m, i, P, lane);
    }
    const V one = (V)1;
    const V inv = one / pivot;       // LLᵀ: 1/L_ii;  LDLᵀ: 1/D_i
    V w = 0;
    for (int64_t base = 0; base < m; base += kWave) {
        const int64_t a = base + lane;
        if (a < m) {
            V z;
            if constexpr (LDLT) z = -c.get(a);
            else z = -(inv * c.get(a));
            c.put(a, z);
            const V prod = c.lv(a) * z;
            w = w + prod;
        }
    }
    c.pass_done();
    const V total = entry_sum<V, kWave>(w);
    if constexpr (LDLT) {
        sii = inv - total;
    } else {
        const V sq = inv * inv;
        const V cross = inv * total;
        sii = sq - cross;
    }
    if (!pivot_ok) __hip_atomic_fetch_max(&P.work->bad, ~(unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (missed) __hip_atomic_fetch_max(&P.work->open, ~(unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

template <typename V, typename I, bool LDLT>
__global__ __launch_bounds__(kBlock) void selinv_syncfree_kernel(const SelinvParams P) {
    using S = Sentinel<V>;
    using Bits = typename S::Bits;
    constexpr int kCap = SelinvGeom<V>::kCap;
    __shared__ int s_rows[kTrsmWaves][kCap];
    __shared__ V s_l[kTrsmWaves][kCap];
    __shared__ V s_acc[kTrsmWaves][kCap];

    const int lane = threadIdx.x & (kWave - 1);
    const int slot = threadIdx.x / kWave;
    const int wg = (int)(blockIdx.x % (unsigned)P.wgc);
    const int cls = wg * kTrsmWaves + slot;
    const int ncls = P.wgc * kTrsmWaves;
    const I* ptr = static_cast<const I*>(P.ptr);
    const I* idx = static_cast<const I*>(P.idx);
    const I* perm = static_cast<const I*>(P.perm);
    const V* val = static_cast<const V*>(P.val);
    Bits* sig = static_cast<Bits*>(P.sig);
    Bits* out = static_cast<Bits*>(P.out);
    SelinvWork* work = P.work;
    unsigned int* done = reinterpret_cast<unsigned int*>(work + 1);
    unsigned long long* const counter = &work->class_ticket[(slot * 64 + wg) * kTicketStride];
    // (rows are staged as 32-bit words: a matrix with more rows than that works in place)
    const int64_t cap = P.n > 0x7fffffffLL ? 0 : kCap;

    for (;;) {
        const unsigned long long t = (unsigned long long)wave_uniform((int64_t)next_row_ticket(counter, lane, ncls, cls));
        if (t >= (unsigned long long)P.n) break;
        const int64_t i = P.n - 1 - (int64_t)t;              // tickets ascend, columns descend
        int64_t s = wave_uniform((int64_t)ptr[i]);
        int64_t e = wave_uniform((int64_t)ptr[i + 1]);
        if (s < 0) s = 0;
        if (e > P.nnz) e = P.nnz;
        if (e < s) e = s;
        // the diagonal's place, the pivot and the first sub-diagonal position p0
        int64_t dp = -1, p0 = s;
        V pivot = 0;
        if constexpr (LDLT) {
            pivot = static_cast<const V*>(P.D)[i];
        } else {
            dp = wave_uniform((int64_t) static_cast<const I*>(P.diag_pos)[i]);
            if (dp < s || dp >= e) dp = -1;                  // (the arrays name none: the column is finished as a broken one)
            p0 = dp >= 0 ? dp + 1 : e;
            if (dp >= 0) pivot = val[value_pos(perm, dp, P.nnz)];
        }
        const bool pivot_ok = pivot != (V)0 && pivot - pivot == (V)0;     // neither zero nor infinite nor NaN
        const int64_t m = e - p0;
        V sii;
        bool alive;
        if (m <= cap) {
            for (int64_t a = lane; a < m; a += kWave) {
                s_rows[slot][a] = (int)idx[p0 + a];
                s_l[slot][a] = val[value_pos(perm, p0 + a, P.nnz)];
            }
            const LdsCol<V> c{s_rows[slot], s_l[slot], s_acc[slot]};
            c.pass_done();
            alive = selinv_column<V, I, LDLT>(c, i, m, pivot, pivot_ok, P, done, lane, sii);
            if (alive) {
                for (int64_t a = lane; a < m; a += kWave) {
                    const Bits z = S::bits(s_acc[slot][a]);
                    __hip_atomic_store(sig + p0 + a, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    out[value_pos(perm, p0 + a, P.nnz)] = z;
                }
            }
        } else {
            const GlobalCol<V, I> c{idx + p0, perm, val, sig + p0, p0, P.nnz};
            alive = selinv_column<V, I, LDLT>(c, i, m, pivot, pivot_ok, P, done, lane, sii);
            if (alive) {
                for (int64_t a = lane; a < m; a += kWave) out[value_pos(perm, p0 + a, P.nnz)] = S::bits(c.get(a));
            }
        }
        if (!alive) {
            __hip_atomic_store(&work->error, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        // the diagonal: every lane holds the same value and stores it to the same word
        if constexpr (LDLT) {
            __hip_atomic_store(static_cast<Bits*>(P.diag_out) + i, S::bits(sii), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (dp >= 0) {
            __hip_atomic_store(sig + dp, S::bits(sii), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            out[value_pos(perm, dp, P.nnz)] = S::bits(sii);
        }
        // publish as ilu_impl.h does: the stores have reached the L2, then ONE wave-wide store of the flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(done + i, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// info[0] = 1 + the lowest column with a zero / non-finite pivot, info[1] = 1 + the lowest column with a lookup that missed; 0: none
__global__ void selinv_info_kernel(const SelinvWork* work, int64_t* info) {
    const unsigned long long b = work->bad, o = work->open;
    info[0] = b ? (int64_t)(~b) + 1 : 0;
    info[1] = o ? (int64_t)(~o) + 1 : 0;
}

}  // namespace tsgu
