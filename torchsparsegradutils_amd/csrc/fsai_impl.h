// The factorised sparse approximate inverse (include/tsgu_hip_fsai.h): one small dense SPD system per row of the pattern S.
//
// Row i of G is the last row of the inverse Cholesky factor of A[J,J], J = cols_S(i): m = |J| is a handful to a few dozen, the
// rows are independent, and the work per row is m³/6 — nothing to stream, nothing to wait for.  So the unit of work is a SUB-WAVE
// GROUP: W = 8, 16, 32 or 64 lanes own one row (m <= W), lane t owns row t of the local matrix, and a wave of 64 builds 8, 4, 2 or 1
// rows at a time.  A workgroup is ONE wave: nothing in a row is shared between waves, so there is no workgroup barrier, and eight
// such workgroups per CU (the most the entry asks for) keep their LDS images, 16.6 KiB each in fp64, resident together.
//
// Dealing: the list of rows (`order`, or 0 … n-1) is cut into chunks of kFsaiRows = 8; a workgroup takes chunks at a grid stride.
// The wave reads the eight lengths, works at the class of the longest, and needs W / 8 passes for its chunk.  With `order` sorted
// by length (the Python plan does that once per pattern) all but three chunks hold rows of one class.
//
// The local matrix is kept as its packed lower triangle in LDS, entry (t, c) at t(t+1)/2 + c: W(W+1)/2 elements per row of G,
// 32·(W+1) <= 2080 per wave in every class.  The two access shapes are conflict-free: "every lane its own row t, one column c"
// hits the banks t(t+1)/2 mod 32, a permutation of 0 … 31 over 32 consecutive t (triangular numbers modulo a power of two), and
// "row c, lanes along its columns" is contiguous; a read of row k by the whole group is a broadcast.
//
//   gather    lane t walks row j_t of tril(A) against J (both ascend: a two-pointer merge) and fills (t, b) for j_b <= j_t
//   factor    left-looking Cholesky, column k = 0 … m-1: every lane t >= k forms a_tk − Σ_{c<k} l_tc·l_kc in ascending c (row k was
//             finished in the steps before), lane k's value is the pivot and goes round by one `__shfl`, l_kk = sqrt(pivot),
//             l_tk = value / l_kk.  One LDS store per lane and step; the wave runs in lockstep, a wave-scope fence keeps the
//             compiler from moving LDS accesses across a step.
//   solve     L·z = e_m is z = e_m / l_mm, and y / sqrt(y_m) with L·Lᵀ·y = e_m is the solution of Lᵀ·g = e_m: one back substitution,
//             row c = m-1 … 0, lane c finishes g_c = (e_c − acc) / l_cc, `__shfl` hands it round, lanes t < c add l_ct·g_c.
//   store     lane t writes g_t: one coalesced vector store per group.
//
// Every sum is formed by one lane in an order that depends on the row alone (ascending c, descending c), the bounds of the loops
// are wave-uniform scalars and only predicate lanes off: the bits of a row do not depend on the class it is built at, on its
// neighbours in the wave or on the grid.  A pivot that is not positive (NaN included) never stops anything: the row is finished in
// IEEE arithmetic and recorded (`info` holds the max of ~row until fsai_info_kernel turns it into 1 + the lowest such row).
#pragma once

#include <limits>

#include "tsgu_common.h"

namespace tsgu {

constexpr int kFsaiCap = 64;                               // the longest row of S: one lane per entry
constexpr int kFsaiRows = 8;                               // rows of a chunk (= rows of a wave in the smallest class)
constexpr int kFsaiTri = (kWave / 2) * (kFsaiCap + 1);     // elements of a wave's LDS image: 32·(W + 1) at W = 64

struct FsaiParams {
    int64_t n, s_nnz, chunks;
    const void* a_ptr;
    const void* a_idx;
    const void* a_val;
    const void* s_ptr;
    const void* s_idx;
    const void* order;          // may be null
    void* out;
    unsigned long long* info;   // zeroed before the launch; max over the broken rows of ~row
};

// LDS operations of one wave complete in issue order; this only keeps the compiler from moving them across a step
__device__ __forceinline__ void fsai_step_done() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }

// The extent [s, s + len) of row `pos` of the list in S, clamped to the arrays; row = -1 when the list names none.
template <typename I>
__device__ __forceinline__ void fsai_row(const FsaiParams& P, int64_t pos, int64_t& row, int64_t& s, int64_t& len) {
    row = -1;
    s = len = 0;
    if (pos >= P.n) return;
    const I* order = static_cast<const I*>(P.order);
    const I* sptr = static_cast<const I*>(P.s_ptr);
    const int64_t r = order ? (int64_t)order[pos] : pos;
    if (r < 0 || r >= P.n) return;
    int64_t a = (int64_t)sptr[r], e = (int64_t)sptr[r + 1];
    if (a < 0) a = 0;
    if (e > P.s_nnz) e = P.s_nnz;
    if (e < a) e = a;
    row = r;
    s = a;
    len = e - a;
}

// The kWave / W rows at the list positions first, first + 1, …: one per group of W lanes.  `mcap` (wave-uniform) bounds the
// systems of this pass.
template <typename V, typename I, int W>
__device__ __forceinline__ void fsai_pass(const FsaiParams& P, int64_t first, int mcap, int lane, V* s_m, int64_t* s_j) {
    constexpr int kTri = W * (W + 1) / 2;
    constexpr int kImage = (kWave / W) * kTri;
    static_assert(kImage <= kFsaiTri, "the LDS image of a wave");
    const I* aptr = static_cast<const I*>(P.a_ptr);
    const I* aidx = static_cast<const I*>(P.a_idx);
    const V* aval = static_cast<const V*>(P.a_val);
    const I* sidx = static_cast<const I*>(P.s_idx);
    V* out = static_cast<V*>(P.out);
    const int gq = lane / W, t = lane % W;

    int64_t row, s, len;
    fsai_row<I>(P, first + gq, row, s, len);
    const bool over = len > W;                       // (only ever a row beyond the capacity: the class is that of the longest row)
    const int m = over ? 0 : (int)len;

    for (int x = lane; x < kImage; x += kWave) s_m[x] = (V)0;
    s_j[lane] = t < m ? (int64_t)sidx[s + t] : (int64_t)-1;
    fsai_step_done();

    V* M = s_m + gq * kTri;
    const int64_t* J = s_j + gq * W;
    const int tt = t * (t + 1) / 2;

    // gather: row j_t of tril(A) against J[0 … t]
    if (t < m) {
        const int64_t j = J[t];
        if (j >= 0 && j < P.n) {
            const int64_t pe = (int64_t)aptr[j + 1];
            int b = 0;
            const int64_t pa = (int64_t)aptr[j];
            for (int64_t p = pa < 0 ? 0 : pa; p < pe; ++p) {
                const int64_t c = (int64_t)aidx[p];
                while (b <= t && J[b] < c) ++b;
                if (b > t) break;
                if (J[b] == c) {
                    M[tt + b] = aval[p];
                    ++b;
                }
            }
        }
    }
    fsai_step_done();

    // factor: A[J,J] = L·Lᵀ in place, column by column
    bool broke = false;
    for (int k = 0; k < mcap; ++k) {
        const int kk = k * (k + 1) / 2;
        const bool act = t >= k && t < m;
        V sv = (V)0;
        if (act) {
            V acc = (V)0;
            for (int c = 0; c < k; ++c) {
                const V prod = M[tt + c] * M[kk + c];
                acc = acc + prod;
            }
            sv = M[tt + k] - acc;
        }
        const V piv = __shfl(sv, k, W);
        if (k < m) broke = broke || !(piv > (V)0);
        const V d = sqrt(piv);
        if (act) M[tt + k] = t == k ? d : sv / d;
        fsai_step_done();
    }

    // solve Lᵀ·g = e_m
    const V dg = t < m ? M[tt + t] : (V)1;
    V acc = (V)0, g = (V)0;
    for (int c = mcap - 1; c >= 0; --c) {
        const int cc = c * (c + 1) / 2;
        V w = (V)0;
        if (t == c && c < m) {
            const V rhs = c == m - 1 ? (V)1 : (V)0;
            w = (rhs - acc) / dg;
            g = w;
        }
        const V wc = __shfl(w, c, W);
        if (t < c && c < m) {
            const V prod = M[cc + t] * wc;
            acc = acc + prod;
        }
    }
    if (t < m) out[s + t] = g;
    if (over) {
        for (int64_t x = t; x < len; x += W) out[s + x] = std::numeric_limits<V>::quiet_NaN();
    }
    // (every lane of the group, one value: rare, and no one-lane tail in front of the caller's back edge)
    if (broke || over) __hip_atomic_fetch_max(P.info, ~(unsigned long long)row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fsai_step_done();
}

template <typename V, typename I, int W>
__device__ __forceinline__ void fsai_chunk(const FsaiParams& P, int64_t first, int mx, int lane, V* s_m, int64_t* s_j) {
    constexpr int kPer = kWave / W;
    const int mcap = mx < W ? mx : W;
    for (int p = 0; p < kFsaiRows / kPer; ++p) fsai_pass<V, I, W>(P, first + p * kPer, mcap, lane, s_m, s_j);
}

template <typename V, typename I>
__global__ __launch_bounds__(kWave) void fsai_kernel(const FsaiParams P) {
    __shared__ V s_m[kFsaiTri];
    __shared__ int64_t s_j[kWave];
    const int lane = threadIdx.x;
    for (int64_t chunk = blockIdx.x; chunk < P.chunks; chunk += gridDim.x) {
        const int64_t first = chunk * kFsaiRows;
        // the longest of the chunk's rows: lanes 0 … 7 hold one length each
        int64_t row, s, len = 0;
        if (lane < kFsaiRows) fsai_row<I>(P, first + lane, row, s, len);
        int mine = len > kFsaiCap ? kFsaiCap + 1 : (int)len;
        for (int step = 1; step < kFsaiRows; step <<= 1) {
            const int other = __shfl_xor(mine, step, kWave);
            mine = other > mine ? other : mine;
        }
        const int mx = __builtin_amdgcn_readfirstlane(mine);
        if (mx <= 8) fsai_chunk<V, I, 8>(P, first, mx, lane, s_m, s_j);
        else if (mx <= 16) fsai_chunk<V, I, 16>(P, first, mx, lane, s_m, s_j);
        else if (mx <= 32) fsai_chunk<V, I, 32>(P, first, mx, lane, s_m, s_j);
        else fsai_chunk<V, I, 64>(P, first, mx, lane, s_m, s_j);
    }
}

// info = 1 + the lowest row that broke down, 0 when none did (behind the build on its stream)
__global__ void fsai_info_kernel(unsigned long long* info) {
    const unsigned long long b = *info;
    *info = b ? ~b + 1 : 0;
}

}  // namespace tsgu
