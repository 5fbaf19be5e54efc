// Shared pieces of the Krylov kernels (CG in krylov.hip, BiCGSTAB in bicgstab.hip, MINRES in minres.hip): lane layout for
// contiguous [n][p] arrays, deterministic block-level column sums, the partial-row fold kernel, and the host launch helpers
// every entry point of the three files is written on.  From tsgu_common.h, shared with every other kernel family:
//   with_value_type(vtype, f)        calls the generic lambda f with a float or a double tag (`using V = decltype(tag)`)
//   launch(kern, blocks, s, args...) one kernel on `blocks` workgroups of kBlock threads, then check_launch()
// and here, host side:
//   launch_lanes<V>(n, p, scalar, wide, go)   geometry of an [n][p] array, then go(instance, geometry) with the scalar-lane or
//                                    the wide-lane instance of a kernel — its argument list is written once, in `go`
//   fold_partials<V>(...)            the fold-then-finalise prefix of the single-workgroup scalar kernels
// device side (what the streaming kernels of the three files are written on):
//   lanes<VEC>(p, lpr, rpp)          a thread's place in the lane layout: its columns, its row slot, the workgroup's first row
//   for_rows<NP>(L, n, f)            f(pass, row) for the rows the thread owns, NP passes unrolled (bicg_update_x_kernel keeps a
//                                    loop of its own, see there)
//   fold_partial_row<V, VEC>(...)    the workgroup's partial row: every lane's accumulators summed per column in a fixed order
//   block_colsum<Acc>(...)           the sum of partial rows over a 64-column window, by one workgroup, in a fixed order
#pragma once

#include "tsgu_common.h"

namespace tsgu {

constexpr int kPasses = 4;  // row passes per block in the elementwise kernels

// Lane layout for a contiguous [n][p] array: lpr lanes per row, each VEC columns wide.
struct VecGeom {
    int vec;
    int lpr;  // lanes per row = ceil(p / vec)
    int rpp;  // rows per pass = 256 / lpr
    int64_t blocks;
};

inline bool vec_geom(int wide, bool can_wide, int64_t n, int64_t p, VecGeom& g) {
    g.vec = can_wide ? wide : 1;
    const int64_t lpr = (p + g.vec - 1) / g.vec;
    if (lpr > kBlock) return false;
    g.lpr = (int)lpr;
    g.rpp = kBlock / g.lpr;
    const int64_t rows_per_block = (int64_t)g.rpp * kPasses;
    g.blocks = (n + rows_per_block - 1) / rows_per_block;
    return true;
}

// A thread's place in that layout: thread t is lane cl of row slot rs, holds columns [c, c + VEC) and, in pass ps, row
// r0 + ps * rpp + rs of the workgroup's rpp * kPasses (* groups) rows.  `on`: the thread has a row slot and columns (lpr need not
// divide kBlock, and the slots past rpp are idle).
struct Lanes {
    int lpr, rpp;
    int cl, rs;
    int64_t c;
    bool on;
    int64_t r0;
};

template <int VEC>
__device__ __forceinline__ Lanes lanes(int64_t p, int lpr, int rpp, int groups = 1) {
    const int t = threadIdx.x;
    Lanes L;
    L.lpr = lpr;
    L.rpp = rpp;
    L.cl = t % lpr;
    L.rs = t / lpr;
    L.c = (int64_t)L.cl * VEC;
    L.on = L.rs < rpp && L.c < p;
    L.r0 = (int64_t)blockIdx.x * rpp * kPasses * groups;
    return L;
}

// f(ps, row) for the rows below n that the thread owns in passes ps0 ... ps0 + NP - 1 (f sees ps = 0 ... NP - 1: the index of
// what a kernel keeps in registers between two walks).  Fully unrolled.  f must not hold a barrier: lanes skip rows.
template <int NP = kPasses, typename F>
__device__ __forceinline__ void for_rows(const Lanes& L, int64_t n, F&& f, int ps0 = 0) {
#pragma unroll
    for (int ps = 0; ps < NP; ++ps) {
        const int64_t row = L.r0 + (int64_t)(ps0 + ps) * L.rpp + L.rs;
        if (L.on && row < n) f(ps, row);
    }
}

// The workgroup's partial row: dst[cc] = the sum over the row slots k = 0 ... rpp - 1, in that order, of the accumulator lane
// (k, cc) holds for column cc.  No atomics and a fixed order: what makes every reduction of these solvers deterministic.
// red: LDS scratch of kBlock * VEC values; one barrier between the writes and the sums, none after the sums (a caller that
// writes `red` again puts one there); called by every thread of the workgroup.
template <typename V, int VEC>
__device__ __forceinline__ void fold_partial_row(V* red, const V (&acc)[VEC], const Lanes& L, int64_t p, V* __restrict__ dst) {
    const int lpr = L.lpr, rpp = L.rpp, cl = L.cl, rs = L.rs;
    if (rs < rpp) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) red[(rs * lpr + cl) * VEC + v] = acc[v];
    }
    __syncthreads();
    for (int64_t cc = threadIdx.x; cc < p; cc += kBlock) {
        V s = 0;
        for (int k = 0; k < rpp; ++k) s += red[k * lpr * VEC + cc];
        dst[cc] = s;
    }
}

// Sum partial[b][c] over b for the calling block's column window [c0, c0+w): result valid
// in threads t < w (thread t owns column c0+t).  red: LDS scratch of kBlock Acc.
template <typename Acc>
__device__ __forceinline__ Acc block_colsum(const Acc* __restrict__ partial, int64_t n_partial, int64_t p,
                                            int64_t c0, int w, Acc* red) {
    const int t = threadIdx.x;
    const int subs = kBlock / w;
    const int sub = t / w, lc = t % w;
    Acc s = 0;
    if (sub < subs) {
        // four independent chains keep four loads in flight per thread (fixed order => deterministic)
        Acc s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int64_t b = sub;
        for (; b + 3 * (int64_t)subs < n_partial; b += 4 * (int64_t)subs) {
            s0 += partial[b * p + c0 + lc];
            s1 += partial[(b + subs) * p + c0 + lc];
            s2 += partial[(b + 2 * (int64_t)subs) * p + c0 + lc];
            s3 += partial[(b + 3 * (int64_t)subs) * p + c0 + lc];
        }
        for (; b < n_partial; b += subs) s0 += partial[b * p + c0 + lc];
        s = (s0 + s1) + (s2 + s3);
    }
    red[t] = s;
    __syncthreads();
    Acc tot = 0;
    if (t < w) {
        for (int k = 0; k < subs; ++k) tot += red[k * w + t];
    }
    __syncthreads();
    return tot;
}

// First level of a three-stage column sum: `rows` partial rows -> kFoldRows rows (block b sums the
// contiguous slice of rows [b*chunk, (b+1)*chunk) in row order).  Keeps the single-block finalisers
// (which need all columns at once) short when a kernel produced tens of thousands of partials.
constexpr int kFoldRows = 256;

template <typename V>
__global__ __launch_bounds__(kBlock) void colsum_fold_kernel(const V* __restrict__ partial, int64_t rows, int64_t p,
                                                             int64_t chunk, V* __restrict__ out, const int* __restrict__ flags) {
    __shared__ V red[kBlock];
    if (flags && flags[0] != 0) return;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    int64_t r1 = r0 + chunk;
    r1 = r1 < rows ? r1 : rows;
    for (int64_t c0 = 0; c0 < p; c0 += 64) {
        const int w = (int)(p - c0 < 64 ? p - c0 : 64);
        const V tot = r0 < r1 ? block_colsum<V>(partial + r0 * p, r1 - r0, p, c0, w, red) : (V)0;
        if ((int)threadIdx.x < w) out[(int64_t)blockIdx.x * p + c0 + threadIdx.x] = tot;
    }
}

template <typename V>
inline bool geom_for(int64_t n, int64_t p, bool aligned, VecGeom& g) {
    constexpr int wide = VT<V>::kWide;
    return vec_geom(wide, aligned && (p % wide == 0), n, p, g);
}

// ---- host side -----------------------------------------------------------------------
// The streaming kernels exist in two instances of one signature, <V, 1> (scalar lanes) and <V, VT<V>::kWide> (16-byte lanes;
// needs 16-byte aligned operands — `aligned` — and p a multiple of the width).  `go(kern, g)` receives the instance that fits
// and the geometry and launches it: on g.blocks workgroups with g.lpr, g.rpp wherever the kernel wants them, or on a grid of
// its own derived from g.
template <typename V, typename Kern, typename Go>
inline int launch_lanes(int64_t n, int64_t p, Kern* scalar, Kern* wide, Go&& go, bool aligned = true) {
    VecGeom g;
    if (!geom_for<V>(n, p, aligned, g)) return TSGU_ERR_TOO_LARGE;
    return go(g.vec == 1 ? scalar : wide, g);
}

// Very many partial rows (the K1 epilogue writes one per workgroup) are folded to kFoldRows rows before a single-workgroup
// finaliser sums them: needs the caller's `fold` buffer and is done when `wanted` and there are more than 4 * kFoldRows rows.
// `fold_flags`: the stop word the fold kernel honours (NULL: always runs).  Leaves the rows to finalise in (src, rows).
template <typename V>
inline int fold_partials(const void* partial, int64_t n_partial, int64_t p, void* fold, bool wanted, const int* fold_flags,
                         hipStream_t s, const V*& src, int64_t& rows) {
    src = (const V*)partial;
    rows = n_partial;
    if (!(fold != nullptr && wanted && n_partial > 4 * kFoldRows)) return TSGU_OK;
    const int64_t chunk = (n_partial + kFoldRows - 1) / kFoldRows;
    if (const int rc = launch(colsum_fold_kernel<V>, kFoldRows, s, src, n_partial, p, chunk, (V*)fold, fold_flags)) return rc;
    src = (const V*)fold;
    rows = kFoldRows;
    return TSGU_OK;
}

}  // namespace tsgu
