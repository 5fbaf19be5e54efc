// Entry points of the multicolour ordering kernels (tsgu_hip_color.h; kernels: color_impl.h).
#include "color_impl.h"

#include "tsgu_hip_color.h"

namespace tsgu {

inline bool color_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool color_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

// bytes from the first to one past the last element of a row-major [rows][p] view
inline uint64_t color_span(int64_t rows, int64_t p, int64_t ld, size_t es) {
    return rows > 0 && p > 0 ? ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)p) * es : 0;
}

// the checks the round and the check share; TSGU_OK with `go` false when there is nothing to do
inline int color_pattern_args(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, int64_t nnz_t, const void* tptr,
                              const void* tidx, const void* colors, int group) {
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n < 0 || nnz < 0 || nnz_t < 0) return TSGU_ERR_BAD_ARG;
    if (group < kAmgGroupMin || group > kAmgGroupMax || (group & (group - 1))) return TSGU_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (n == 0) return TSGU_OK;
    const size_t is = itype == TSGU_I32 ? 4 : 8;
    if (!ptr || !colors || (!idx && nnz > 0)) return TSGU_ERR_BAD_ARG;
    if (!tptr && (tidx || nnz_t > 0)) return TSGU_ERR_BAD_ARG;
    if (tptr && !tidx && nnz_t > 0) return TSGU_ERR_BAD_ARG;
    if (!color_aligned(ptr, is) || !color_aligned(idx, is) || !color_aligned(tptr, is) || !color_aligned(tidx, is) ||
        !color_aligned(colors, 4))
        return TSGU_ERR_BAD_ARG;
    return TSGU_OK;
}

template <template <typename, int> class Launcher>
inline int color_dispatch(int itype, int group, int64_t n, hipStream_t s, const ColorParams& P) {
    return with_index_type(itype, [&](auto i) {
        using I = decltype(i);
        int rc = TSGU_ERR_BAD_ARG;
        dispatch_pow2<kAmgGroupMin, kAmgGroupMax>(group, [&](auto w) {
            constexpr int W = decltype(w)::value;
            const int64_t rows = kBlock / W;
            rc = Launcher<I, W>::run((n + rows - 1) / rows, s, P);
        });
        return rc;
    });
}

template <typename I, int W>
struct RoundLauncher {
    static int run(int64_t blocks, hipStream_t s, const ColorParams& P) { return launch(color_round_kernel<I, W>, blocks, s, P); }
};
template <typename I, int W>
struct CheckLauncher {
    static int run(int64_t blocks, hipStream_t s, const ColorParams& P) { return launch(color_check_kernel<I, W>, blocks, s, P); }
};

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_color_geometry(int* min_group, int* max_group, int* window, int* sweep_min_group, int* sweep_max_group, int* column_tile) {
    if (!min_group || !max_group || !window || !sweep_min_group || !sweep_max_group || !column_tile) return TSGU_ERR_BAD_ARG;
    *min_group = kAmgGroupMin;
    *max_group = kAmgGroupMax;
    *window = kColorWindow;
    *sweep_min_group = kSweepGroupMin;
    *sweep_max_group = kSweepGroupMax;
    *column_tile = kAmgColumnTile;
    return TSGU_OK;
}

int tsgu_csr_color_round(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, int64_t nnz_t, const void* tptr,
                         const void* tidx, const void* in, void* out, void* undecided, int group, int device, void* stream) {
    if (const int rc = color_pattern_args(itype, n, nnz, ptr, idx, nnz_t, tptr, tidx, in, group)) return rc;
    if (n == 0) return TSGU_OK;
    if (!out || !undecided || !color_aligned(out, 4) || !color_aligned(undecided, 8)) return TSGU_ERR_BAD_ARG;
    if (color_ranges_meet(in, (uint64_t)n * 4, out, (uint64_t)n * 4)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    ColorParams P{};
    P.n = n;
    P.nnz = nnz;
    P.nnz_t = nnz_t;
    P.ptr = ptr;
    P.idx = idx;
    P.tptr = tptr;
    P.tidx = tidx;
    P.in = static_cast<const int*>(in);
    P.out = static_cast<int*>(out);
    P.word = static_cast<unsigned long long*>(undecided);
    return color_dispatch<RoundLauncher>(itype, group, n, static_cast<hipStream_t>(stream), P);
}

int tsgu_csr_color_check(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, int64_t nnz_t, const void* tptr,
                         const void* tidx, const void* colors, int64_t n_colors, void* first, int group, int device, void* stream) {
    if (!first || !color_aligned(first, 8) || n_colors < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = color_pattern_args(itype, n, nnz, ptr, idx, nnz_t, tptr, tidx, n > 0 ? colors : first, group)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(first, n > 0 ? 0xff : 0, 8, s) != hipSuccess) return TSGU_ERR_RUNTIME;
    if (n == 0) return TSGU_OK;
    ColorParams P{};
    P.n = n;
    P.nnz = nnz;
    P.nnz_t = nnz_t;
    P.n_colors = n_colors;
    P.ptr = ptr;
    P.idx = idx;
    P.tptr = tptr;
    P.tidx = tidx;
    P.in = static_cast<const int*>(colors);
    P.word = static_cast<unsigned long long*>(first);
    if (const int rc = color_dispatch<CheckLauncher>(itype, group, n, s, P)) return rc;
    hipLaunchKernelGGL(color_check_finish_kernel, dim3(1), dim3(kWave), 0, s, P.word);
    return check_launch();
}

int tsgu_csr_color_sweep(int vtype, int itype, int mode, int64_t n, int64_t nnz, int64_t n_val, int64_t row0, int64_t row1, int64_t p,
                         const void* begin, const void* end, const void* idx, const void* diag, const void* vmap, const void* val,
                         const void* b, int64_t ldb, const void* bmap, void* x, int64_t ldx, void* out, int64_t ldo,
                         const void* out_rows, int group, int device, void* stream) {
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;     // (bf16 included)
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (mode != kSweepDivide && mode != kSweepUnit && mode != kSweepScaled) return TSGU_ERR_BAD_ARG;
    if (n < 0 || nnz < 0 || n_val < 0 || p < 0 || row0 < 0 || row1 < row0 || row1 > n) return TSGU_ERR_BAD_ARG;
    if (group < kSweepGroupMin || group > kSweepGroupMax || (group & (group - 1))) return TSGU_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (row0 == row1 || p == 0) return TSGU_OK;
    const size_t es = vtype == TSGU_F32 ? 4 : 8, is = itype == TSGU_I32 ? 4 : 8;
    if (!begin || !end || !b || !x || ((!idx || !val) && nnz > 0) || (mode != kSweepUnit && (!diag || !val))) return TSGU_ERR_BAD_ARG;
    if (out_rows && !out) return TSGU_ERR_BAD_ARG;
    for (const void* q : {begin, end, idx, diag, vmap, bmap, out_rows})
        if (!color_aligned(q, is)) return TSGU_ERR_BAD_ARG;
    for (const void* q : {val, b, static_cast<const void*>(x), static_cast<const void*>(out)})
        if (!color_aligned(q, es)) return TSGU_ERR_BAD_ARG;
    if (ldb < p || ldx < p || (out && ldo < p)) return TSGU_ERR_BAD_ARG;
    const uint64_t x_bytes = color_span(n, p, ldx, es);
    if (!(b == x && ldb == ldx && !bmap) && color_ranges_meet(x, x_bytes, b, color_span(n, p, ldb, es))) return TSGU_ERR_BAD_ARG;
    if (out && color_ranges_meet(x, x_bytes, out, color_span(n, p, ldo, es))) return TSGU_ERR_BAD_ARG;
    const int cl = p >= kAmgColumnTile ? kAmgColumnTile : next_pow2(p);
    const int64_t per_group = (int64_t)cl * (group / kAmgGroup);
    const int64_t tiles = (p + per_group - 1) / per_group;
    if (tiles > 65535) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    ColorSweepParams P{};
    P.n = n;
    P.nnz = nnz;
    P.n_val = n_val;
    P.row0 = row0;
    P.row1 = row1;
    P.p = p;
    P.begin = begin;
    P.end = end;
    P.idx = idx;
    P.diag = diag;
    P.vmap = vmap;
    P.val = val;
    P.b = b;
    P.bmap = bmap;
    P.x = x;
    P.out = out;
    P.out_rows = out_rows;
    P.ldb = ldb;
    P.ldx = ldx;
    P.ldo = ldo;
    P.mode = mode;
    P.group = group;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows = kBlock / group;
    const dim3 grid((unsigned)((row1 - row0 + rows - 1) / rows), (unsigned)tiles);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        dispatch_pow2<1, kAmgColumnTile>(cl, [&](auto k) {
            hipLaunchKernelGGL((color_sweep_kernel<V, I, decltype(k)::value>), grid, dim3(kBlock), 0, s, P);
        });
        return check_launch();
    });
}

}  // extern "C"
