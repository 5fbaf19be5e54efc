// Entry points of the aggregation multigrid kernels (tsgu_hip_amg.h; kernels: amg_impl.h).
#include "amg_impl.h"

#include "tsgu_hip_amg.h"

namespace tsgu {

inline bool amg_aligned(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte
inline bool amg_ranges_meet(const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return na && nb && x < y + nb && y < x + na;
}

// bytes from the first to one past the last element of a row-major [rows][p] view
inline uint64_t amg_span(int64_t rows, int64_t p, int64_t ld, size_t es) {
    return rows > 0 && p > 0 ? ((uint64_t)(rows - 1) * (uint64_t)ld + (uint64_t)p) * es : 0;
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_amg_geometry(int* min_group, int* max_group, int* column_tile) {
    if (!min_group || !max_group || !column_tile) return TSGU_ERR_BAD_ARG;
    *min_group = kAmgGroupMin;
    *max_group = kAmgGroupMax;
    *column_tile = kAmgColumnTile;
    return TSGU_OK;
}

int tsgu_csr_amg_hop(int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* in, void* out, int group,
                     int device, void* stream) {
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n < 0 || nnz < 0) return TSGU_ERR_BAD_ARG;
    if (group < kAmgGroupMin || group > kAmgGroupMax || (group & (group - 1))) return TSGU_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (n == 0) return TSGU_OK;
    const size_t is = itype == TSGU_I32 ? 4 : 8;
    if (!ptr || !in || !out || (!idx && nnz > 0)) return TSGU_ERR_BAD_ARG;
    if (!amg_aligned(ptr, is) || !amg_aligned(idx, is) || !amg_aligned(in, 8) || !amg_aligned(out, 8)) return TSGU_ERR_BAD_ARG;
    if (amg_ranges_meet(in, (uint64_t)n * 8, out, (uint64_t)n * 8)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    AmgHopParams P{};
    P.n = n;
    P.nnz = nnz;
    P.ptr = ptr;
    P.idx = idx;
    P.in = static_cast<const unsigned long long*>(in);
    P.out = static_cast<unsigned long long*>(out);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_index_type(itype, [&](auto i) {
        using I = decltype(i);
        int rc = TSGU_ERR_BAD_ARG;
        dispatch_pow2<kAmgGroupMin, kAmgGroupMax>(group, [&](auto w) {
            constexpr int W = decltype(w)::value;
            const int64_t rows = kBlock / W;
            rc = launch(amg_hop_kernel<I, W>, (n + rows - 1) / rows, s, P);
        });
        return rc;
    });
}

int tsgu_amg_mis2_update(int mode, int64_t n, const void* key, const void* t, void* out, void* undecided, int device, void* stream) {
    if (mode < 0 || mode > 2 || n < 0) return TSGU_ERR_BAD_ARG;
    if (n > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (n == 0) return TSGU_OK;
    if (!out || !amg_aligned(out, 8)) return TSGU_ERR_BAD_ARG;
    if (mode >= 1 && (!key || !amg_aligned(key, 8))) return TSGU_ERR_BAD_ARG;
    if (mode == 1 && (!t || !undecided || !amg_aligned(t, 8) || !amg_aligned(undecided, 8))) return TSGU_ERR_BAD_ARG;
    if (mode == 1 && amg_ranges_meet(t, (uint64_t)n * 8, out, (uint64_t)n * 8)) return TSGU_ERR_BAD_ARG;
    if (mode >= 1 && key != out && amg_ranges_meet(key, (uint64_t)n * 8, out, (uint64_t)n * 8)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    return launch(amg_mis2_kernel, (n + kBlock - 1) / kBlock, static_cast<hipStream_t>(stream), mode, n,
                  static_cast<const unsigned long long*>(key), static_cast<const unsigned long long*>(t),
                  static_cast<unsigned long long*>(out), static_cast<unsigned long long*>(undecided));
}

int tsgu_csr_affine_spmm(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t p, const void* ptr, const void* idx,
                         const void* val, const void* x, int64_t ldx, const void* c, int64_t ldc, const void* b, int64_t ldb,
                         const void* w, double alpha, void* out, int64_t ldo, int device, void* stream) {
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;     // (bf16 included)
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || p < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows > 0x7fffffffLL * (kBlock / kAmgGroup)) return TSGU_ERR_TOO_LARGE;
    if (n_rows == 0 || p == 0) return TSGU_OK;
    const size_t es = vtype == TSGU_F32 ? 4 : 8, is = itype == TSGU_I32 ? 4 : 8;
    if (!ptr || !out || ((!idx || !val) && nnz > 0) || (!x && nnz > 0 && n_cols > 0)) return TSGU_ERR_BAD_ARG;
    if (!amg_aligned(ptr, is) || !amg_aligned(idx, is)) return TSGU_ERR_BAD_ARG;
    for (const void* q : {val, x, c, b, w, static_cast<const void*>(out)})
        if (!amg_aligned(q, es)) return TSGU_ERR_BAD_ARG;
    if (ldx < p || ldo < p || (c && ldc < p) || (b && ldb < p)) return TSGU_ERR_BAD_ARG;
    const uint64_t out_bytes = amg_span(n_rows, p, ldo, es);
    if (x && amg_ranges_meet(out, out_bytes, x, amg_span(n_cols, p, ldx, es))) return TSGU_ERR_BAD_ARG;
    if (c && !(c == out && ldc == ldo) && amg_ranges_meet(out, out_bytes, c, amg_span(n_rows, p, ldc, es))) return TSGU_ERR_BAD_ARG;
    if (b && !(b == out && ldb == ldo) && amg_ranges_meet(out, out_bytes, b, amg_span(n_rows, p, ldb, es))) return TSGU_ERR_BAD_ARG;
    if (w && amg_ranges_meet(out, out_bytes, w, (uint64_t)n_rows * es)) return TSGU_ERR_BAD_ARG;
    const int cl = p >= kAmgColumnTile ? kAmgColumnTile : next_pow2(p);
    const int64_t tiles = (p + cl - 1) / cl;
    if (tiles > 65535) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    AmgAffineParams P{};
    P.n_rows = n_rows;
    P.n_cols = n_cols;
    P.nnz = nnz;
    P.p = p;
    P.ptr = ptr;
    P.idx = idx;
    P.val = val;
    P.x = x;
    P.c = c;
    P.b = b;
    P.w = w;
    P.out = out;
    P.ldx = ldx;
    P.ldc = ldc;
    P.ldb = ldb;
    P.ldo = ldo;
    P.alpha = alpha;
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr int64_t rows = kBlock / kAmgGroup;
    const dim3 grid((unsigned)((n_rows + rows - 1) / rows), (unsigned)tiles);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        dispatch_pow2<1, kAmgColumnTile>(cl, [&](auto k) {
            hipLaunchKernelGGL((amg_affine_kernel<V, I, decltype(k)::value>), grid, dim3(kBlock), 0, s, P);
        });
        return check_launch();
    });
}

}  // extern "C"
