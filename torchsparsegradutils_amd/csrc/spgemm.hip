// Sparse × sparse products: instantiations (fp32, fp64, bf16 × int32, int64 × four bins) and the extern "C" entry points of
// include/tsgu_hip_spgemm.h.
#include "spgemm_impl.h"

#include "../../include/tsgu_hip_spgemm.h"

using namespace tsgu;

namespace {

constexpr int64_t kI31 = 0x7fffffffLL;

bool index_type(int itype) { return itype == TSGU_I32 || itype == TSGU_I64; }
bool value_type(int vtype) { return vtype == TSGU_F32 || vtype == TSGU_F64 || vtype == TSGU_BF16; }

int shape_check(int64_t n_rows, int64_t n_inner, int64_t n_cols) {
    if (n_rows < 0 || n_inner < 0 || n_cols < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows > kI31 || n_inner > kI31 || n_cols >= kI31) return TSGU_ERR_TOO_LARGE;      // (the sort's sentinel is 2^31 - 1)
    return TSGU_OK;
}

bool any_null(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if (!q) return true;
    return false;
}

int64_t blocks_for(int64_t n, int per_block) { return (n + per_block - 1) / per_block; }

}  // namespace

extern "C" {

int tsgu_spgemm_bins(int* limits, int* lanes) {
    if (!limits || !lanes) return TSGU_ERR_BAD_ARG;
    for (int b = 0; b < 3; ++b) limits[b] = kSpgemmLimit[b];
    for (int b = 0; b < kSpgemmBins; ++b) lanes[b] = kSpgemmGroup[b];
    return TSGU_OK;
}

int tsgu_spgemm_row_bound(int itype, int64_t n_rows, int64_t n_inner, const void* a_ptr, const void* a_idx, const void* b_ptr,
                          int64_t* ub, int device, void* stream) {
    if (!index_type(itype)) return TSGU_ERR_BAD_DTYPE;
    if (const int rc = shape_check(n_rows, n_inner, 0)) return rc;
    if (n_rows == 0) return TSGU_OK;
    if (any_null({a_ptr, b_ptr, ub})) return TSGU_ERR_BAD_ARG;      // (a_idx may be NULL for a pattern without entries)
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_index_type(itype, [&](auto i) {
        using I = decltype(i);
        return launch(spgemm_row_bound_kernel<I>, blocks_for(n_rows, kBlock), s, n_rows, n_inner, static_cast<const I*>(a_ptr),
                      static_cast<const I*>(a_idx), static_cast<const I*>(b_ptr), ub);
    });
}

int tsgu_spgemm_symbolic(int itype, int bin, int64_t n_bin, const int* rows, int64_t n_rows, int64_t n_inner, int64_t n_cols,
                         const void* a_ptr, const void* a_idx, const void* b_ptr, const void* b_idx, int* scratch,
                         const int64_t* sptr, int fill, int64_t* cnt, const void* c_ptr, void* c_idx, int device, void* stream) {
    if (!index_type(itype)) return TSGU_ERR_BAD_DTYPE;
    if (bin < 0 || bin >= kSpgemmBins || n_bin < 0 || n_bin > n_rows || (fill != 0 && fill != 1)) return TSGU_ERR_BAD_ARG;
    if (const int rc = shape_check(n_rows, n_inner, n_cols)) return rc;
    if (n_bin == 0) return TSGU_OK;
    // a row in a bin has ub >= 1: both patterns have entries
    if (any_null({rows, a_ptr, a_idx, b_ptr, b_idx})) return TSGU_ERR_BAD_ARG;
    if (bin == kSpgemmBins - 1 && any_null({scratch, sptr})) return TSGU_ERR_BAD_ARG;
    if (fill ? any_null({c_ptr, c_idx}) : !cnt) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SpgemmParams P{};
    P.n_bin = n_bin, P.rows = rows, P.n_rows = n_rows, P.n_inner = n_inner, P.n_cols = n_cols;
    P.a_ptr = a_ptr, P.a_idx = a_idx, P.b_ptr = b_ptr, P.b_idx = b_idx;
    P.scratch = scratch, P.sptr = sptr, P.fill = fill, P.cnt = cnt, P.c_ptr = const_cast<void*>(c_ptr), P.c_idx = c_idx;
    return with_index_type(itype, [&](auto i) {
        using I = decltype(i);
        return spgemm_dispatch_bin(bin, [&](auto group, auto cap, auto global) {
            constexpr int GROUP = decltype(group)::value, CAP = decltype(cap)::value;
            constexpr bool GLOBAL = decltype(global)::value;
            const int64_t blocks = blocks_for(n_bin, kBlock / GROUP);
            if (blocks > kI31) return (int)TSGU_ERR_TOO_LARGE;
            return launch(spgemm_symbolic_kernel<I, GROUP, CAP, GLOBAL>, blocks, s, P);
        });
    });
}

int tsgu_spgemm_numeric(int vtype, int itype, int bin, int64_t n_bin, const int* rows, int64_t n_rows, int64_t n_inner,
                        int64_t n_cols, const void* a_ptr, const void* a_idx, const void* a_val, const void* b_ptr,
                        const void* b_idx, const void* b_val, const void* c_ptr, const void* c_idx, void* acc, void* c_val,
                        int device, void* stream) {
    if (!value_type(vtype) || !index_type(itype)) return TSGU_ERR_BAD_DTYPE;
    if (bin < 0 || bin >= kSpgemmBins || n_bin < 0 || n_bin > n_rows) return TSGU_ERR_BAD_ARG;
    if (const int rc = shape_check(n_rows, n_inner, n_cols)) return rc;
    if (n_bin == 0) return TSGU_OK;
    if (any_null({rows, a_ptr, a_idx, a_val, b_ptr, b_idx, b_val, c_ptr, c_idx, c_val})) return TSGU_ERR_BAD_ARG;
    if (bin == kSpgemmBins - 1 && !acc) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SpgemmParams P{};
    P.n_bin = n_bin, P.rows = rows, P.n_rows = n_rows, P.n_inner = n_inner, P.n_cols = n_cols;
    P.a_ptr = a_ptr, P.a_idx = a_idx, P.a_val = a_val, P.b_ptr = b_ptr, P.b_idx = b_idx, P.b_val = b_val;
    P.c_ptr = const_cast<void*>(c_ptr), P.c_idx = const_cast<void*>(c_idx), P.c_val = c_val, P.acc = acc;
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        return spgemm_dispatch_bin(bin, [&](auto group, auto cap, auto global) {
            constexpr int GROUP = decltype(group)::value, CAP = decltype(cap)::value;
            constexpr bool GLOBAL = decltype(global)::value;
            const int64_t blocks = blocks_for(n_bin, kBlock / GROUP);
            if (blocks > kI31) return (int)TSGU_ERR_TOO_LARGE;
            return launch(spgemm_numeric_kernel<V, I, GROUP, CAP, GLOBAL>, blocks, s, P);
        });
    });
}

int tsgu_spgemm_grad_a(int vtype, int itype, int64_t n_rows, int64_t n_inner, int64_t n_cols, int64_t nnz_a, const void* a_row,
                       const void* a_idx, const void* b_ptr, const void* b_idx, const void* b_val, const void* c_ptr,
                       const void* c_idx, const void* g, void* grad_a, int device, void* stream) {
    if (!value_type(vtype) || !index_type(itype)) return TSGU_ERR_BAD_DTYPE;
    if (nnz_a < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = shape_check(n_rows, n_inner, n_cols)) return rc;
    if (nnz_a == 0) return TSGU_OK;
    // (b_idx, b_val, c_idx and g may be NULL: a B or a C without entries is never dereferenced)
    if (any_null({a_row, a_idx, b_ptr, c_ptr, grad_a})) return TSGU_ERR_BAD_ARG;
    const int64_t blocks = blocks_for(nnz_a, kBlock);
    if (blocks > kI31) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SpgemmGradParams P{};
    P.n_entries = nnz_a, P.n_rows = n_rows, P.n_inner = n_inner, P.n_cols = n_cols, P.row = a_row, P.idx = a_idx;
    P.w_ptr = b_ptr, P.w_idx = b_idx, P.w_val = b_val, P.c_ptr = c_ptr, P.c_idx = c_idx, P.g = g, P.out = grad_a;
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        return launch(spgemm_grad_a_kernel<decltype(v), decltype(i)>, blocks, s, P);
    });
}

int tsgu_spgemm_grad_b(int vtype, int itype, int64_t n_rows, int64_t n_inner, int64_t n_cols, int64_t nnz_b, const void* b_row,
                       const void* b_idx, const void* t_ptr, const void* t_idx, const void* t_perm, const void* a_val,
                       const void* c_ptr, const void* c_idx, const void* g, void* grad_b, int device, void* stream) {
    if (!value_type(vtype) || !index_type(itype)) return TSGU_ERR_BAD_DTYPE;
    if (nnz_b < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = shape_check(n_rows, n_inner, n_cols)) return rc;
    if (nnz_b == 0) return TSGU_OK;
    // (t_idx, t_perm, a_val, c_idx and g may be NULL: an A or a C without entries is never dereferenced)
    if (any_null({b_row, b_idx, t_ptr, c_ptr, grad_b})) return TSGU_ERR_BAD_ARG;
    const int64_t blocks = blocks_for(nnz_b, kBlock);
    if (blocks > kI31) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    SpgemmGradParams P{};
    P.n_entries = nnz_b, P.n_rows = n_rows, P.n_inner = n_inner, P.n_cols = n_cols, P.row = b_row, P.idx = b_idx;
    P.w_ptr = t_ptr, P.w_idx = t_idx, P.w_perm = t_perm, P.w_val = a_val, P.c_ptr = c_ptr, P.c_idx = c_idx, P.g = g, P.out = grad_b;
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        return launch(spgemm_grad_b_kernel<decltype(v), decltype(i)>, blocks, s, P);
    });
}

}  // extern "C"
