// Density reductions of the sparse multivariate normal: instantiations (fp32, fp64 × int32, int64) and the extern "C" entry points.
#include "mvn_impl.h"

using namespace tsgu;

namespace {

inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }
inline int64_t blocks_for(int64_t threads) { return (threads + kBlock - 1) / kBlock; }

template <typename V>
int finalize(const void* partial, int64_t nb, int64_t n_out, void* out, hipStream_t s) {
    const int64_t blocks = (n_out + kBlock / kWave - 1) / (kBlock / kWave);
    if (!grid_ok(blocks)) return TSGU_ERR_TOO_LARGE;
    hipLaunchKernelGGL((mvn_finalize_kernel<V>), dim3((unsigned)blocks), dim3(kBlock), 0, s,
                       static_cast<const typename VT<V>::Acc*>(partial), nb, n_out, static_cast<V*>(out));
    return check_launch();
}

}  // namespace

extern "C" {

int64_t tsgu_mvn_reduce_blocks(int64_t rows_per_item) { return rows_per_item < 0 ? -1 : mvn_blocks(rows_per_item); }

int tsgu_csr_diag_positions(int itype, int64_t n_rows, int64_t nnz, const void* crow, const void* col, const void* perm,
                            void* pos, int device, void* stream) {
    if (n_rows < 0 || nnz < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows == 0) return TSGU_OK;
    if (!crow || !pos || (nnz > 0 && !col)) return TSGU_ERR_BAD_ARG;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    const int64_t blocks = blocks_for(n_rows);
    if (!grid_ok(blocks)) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_index_type(itype, [&](auto i) {
        using I = decltype(i);
        return launch(diag_positions_kernel<I>, blocks, s, n_rows, nnz, (const I*)crow, (const I*)col, (const I*)perm, (I*)pos);
    });
}

int tsgu_diag_logsum(int vtype, int itype, int64_t n_rows, int64_t rows_per_item, int64_t n_val, const void* pos,
                     const void* val, void* out, void* partial, int64_t partial_elems, int device, void* stream) {
    if (n_rows < 0 || rows_per_item <= 0 || n_rows % rows_per_item != 0 || n_val < 0) return TSGU_ERR_BAD_ARG;
    const int64_t items = n_rows / rows_per_item;
    if (items == 0) return TSGU_OK;
    if (!val || !out || !partial) return TSGU_ERR_BAD_ARG;
    if (!pos && n_val < n_rows) return TSGU_ERR_BAD_ARG;
    const int64_t nb = mvn_blocks(rows_per_item);
    if (partial_elems < items * nb) return TSGU_ERR_BAD_ARG;
    if (items > 65535) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        hipLaunchKernelGGL((diag_logsum_partial_kernel<V, I>), dim3((unsigned)nb, (unsigned)items), dim3(kBlock), 0, s,
                           rows_per_item, mvn_chunk(rows_per_item), n_val, static_cast<const I*>(pos),
                           static_cast<const V*>(val), static_cast<typename VT<V>::Acc*>(partial));
        if (const int rc = check_launch()) return rc;
        return finalize<V>(partial, nb, items, out, s);
    });
}

int tsgu_diag_logsum_backward(int vtype, int itype, int64_t n_rows, int64_t rows_per_item, int64_t nnz, const void* crow,
                              const void* perm, const void* pos, const void* val, const void* g, void* grad, int fill,
                              int device, void* stream) {
    if (n_rows < 0 || rows_per_item <= 0 || n_rows % rows_per_item != 0 || nnz < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows == 0) return TSGU_OK;
    if (!val || !g || !grad) return TSGU_ERR_BAD_ARG;
    if (pos && fill && !crow) return TSGU_ERR_BAD_ARG;
    if (!pos && nnz < n_rows) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        if (!pos) {      // dense vector: grad[i] = g[item] / val[i]
            const int64_t blocks = blocks_for(n_rows);
            if (!grid_ok(blocks)) return (int)TSGU_ERR_TOO_LARGE;
            hipLaunchKernelGGL((vec_logsum_bwd_kernel<V>), dim3((unsigned)blocks), dim3(kBlock), 0, s, n_rows, rows_per_item,
                               static_cast<const V*>(val), static_cast<const V*>(g), static_cast<V*>(grad));
            return check_launch();
        }
        const int64_t blocks = blocks_for(n_rows * kMvnRowLanes);
        if (!grid_ok(blocks)) return (int)TSGU_ERR_TOO_LARGE;
        hipLaunchKernelGGL((diag_logsum_bwd_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, n_rows, rows_per_item,
                           nnz, static_cast<const I*>(crow), static_cast<const I*>(perm), static_cast<const I*>(pos),
                           static_cast<const V*>(val), static_cast<const V*>(g), static_cast<V*>(grad), fill);
        return check_launch();
    });
}

int tsgu_quadform(int vtype, int64_t n, int64_t k, const void* Y, int64_t ldy, int64_t y_col_stride, const void* E,
                  int64_t lde, int64_t e_col_stride, const void* w, int w_mode, int64_t rows_per_item, void* out,
                  void* partial, int64_t partial_elems, int device, void* stream) {
    if (n < 0 || k < 0 || rows_per_item <= 0 || n % rows_per_item != 0 || w_mode < 0 || w_mode > 2) return TSGU_ERR_BAD_ARG;
    const int64_t items = n / rows_per_item;
    if (items == 0 || k == 0) return TSGU_OK;
    if (!Y || !out || !partial || (w_mode != 0 && !w)) return TSGU_ERR_BAD_ARG;
    const int64_t nb = mvn_blocks(rows_per_item);
    if (partial_elems < items * k * nb) return TSGU_ERR_BAD_ARG;
    const int64_t col_tiles = (k + kBlock - 1) / kBlock;
    if (items > 65535 || col_tiles > 65535) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto v) {
        using V = decltype(v);
        QuadArgs<V> a{static_cast<const V*>(Y), ldy, y_col_stride, static_cast<const V*>(E), lde, e_col_stride,
                      static_cast<const V*>(w), w_mode, k, rows_per_item, mvn_chunk(rows_per_item)};
        const int row_major = (k > 1 && y_col_stride == 1) ? 1 : 0;
        hipLaunchKernelGGL((quadform_partial_kernel<V>), dim3((unsigned)nb, (unsigned)items, (unsigned)col_tiles), dim3(kBlock),
                           0, s, a, row_major, static_cast<typename VT<V>::Acc*>(partial));
        if (const int rc = check_launch()) return rc;
        return finalize<V>(partial, nb, items * k, out, s);
    });
}

int tsgu_quadform_backward(int vtype, int64_t n, int64_t k, const void* Y, int64_t ldy, int64_t y_col_stride, const void* E,
                           int64_t lde, int64_t e_col_stride, const void* w, int w_mode, int64_t rows_per_item, const void* g,
                           void* grad_Y, int64_t ldg, int64_t g_col_stride, void* grad_w, int device, void* stream) {
    if (n < 0 || k < 0 || rows_per_item <= 0 || n % rows_per_item != 0 || w_mode < 0 || w_mode > 2) return TSGU_ERR_BAD_ARG;
    if (n == 0) return TSGU_OK;
    if (!Y || !g || !grad_Y || (w_mode != 0 && !w) || (grad_w && w_mode == 0)) return TSGU_ERR_BAD_ARG;
    const int64_t blocks = blocks_for(n);
    if (!grid_ok(blocks)) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto v) {
        using V = decltype(v);
        QuadArgs<V> a{static_cast<const V*>(Y), ldy, y_col_stride, static_cast<const V*>(E), lde, e_col_stride,
                      static_cast<const V*>(w), w_mode, k, rows_per_item, 0};
        hipLaunchKernelGGL((quadform_bwd_kernel<V>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a, n, static_cast<const V*>(g),
                           static_cast<V*>(grad_Y), ldg, g_col_stride, static_cast<V*>(grad_w));
        return check_launch();
    });
}

int tsgu_csr_row_sumsq(int vtype, int itype, int64_t n_rows, int64_t nnz, int64_t n_w, const void* crow, const void* col,
                       const void* perm, const void* val, const void* w, const void* add, void* out, int device,
                       void* stream) {
    if (n_rows < 0 || nnz < 0 || n_w < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows == 0) return TSGU_OK;
    if (!crow || !out || (nnz > 0 && (!col || !val))) return TSGU_ERR_BAD_ARG;
    const int64_t blocks = blocks_for(n_rows * kMvnRowLanes);
    if (!grid_ok(blocks)) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        hipLaunchKernelGGL((row_sumsq_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, n_rows, nnz, n_w,
                           static_cast<const I*>(crow), static_cast<const I*>(col), static_cast<const I*>(perm),
                           static_cast<const V*>(val), static_cast<const V*>(w), static_cast<const V*>(add), static_cast<V*>(out));
        return check_launch();
    });
}

int tsgu_csr_row_sumsq_backward(int vtype, int itype, int64_t n_rows, int64_t nnz, int64_t n_w, const void* crow,
                                const void* col, const void* perm, const void* val, const void* w, const void* g, void* grad_val,
                                int device, void* stream) {
    if (n_rows < 0 || nnz < 0 || n_w < 0) return TSGU_ERR_BAD_ARG;
    if (n_rows == 0 || nnz == 0) return TSGU_OK;
    if (!crow || !col || !val || !g || !grad_val) return TSGU_ERR_BAD_ARG;
    const int64_t blocks = blocks_for(n_rows * kMvnRowLanes);
    if (!grid_ok(blocks)) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        hipLaunchKernelGGL((row_sumsq_bwd_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, n_rows, nnz, n_w,
                           static_cast<const I*>(crow), static_cast<const I*>(col), static_cast<const I*>(perm),
                           static_cast<const V*>(val), static_cast<const V*>(w), static_cast<const V*>(g),
                           static_cast<V*>(grad_val));
        return check_launch();
    });
}

}  // extern "C"
