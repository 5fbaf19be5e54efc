// Segmented log-sum-exp and its gradient: instantiations (fp32, fp64, bf16 × int32, int64) and the extern "C" entry points.
#include "logsumexp_impl.h"

using namespace tsgu;

extern "C" {

int tsgu_segment_logsumexp_workspace(int vtype, int64_t nnz, int64_t* bytes_host) {
    if (nnz < 0 || !bytes_host) return TSGU_ERR_BAD_ARG;
    const int64_t b = seg_ws_bytes(vtype, nnz);
    if (b < 0) return TSGU_ERR_BAD_DTYPE;
    *bytes_host = b;
    return TSGU_OK;
}

int tsgu_segment_logsumexp(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm,
                           const void* val, int include_zeros, int64_t axis_len, void* out, int64_t groups_per_item,
                           int64_t item_stride, void* workspace, int64_t workspace_bytes, int device, void* stream) {
    if (n_groups < 0 || nnz < 0 || axis_len < 0) return TSGU_ERR_BAD_ARG;
    if (n_groups == 0) return TSGU_OK;
    if (groups_per_item <= 0 || n_groups % groups_per_item != 0 || item_stride < groups_per_item) return TSGU_ERR_BAD_ARG;
    if (!ptr || !out || !workspace || (nnz > 0 && !val)) return TSGU_ERR_BAD_ARG;
    const int64_t need = seg_ws_bytes(vtype, nnz);
    if (need < 0) return TSGU_ERR_BAD_DTYPE;
    if (workspace_bytes < need || !aligned16(workspace)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        LseFwd<V> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.val = static_cast<const V*>(val);
        P.out = static_cast<V*>(out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = seg_ranges(seg_range_of(vtype), nnz);
        P.axis_len = include_zeros ? axis_len : -1;
        P.gpi = groups_per_item;
        P.ostride = item_stride;
        P.vec_ok = aligned16(val) ? 1 : 0;
        seg_set_workspace<typename VT<V>::Acc>(P, workspace);
        const int64_t blocks = seg_blocks(P.n_ranges);
        if (blocks > 0x7fffffffLL) return (int)TSGU_ERR_TOO_LARGE;
        if (const int rc = launch(lse_fwd_kernel<V, I>, blocks, s, P)) return rc;
        return P.n_ranges > 1 ? launch(seg_merge_kernel<LseOp<V>, I>, blocks, s, P) : (int)TSGU_OK;
    });
}

int tsgu_segment_logsumexp_backward(int vtype, int itype, int64_t nnz, const void* val, const void* ptr, int64_t n_groups,
                                    const void* g_grp, const void* lse_grp, const void* idx, const void* g_idx,
                                    const void* lse_idx, void* grad, int device, void* stream) {
    if (nnz < 0 || n_groups < 0) return TSGU_ERR_BAD_ARG;
    if (nnz == 0) return TSGU_OK;
    if (!val || !grad || (!ptr && !idx)) return TSGU_ERR_BAD_ARG;
    if ((ptr && (!g_grp || !lse_grp || n_groups <= 0)) || (idx && (!g_idx || !lse_idx))) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        LseBwd<V> P{};
        P.ptr = ptr;
        P.g1 = static_cast<const V*>(g_grp);
        P.lse1 = static_cast<const V*>(lse_grp);
        P.idx = idx;
        P.g2 = static_cast<const V*>(g_idx);
        P.lse2 = static_cast<const V*>(lse_idx);
        P.val = static_cast<const V*>(val);
        P.grad = static_cast<V*>(grad);
        P.n1 = n_groups;
        P.nnz = nnz;
        P.vec_ok = aligned16(val) && aligned16(grad) ? 1 : 0;
        constexpr int64_t per_block = (int64_t)kBlock * VT<V>::kWide;
        const int64_t blocks = (nnz + per_block - 1) / per_block;
        if (blocks > 0x7fffffffLL) return (int)TSGU_ERR_TOO_LARGE;
        return launch(lse_bwd_kernel<V, I>, blocks, s, P);
    });
}

}  // extern "C"
