// Segmented log-sum-exp and its gradient: instantiations (fp32, fp64, bf16 × int32, int64) and the extern "C" entry points.
#include "logsumexp_impl.h"

using namespace tsgu;

namespace {

template <typename V>
int64_t lse_ranges(int64_t nnz) {
    constexpr int64_t R = lse_range<typename VT<V>::Acc>();
    return nnz > 0 ? (nnz + R - 1) / R : 1;
}

template <typename V>
int64_t lse_ws_bytes(int64_t nnz) {
    return lse_ranges<V>(nnz) * (int64_t)(4 * sizeof(typename VT<V>::Acc) + sizeof(int64_t));
}

int64_t ws_bytes_of(int vtype, int64_t nnz) {
    if (vtype == TSGU_F32) return lse_ws_bytes<float>(nnz);
    if (vtype == TSGU_F64) return lse_ws_bytes<double>(nnz);
    if (vtype == TSGU_BF16) return lse_ws_bytes<bf16_t>(nnz);
    return -1;
}

template <typename V, typename I>
int lse_fwd_launch(LseFwd<V> P, hipStream_t s) {
    using Acc = typename VT<V>::Acc;
    P.n_ranges = lse_ranges<V>(P.nnz);
    P.tail = reinterpret_cast<int64_t*>(static_cast<char*>(P.part) + P.n_ranges * 4 * sizeof(Acc));
    const int64_t blocks = (P.n_ranges + kLseWavesPerBlock - 1) / kLseWavesPerBlock;
    if (blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    hipLaunchKernelGGL((lse_fwd_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    if (const int rc = check_launch()) return rc;
    if (P.n_ranges > 1) {
        hipLaunchKernelGGL((lse_merge_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
        if (const int rc = check_launch()) return rc;
    }
    return TSGU_OK;
}

template <typename V, typename I>
int lse_bwd_launch(const LseBwd<V>& P, hipStream_t s) {
    constexpr int64_t per_block = (int64_t)kBlock * VT<V>::kWide;
    const int64_t blocks = (P.nnz + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    hipLaunchKernelGGL((lse_bwd_kernel<V, I>), dim3((unsigned)blocks), dim3(kBlock), 0, s, P);
    return check_launch();
}

}  // namespace

extern "C" {

int tsgu_segment_logsumexp_workspace(int vtype, int64_t nnz, int64_t* bytes_host) {
    if (nnz < 0 || !bytes_host) return TSGU_ERR_BAD_ARG;
    const int64_t b = ws_bytes_of(vtype, nnz);
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
    const int64_t need = ws_bytes_of(vtype, nnz);
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
        P.part = workspace;
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.axis_len = include_zeros ? axis_len : -1;
        P.gpi = groups_per_item;
        P.ostride = item_stride;
        P.vec_ok = aligned16(val) ? 1 : 0;
        return lse_fwd_launch<V, I>(P, s);
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
        return lse_bwd_launch<V, I>(P, s);
    });
}

}  // extern "C"
