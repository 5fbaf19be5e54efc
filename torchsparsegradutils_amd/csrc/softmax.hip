// Segmented softmax / log-softmax and their gradient: instantiations (fp32, fp64, bf16 × int32, int64) and the extern "C" entry
// points of include/tsgu_hip_softmax.h.
#include "softmax_impl.h"

#include "../../include/tsgu_hip_softmax.h"

using namespace tsgu;

namespace {

// The host-side refusals both entries share; `blocks`: workgroups of the main kernel.
int sm_check(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, std::initializer_list<const void*> operands,
             const void* workspace, int64_t workspace_bytes, int64_t* n_ranges, int64_t* blocks) {
    const int64_t range = seg_range_of(vtype);
    if (range < 0 || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (n_groups < 0 || nnz < 0 || workspace_bytes < 0) return TSGU_ERR_BAD_ARG;
    *n_ranges = seg_ranges(range, nnz);
    *blocks = seg_blocks(*n_ranges);
    if (n_groups == 0 || nnz == 0) return TSGU_OK;
    if (!ptr) return TSGU_ERR_BAD_ARG;
    for (const void* p : operands)
        if (!p) return TSGU_ERR_BAD_ARG;
    if (*blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (workspace || workspace_bytes) {
        if (!workspace || !aligned16(workspace) || workspace_bytes < seg_ws_bytes(vtype, nnz)) return TSGU_ERR_BAD_ARG;
    }
    return TSGU_OK;
}

}  // namespace

extern "C" {

int tsgu_segment_softmax_workspace(int vtype, int64_t nnz, int64_t* bytes_host) {
    if (nnz < 0 || !bytes_host) return TSGU_ERR_BAD_ARG;
    const int64_t b = seg_ws_bytes(vtype, nnz);
    if (b < 0) return TSGU_ERR_BAD_DTYPE;
    *bytes_host = b;
    return TSGU_OK;
}

int tsgu_segment_softmax(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* val,
                         int log_form, void* out, void* workspace, int64_t workspace_bytes, int device, void* stream) {
    int64_t n_ranges = 0, blocks = 0;
    if (const int rc = sm_check(vtype, itype, n_groups, nnz, ptr, {val, out}, workspace, workspace_bytes, &n_ranges, &blocks)) return rc;
    if (n_groups == 0 || nnz == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        SmFwd<V> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.val = static_cast<const V*>(val);
        P.out = static_cast<V*>(out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = n_ranges;
        P.log_form = log_form ? 1 : 0;
        P.vec_ok = aligned16(val) && aligned16(out) ? 1 : 0;
        seg_set_workspace<typename VT<V>::Acc>(P, workspace);
        if (const int rc = launch(sm_fwd_kernel<V, I>, blocks, s, P)) return rc;
        if (!workspace) return (int)TSGU_OK;
        if (const int rc = launch(seg_merge_kernel<SmFwdOp<V>, I>, blocks, s, P)) return rc;
        return launch(seg_fix_kernel<SmFwdOp<V>, I>, blocks, s, P);
    });
}

int tsgu_segment_softmax_backward(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm,
                                  const void* y, const void* g, int log_form, void* gin, void* workspace,
                                  int64_t workspace_bytes, int device, void* stream) {
    int64_t n_ranges = 0, blocks = 0;
    if (const int rc = sm_check(vtype, itype, n_groups, nnz, ptr, {y, g, gin}, workspace, workspace_bytes, &n_ranges, &blocks)) return rc;
    if (n_groups == 0 || nnz == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        SmBwd<V> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.y = static_cast<const V*>(y);
        P.g = static_cast<const V*>(g);
        P.gin = static_cast<V*>(gin);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = n_ranges;
        P.log_form = log_form ? 1 : 0;
        P.vec_ok = aligned16(y) && aligned16(g) && aligned16(gin) ? 1 : 0;
        seg_set_workspace<typename VT<V>::Acc>(P, workspace);
        if (const int rc = launch(sm_bwd_kernel<V, I>, blocks, s, P)) return rc;
        if (!workspace) return (int)TSGU_OK;
        if (const int rc = launch(seg_merge_kernel<SmBwdOp<V>, I>, blocks, s, P)) return rc;
        return launch(seg_fix_kernel<SmBwdOp<V>, I>, blocks, s, P);
    });
}

}  // extern "C"
