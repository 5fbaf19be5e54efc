// Segmented softmax / log-softmax and their gradient: instantiations (fp32, fp64, bf16 × int32, int64) and the extern "C" entry
// points of include/tsgu_hip_softmax.h.
#include "softmax_impl.h"

#include "../../include/tsgu_hip_softmax.h"

using namespace tsgu;

namespace {

int64_t sm_range_of(int vtype) {
    if (vtype == TSGU_F32 || vtype == TSGU_BF16) return lse_range<float>();
    if (vtype == TSGU_F64) return lse_range<double>();
    return -1;
}

int64_t sm_ranges(int64_t range, int64_t nnz) { return nnz > 0 ? (nnz + range - 1) / range : 1; }

// Acc[n_ranges][kSmSlots] and the tail groups int64[n_ranges]
int64_t sm_ws_bytes(int vtype, int64_t nnz) {
    const int64_t range = sm_range_of(vtype);
    if (range < 0) return -1;
    return sm_ranges(range, nnz) * (int64_t)(kSmSlots * (kLseStageBytes / range) + sizeof(int64_t));
}

// The host-side refusals both entries share; `blocks`: workgroups of the main kernel.
int sm_check(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, std::initializer_list<const void*> operands,
             const void* workspace, int64_t workspace_bytes, int64_t* n_ranges, int64_t* blocks) {
    const int64_t range = sm_range_of(vtype);
    if (range < 0 || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (n_groups < 0 || nnz < 0 || workspace_bytes < 0) return TSGU_ERR_BAD_ARG;
    *n_ranges = sm_ranges(range, nnz);
    *blocks = (*n_ranges + kLseWavesPerBlock - 1) / kLseWavesPerBlock;
    if (n_groups == 0 || nnz == 0) return TSGU_OK;
    if (!ptr) return TSGU_ERR_BAD_ARG;
    for (const void* p : operands)
        if (!p) return TSGU_ERR_BAD_ARG;
    if (*blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (workspace || workspace_bytes) {
        if (!workspace || !aligned16(workspace) || workspace_bytes < sm_ws_bytes(vtype, nnz)) return TSGU_ERR_BAD_ARG;
    }
    return TSGU_OK;
}

template <typename P>
void sm_set_workspace(P& p, void* workspace, int64_t acc_bytes) {
    p.part = workspace;
    p.tail = workspace ? reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + p.n_ranges * kSmSlots * acc_bytes) : nullptr;
}

}  // namespace

extern "C" {

int tsgu_segment_softmax_workspace(int vtype, int64_t nnz, int64_t* bytes_host) {
    if (nnz < 0 || !bytes_host) return TSGU_ERR_BAD_ARG;
    const int64_t b = sm_ws_bytes(vtype, nnz);
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
        sm_set_workspace(P, workspace, sizeof(typename VT<V>::Acc));
        if (const int rc = launch(sm_fwd_kernel<V, I>, blocks, s, P)) return rc;
        if (!workspace) return (int)TSGU_OK;
        if (const int rc = launch(sm_merge_kernel<V, I>, blocks, s, P)) return rc;
        return launch(sm_fix_kernel<V, I>, blocks, s, P);
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
        sm_set_workspace(P, workspace, sizeof(typename VT<V>::Acc));
        if (const int rc = launch(sm_bwd_kernel<V, I>, blocks, s, P)) return rc;
        if (!workspace) return (int)TSGU_OK;
        if (const int rc = launch(sm_bwd_merge_kernel<V, I>, blocks, s, P)) return rc;
        return launch(sm_bwd_fix_kernel<V, I>, blocks, s, P);
    });
}

}  // extern "C"
