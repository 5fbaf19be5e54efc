// Sinkhorn half steps, their adjoints, the transport plan and the segmented sum: instantiations (fp32, fp64, bf16 × int32, int64)
// and the extern "C" entry points of tsgu_hip_sinkhorn.h.
#include "sinkhorn_impl.h"

#include "tsgu_hip_sinkhorn.h"

using namespace tsgu;

namespace {

// The host-side refusals the walking entries share; `blocks`: workgroups of the main kernel.  nnz = 0 still launches (every group
// is written), so `val`-like operands are checked only when there are entries.
int sk_check(int vtype, int itype, int64_t n_groups, int64_t nnz, std::initializer_list<const void*> always,
             std::initializer_list<const void*> with_entries, const void* workspace, int64_t workspace_bytes, int64_t* n_ranges,
             int64_t* blocks) {
    const int64_t range = seg_range_of(vtype);
    if (range < 0 || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (n_groups < 0 || nnz < 0 || workspace_bytes < 0) return TSGU_ERR_BAD_ARG;
    *n_ranges = seg_ranges(range, nnz);
    *blocks = seg_blocks(*n_ranges);
    if (n_groups == 0) return TSGU_OK;
    for (const void* p : always)
        if (!p) return TSGU_ERR_BAD_ARG;
    if (nnz > 0)
        for (const void* p : with_entries)
            if (!p) return TSGU_ERR_BAD_ARG;
    if (*blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (workspace || workspace_bytes) {
        if (!workspace || !aligned16(workspace) || workspace_bytes < seg_ws_bytes(vtype, nnz)) return TSGU_ERR_BAD_ARG;
    }
    return TSGU_OK;
}

}  // namespace

extern "C" {

int tsgu_sinkhorn_workspace(int vtype, int64_t nnz, int64_t* bytes_host) {
    if (nnz < 0 || !bytes_host) return TSGU_ERR_BAD_ARG;
    const int64_t b = seg_ws_bytes(vtype, nnz);
    if (b < 0) return TSGU_ERR_BAD_DTYPE;
    *bytes_host = b;
    return TSGU_OK;
}

int tsgu_sinkhorn_half(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* idx,
                       const void* val, const void* other, const void* log_marg, void* out, void* workspace, int64_t workspace_bytes,
                       int device, void* stream) {
    int64_t n_ranges = 0, blocks = 0;
    if (const int rc = sk_check(vtype, itype, n_groups, nnz, {ptr, out}, {idx, val, other}, workspace, workspace_bytes, &n_ranges, &blocks))
        return rc;
    if (n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        using Acc = typename VT<V>::Acc;
        SkHalf<V> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.idx = idx;
        P.val = static_cast<const V*>(val);
        P.other = static_cast<const Acc*>(other);
        P.log_marg = static_cast<const Acc*>(log_marg);
        P.out = static_cast<Acc*>(out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = n_ranges;
        P.vec_ok = aligned16(val) ? 1 : 0;
        seg_set_workspace<Acc>(P, workspace);
        if (const int rc = launch(sk_half_kernel<V, I>, blocks, s, P)) return rc;
        return workspace && n_ranges > 1 ? launch(seg_merge_kernel<SkHalfOp<V>, I>, blocks, s, P) : (int)TSGU_OK;
    });
}

int tsgu_sinkhorn_plan(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* idx, const void* val,
                       const void* pot_group, const void* pot_other, void* out, int device, void* stream) {
    if (seg_range_of(vtype) < 0 || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (nnz < 0 || n_groups < 0) return TSGU_ERR_BAD_ARG;
    if (nnz == 0) return TSGU_OK;
    if (n_groups == 0 || !ptr || !idx || !val || !pot_group || !pot_other || !out) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        using Acc = typename VT<V>::Acc;
        SkPlan<V> P{};
        P.ptr = ptr;
        P.idx = idx;
        P.val = static_cast<const V*>(val);
        P.pot_group = static_cast<const Acc*>(pot_group);
        P.pot_other = static_cast<const Acc*>(pot_other);
        P.out = static_cast<V*>(out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.vec_ok = aligned16(val) && aligned16(out) ? 1 : 0;
        constexpr int64_t per_block = (int64_t)kBlock * VT<V>::kWide;
        const int64_t blocks = (nnz + per_block - 1) / per_block;
        if (blocks > 0x7fffffffLL) return (int)TSGU_ERR_TOO_LARGE;
        return launch(sk_plan_kernel<V, I>, blocks, s, P);
    });
}

int tsgu_sinkhorn_half_backward(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* idx,
                                const void* grp, const void* val, const void* pot_group, const void* pot_other,
                                const void* log_marg_other, const void* g_other, void* grad, void* g_out, int accumulate,
                                void* workspace, int64_t workspace_bytes, int device, void* stream) {
    int64_t n_ranges = 0, blocks = 0;
    if (const int rc = sk_check(vtype, itype, n_groups, nnz, {ptr, g_out}, {idx, grp, val, pot_group, pot_other, g_other, grad}, workspace,
                                workspace_bytes, &n_ranges, &blocks))
        return rc;
    if (n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        using Acc = typename VT<V>::Acc;
        SkBwd<V> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.idx = idx;
        P.grp = grp;
        P.val = static_cast<const V*>(val);
        P.pot_group = static_cast<const Acc*>(pot_group);
        P.pot_other = static_cast<const Acc*>(pot_other);
        P.log_marg_other = static_cast<const Acc*>(log_marg_other);
        P.g_other = static_cast<const Acc*>(g_other);
        P.grad = static_cast<Acc*>(grad);
        P.g_out = static_cast<Acc*>(g_out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = n_ranges;
        P.accumulate = accumulate ? 1 : 0;
        P.vec_ok = aligned16(val) ? 1 : 0;
        seg_set_workspace<Acc>(P, workspace);
        if (const int rc = launch(sk_half_bwd_kernel<V, I>, blocks, s, P)) return rc;
        return workspace && n_ranges > 1 ? launch(seg_merge_kernel<SkBwdOp<V>, I>, blocks, s, P) : (int)TSGU_OK;
    });
}

int tsgu_segment_sum(int vtype, int itype, int64_t n_groups, int64_t nnz, const void* ptr, const void* perm, const void* val,
                     const void* add, void* out, void* workspace, int64_t workspace_bytes, int device, void* stream) {
    int64_t n_ranges = 0, blocks = 0;
    if (const int rc = sk_check(vtype, itype, n_groups, nnz, {ptr, out}, {val}, workspace, workspace_bytes, &n_ranges, &blocks)) return rc;
    if (n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // (the values are accumulators already: bf16 operands sum as fp32)
    return with_types<float, double>(vtype == TSGU_BF16 ? (int)TSGU_F32 : vtype, itype, [&](auto a, auto i) {
        using A = decltype(a);
        using I = decltype(i);
        SegSum<A> P{};
        P.ptr = ptr;
        P.perm = perm;
        P.val = static_cast<const A*>(val);
        P.add = static_cast<const A*>(add);
        P.out = static_cast<A*>(out);
        P.n_groups = n_groups;
        P.nnz = nnz;
        P.n_ranges = n_ranges;
        P.vec_ok = aligned16(val) ? 1 : 0;
        seg_set_workspace<A>(P, workspace);
        if (const int rc = launch(seg_sum_kernel<A, I>, blocks, s, P)) return rc;
        return workspace && n_ranges > 1 ? launch(seg_merge_kernel<SegSumOp<A>, I>, blocks, s, P) : (int)TSGU_OK;
    });
}

}  // extern "C"
