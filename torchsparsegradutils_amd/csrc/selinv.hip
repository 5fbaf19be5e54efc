// Entry points of the selected inversion (include/tsgu_hip_selinv.h; kernels: selinv_impl.h).
#include "selinv_impl.h"

#include "../../include/tsgu_hip_selinv.h"

namespace tsgu {

template <typename V, typename I, bool LDLT>
int selinv_launch(const SelinvParams& P, int64_t* info, int n_cu, int wg_per_cu, hipStream_t stream) {
    // re-initialised every call: tickets, error word, the two report words and done[] are ONE block at the start of the work buffer
    if (hipMemsetAsync(P.work, 0, (size_t)selinv_zero_bytes(P.n), stream) != hipSuccess) return TSGU_ERR_RUNTIME;
    const int64_t blocks = persistent_blocks(n_cu, wg_per_cu, P.n);
    SelinvParams Q = P;
    Q.wgc = (int)(blocks < 64 ? blocks : 64);
    Q.sig = reinterpret_cast<char*>(P.work) + selinv_zero_bytes(P.n);
    hipLaunchKernelGGL((selinv_syncfree_kernel<V, I, LDLT>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, Q);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(selinv_info_kernel, dim3(1), dim3(1), 0, stream, P.work, info);
    return check_launch();
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int64_t tsgu_csc_selinv_work_bytes(int vtype, int64_t n, int64_t nnz) {
    if (n < 0 || nnz < 0 || (vtype != TSGU_F32 && vtype != TSGU_F64)) return 0;
    return selinv_work_bytes(n, nnz, vtype == TSGU_F32 ? 4 : 8);
}

int tsgu_csc_selinv_geometry(int vtype, int* column_capacity, int* waves_per_block) {
    if (!column_capacity || !waves_per_block) return TSGU_ERR_BAD_ARG;
    return with_value_type<float, double>(vtype, [&](auto v) {
        *column_capacity = SelinvGeom<decltype(v)>::kCap;
        *waves_per_block = kTrsmWaves;
        return (int)TSGU_OK;
    });
}

int tsgu_csc_selinv(int vtype, int itype, int64_t n, int64_t nnz, const void* colptr, const void* rowidx, const void* perm,
                    const void* diag_pos, const void* val, const void* D, void* out, void* diag_out, void* work, int64_t* info,
                    int workgroups_per_cu, int device, void* stream) {
    if (n < 0 || nnz < 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n == 0) return TSGU_OK;
    if (!colptr || !work || !info || (D ? !diag_out : !diag_pos)) return TSGU_ERR_BAD_ARG;
    if (nnz > 0 && (!rowidx || !val || !out)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    const int n_cu = device_cu_count(device);
    if (n_cu == 0) return TSGU_ERR_RUNTIME;
    SelinvParams P{};
    P.n = n;
    P.nnz = nnz;
    P.ptr = colptr;
    P.idx = rowidx;
    P.perm = perm;
    P.diag_pos = diag_pos;
    P.val = val;
    P.D = D;
    P.out = out;
    P.diag_out = diag_out;
    P.work = static_cast<SelinvWork*>(work);
    P.timeout_ticks = kSpinTimeoutTicks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        return D ? selinv_launch<V, I, true>(P, info, n_cu, workgroups_per_cu, s) : selinv_launch<V, I, false>(P, info, n_cu, workgroups_per_cu, s);
    });
}

}  // extern "C"
