// Entry points of the zero-fill incomplete factorisations (include/tsgu_hip_factor.h; kernels: ilu_impl.h).
#include "ilu_impl.h"

#include "../../include/tsgu_hip_factor.h"

namespace tsgu {

template <typename V, typename I, bool IC>
int factor_launch(const FactorParams& P, int64_t* info, int n_cu, int wg_per_cu, hipStream_t stream) {
    // re-initialised every call: tickets, error word, breakdown word and done[] are ONE block at the start of the work buffer
    if (hipMemsetAsync(P.work, 0, (size_t)factor_zero_bytes(P.n), stream) != hipSuccess) return TSGU_ERR_RUNTIME;
    const int64_t blocks = persistent_blocks(n_cu, wg_per_cu, P.n);
    FactorParams Q = P;
    Q.wgc = (int)(blocks < 64 ? blocks : 64);
    hipLaunchKernelGGL((factor_syncfree_kernel<V, I, IC>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, Q);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(factor_info_kernel, dim3(1), dim3(1), 0, stream, P.work, info);
    return check_launch();
}

template <bool IC>
int factor_entry(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* diag_pos, const void* val,
                 double shift, void* out, void* work, int64_t* info, int workgroups_per_cu, int device, void* stream) {
    if (n < 0 || nnz < 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;     // (bf16 included: a bf16 factor is of no use)
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n == 0) return TSGU_OK;
    if (!ptr || !idx || !diag_pos || !val || !out || !work || !info) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    const int n_cu = device_cu_count(device);
    if (n_cu == 0) return TSGU_ERR_RUNTIME;
    FactorParams P{};
    P.n = n;
    P.nnz = nnz;
    P.ptr = ptr;
    P.idx = idx;
    P.diag_pos = diag_pos;
    P.val = val;
    P.out = out;
    P.work = static_cast<FactorWork*>(work);
    P.diag_scale = 1.0 + shift;
    P.timeout_ticks = kSpinTimeoutTicks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        return factor_launch<decltype(v), decltype(i), IC>(P, info, n_cu, workgroups_per_cu, s);
    });
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int64_t tsgu_csr_factor_work_bytes(int64_t n) { return n < 0 ? 0 : factor_zero_bytes(n); }

int tsgu_csr_factor_geometry(int vtype, int* row_capacity, int* waves_per_block) {
    if (!row_capacity || !waves_per_block) return TSGU_ERR_BAD_ARG;
    return with_value_type<float, double>(vtype, [&](auto v) {
        *row_capacity = FactorGeom<decltype(v)>::kCap;
        *waves_per_block = kTrsmWaves;
        return (int)TSGU_OK;
    });
}

int tsgu_csr_ilu0(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* diag_pos, const void* val,
                  double shift, void* out, void* work, int64_t* info, int workgroups_per_cu, int device, void* stream) {
    return factor_entry<false>(vtype, itype, n, nnz, ptr, idx, diag_pos, val, shift, out, work, info, workgroups_per_cu, device, stream);
}

int tsgu_csr_ic0(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* diag_pos, const void* val,
                 double shift, void* out, void* work, int64_t* info, int workgroups_per_cu, int device, void* stream) {
    return factor_entry<true>(vtype, itype, n, nnz, ptr, idx, diag_pos, val, shift, out, work, info, workgroups_per_cu, device, stream);
}

}  // extern "C"
