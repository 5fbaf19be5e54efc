// Entry points of the factorised sparse approximate inverse (include/tsgu_hip_fsai.h; kernel: fsai_impl.h).
#include "fsai_impl.h"

#include "../../include/tsgu_hip_fsai.h"

namespace tsgu {

template <typename V, typename I>
int fsai_launch(const FsaiParams& P, int n_cu, int wg_per_cu, hipStream_t stream) {
    if (hipMemsetAsync(P.info, 0, sizeof(unsigned long long), stream) != hipSuccess) return TSGU_ERR_RUNTIME;
    const int per_cu = wg_per_cu < 1 ? 1 : (wg_per_cu > 8 ? 8 : wg_per_cu);
    const int64_t resident = (int64_t)n_cu * per_cu;
    const int64_t blocks = P.chunks < resident ? P.chunks : resident;
    hipLaunchKernelGGL((fsai_kernel<V, I>), dim3((unsigned)blocks), dim3(kWave), 0, stream, P);
    if (const int rc = check_launch()) return rc;
    hipLaunchKernelGGL(fsai_info_kernel, dim3(1), dim3(1), 0, stream, P.info);
    return check_launch();
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_csr_fsai_geometry(int vtype, int* row_capacity, int* rows_per_block) {
    if (!row_capacity || !rows_per_block) return TSGU_ERR_BAD_ARG;
    return with_value_type<float, double>(vtype, [&](auto) {
        *row_capacity = kFsaiCap;
        *rows_per_block = kFsaiRows;
        return (int)TSGU_OK;
    });
}

int tsgu_csr_fsai(int vtype, int itype, int64_t n, const void* a_ptr, const void* a_idx, const void* a_val, const void* s_ptr,
                  const void* s_idx, int64_t s_nnz, const void* order, void* out, int64_t* info, int workgroups_per_cu, int device,
                  void* stream) {
    if (n < 0 || s_nnz < 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;     // (bf16 included)
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n == 0) return TSGU_OK;                                                // (nothing to build: info is the caller's)
    if (!a_ptr || !a_idx || !a_val || !s_ptr || !s_idx || !out || !info) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_cu = device_cu_count(device);
    if (n_cu == 0) return TSGU_ERR_RUNTIME;
    FsaiParams P{};
    P.n = n;
    P.s_nnz = s_nnz;
    P.chunks = (n + kFsaiRows - 1) / kFsaiRows;
    P.a_ptr = a_ptr;
    P.a_idx = a_idx;
    P.a_val = a_val;
    P.s_ptr = s_ptr;
    P.s_idx = s_idx;
    P.order = order;
    P.out = out;
    P.info = reinterpret_cast<unsigned long long*>(info);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        return fsai_launch<decltype(v), decltype(i)>(P, n_cu, workgroups_per_cu, s);
    });
}

}  // extern "C"
