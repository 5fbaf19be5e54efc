// K10: entry points of the Lanczos quadrature and the Rademacher fill (quadrature_impl.h; contracts in tsgu_hip_quadrature.h).
#include "quadrature_impl.h"
#include "tsgu_hip_quadrature.h"

using namespace tsgu;

extern "C" {

int tsgu_quadrature_geometry(int* steps_cap, int64_t* work_bytes_per_column) {
    if (!steps_cap || !work_bytes_per_column) return TSGU_ERR_BAD_ARG;
    *steps_cap = kQuadCap;
    *work_bytes_per_column = (int64_t)3 * kQuadCap * sizeof(double);
    return TSGU_OK;
}

int tsgu_tridiag_quadrature(int vtype, int kind, int fn, int r, int64_t p, const void* coef, const void* scale, void* out, int* info,
                            void* work, int device, void* stream) {
    if (!coef || !out || !info || r <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    if (kind != kQuadCg && kind != kQuadEntries) return TSGU_ERR_BAD_ARG;
    if (fn < kQuadLog || fn > kQuadOne) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (r > kQuadCap) return TSGU_ERR_TOO_LARGE;
    const bool lds = r <= kQuadLdsRows;
    if (r > kQuadNoWorkRows && (!work || (reinterpret_cast<uintptr_t>(work) & 7u))) return TSGU_ERR_BAD_ARG;
    const int64_t grid = (p + kQuadLanes - 1) / kQuadLanes;
    if (grid > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const QuadParams P{kind, fn, r, p, coef, scale, out, info, static_cast<double*>(work)};
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        if (lds) {
            const int bytes = 3 * (int)sizeof(double) * kQuadLanes * r;
            return launch_large_lds<tridiag_quadrature_kernel<V, true>>(device, grid, kQuadLanes, bytes, kQuadMaxLds, s, P);
        }
        hipLaunchKernelGGL((tridiag_quadrature_kernel<V, false>), dim3((unsigned)grid), dim3(kQuadLanes), 0, s, P);
        return check_launch();
    });
}

int tsgu_rademacher_fill(int vtype, int64_t n, int64_t p, int64_t seed, void* out, int device, void* stream) {
    if (!out || n <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (n > 0xffffffffLL || p > 0x7fffffffLL || n > (0x7fffffffLL * kBlock) / p) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t blocks = (n * p + kBlock - 1) / kBlock;
    const unsigned word = rademacher_seed_word(seed);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        return launch(rademacher_fill_kernel<V>, blocks, s, n, p, word, (V*)out);
    });
}

}  // extern "C"
