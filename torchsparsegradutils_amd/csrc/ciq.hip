// K11: entry points of the contour-quadrature update (ciq_impl.h; contracts in tsgu_hip_ciq.h).
#include "ciq_impl.h"
#include "tsgu_hip_ciq.h"

using namespace tsgu;

namespace {

inline bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace

extern "C" {

int tsgu_ciq_geometry(int vtype, int64_t n, int64_t p, int* shift_cap, int* plane_align, int64_t* rows_per_workgroup,
                      int64_t* workgroups) {
    if (!shift_cap || !plane_align || !rows_per_workgroup || !workgroups || n <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    VecGeom g;
    const bool ok = vtype == TSGU_F32 ? geom_for<float>(n, p, true, g) : geom_for<double>(n, p, true, g);
    if (!ok || g.blocks > 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    *shift_cap = kCiqShiftCap;
    *plane_align = vtype == TSGU_F32 ? 4 : 2;
    *rows_per_workgroup = (int64_t)g.rpp * kPasses;
    *workgroups = g.blocks;
    return TSGU_OK;
}

int tsgu_ciq_update(int vtype, int64_t n, int64_t p, int n_shift, void* zc, const void* zp, void* wpp, const void* wp,
                    int64_t shift_stride, void* acc, void* keep, const void* scal, const void* omega, const int* done, const int* flags,
                    int device, void* stream) {
    if (!zc || !zp || !wpp || !wp || !acc || !scal || !omega || !done || !flags || n <= 0 || p <= 0 || n_shift < 1)
        return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    const size_t elem = vtype == TSGU_F64 ? 8 : 4;
    if (!(aligned16(zc) && aligned16(zp) && aligned16(wpp) && aligned16(wp) && aligned16(acc) && aligned16(keep))) return TSGU_ERR_BAD_ARG;
    if (!(aligned_to(scal, elem) && aligned_to(omega, elem) && aligned_to(done, 4) && aligned_to(flags, 4))) return TSGU_ERR_BAD_ARG;
    if (n > INT64_MAX / p || shift_stride < n * p || ((shift_stride * (int64_t)elem) & 15)) return TSGU_ERR_BAD_ARG;
    if (n_shift > kCiqShiftCap) return TSGU_ERR_TOO_LARGE;
    VecGeom probe;
    if (!(vtype == TSGU_F32 ? geom_for<float>(n, p, true, probe) : geom_for<double>(n, p, true, probe)) || probe.blocks > 0x7fffffffLL)
        return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        auto go = [&](auto kern, const VecGeom& g) -> int {
            return launch(kern, g.blocks, s, n, p, n_shift, (V*)zc, (const V*)zp, (V*)wpp, (const V*)wp, shift_stride, (V*)acc, (V*)keep,
                          (const V*)scal, (const V*)omega, done, flags, g.lpr, g.rpp);
        };
        if (keep) return launch_lanes<V>(n, p, ciq_update_kernel<V, 1, true>, ciq_update_kernel<V, wide, true>, go);
        return launch_lanes<V>(n, p, ciq_update_kernel<V, 1, false>, ciq_update_kernel<V, wide, false>, go);
    });
}

int tsgu_ciq_stop(int vtype, int64_t p, int n_shift, const void* scal, double tol, void* est, int* done, int* flags, int device,
                  void* stream) {
    if (!scal || !est || !done || !flags || p <= 0 || n_shift < 1) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    const size_t elem = vtype == TSGU_F64 ? 8 : 4;
    if (!(aligned_to(scal, elem) && aligned_to(est, elem) && aligned_to(done, 4) && aligned_to(flags, 4))) return TSGU_ERR_BAD_ARG;
    if (n_shift > kCiqShiftCap || p > (int64_t)kBlock * 16) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        return launch(ciq_stop_kernel<V>, 1, s, p, n_shift, (const V*)scal, (V)tol, (V*)est, done, flags);
    });
}

}  // extern "C"
