// K8: entry points of the GMRES Arnoldi kernels (gmres_impl.h; contracts in tsgu_hip_gmres.h).
#include "gmres_impl.h"
#include "tsgu_hip_gmres.h"

using namespace tsgu;

namespace {

// a basis of k blocks, `slab` elements apart: every block must start on a 16-byte boundary
inline bool block_args_ok(int64_t n, int64_t p, int k, int64_t slab) {
    return n > 0 && p > 0 && k >= 1 && k <= kGmresCap + 1 && slab >= n * p && slab % 4 == 0;
}

// the value types and widths the lane geometry covers, decided before the device is touched
inline int lanes_cover(int vtype, int64_t n, int64_t p) {
    return with_value_type(vtype, [&](auto tag) -> int {
        VecGeom g;
        return geom_for<decltype(tag)>(n, p, true, g) ? TSGU_OK : TSGU_ERR_TOO_LARGE;
    });
}

}  // namespace

extern "C" {

int tsgu_gmres_geometry(int vtype, int64_t n, int64_t p, int* restart_cap, int* group, int64_t* rows_per_workgroup,
                        int64_t* partial_rows) {
    if (!restart_cap || !group || !rows_per_workgroup || !partial_rows || n <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        VecGeom g;
        if (!geom_for<V>(n, p, true, g)) return TSGU_ERR_TOO_LARGE;
        *restart_cap = kGmresCap;
        *group = kGmresGroup;
        *rows_per_workgroup = (int64_t)g.rpp * kPasses;
        *partial_rows = g.blocks;
        return TSGU_OK;
    });
}

int tsgu_gmres_project(int vtype, int64_t n, int64_t p, int k, const void* w, const void* basis, int64_t slab, void* partial,
                       const int* flags, int inner, int device, void* stream) {
    if (!block_args_ok(n, p, k, slab) || !w || !basis || !partial || !flags) return TSGU_ERR_BAD_ARG;
    if (!(aligned16(w) && aligned16(basis))) return TSGU_ERR_BAD_ARG;
    if (const int rc = lanes_cover(vtype, n, p)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        return launch_lanes<V>(n, p, gmres_project_kernel<V, 1>, gmres_project_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
            return launch(kern, g.blocks, s, n, p, k, (const V*)w, (const V*)basis, slab, (V*)partial, flags, inner, g.lpr, g.rpp);
        });
    });
}

int tsgu_gmres_subtract(int vtype, int64_t n, int64_t p, int k, const void* w, const void* basis, int64_t slab, const void* coef,
                        void* out, void* partial, const int* flags, int inner, int device, void* stream) {
    if (!block_args_ok(n, p, k, slab) || !w || !basis || !coef || !out || !partial || !flags) return TSGU_ERR_BAD_ARG;
    if (!(aligned16(w) && aligned16(basis) && aligned16(out))) return TSGU_ERR_BAD_ARG;
    if (const int rc = lanes_cover(vtype, n, p)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        return launch_lanes<V>(n, p, gmres_subtract_kernel<V, 1>, gmres_subtract_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
            return launch(kern, g.blocks, s, n, p, k, (const V*)w, (const V*)basis, slab, (const V*)coef, (V*)out, (V*)partial, flags,
                          inner, g.lpr, g.rpp);
        });
    });
}

int tsgu_gmres_scale(int vtype, int64_t n, int64_t p, const void* w, const void* hnorm, void* out, const int* flags, int inner,
                     int device, void* stream) {
    if (n <= 0 || p <= 0 || !w || !hnorm || !out || !flags) return TSGU_ERR_BAD_ARG;
    if (!(aligned16(w) && aligned16(out))) return TSGU_ERR_BAD_ARG;
    if (const int rc = lanes_cover(vtype, n, p)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        return launch_lanes<V>(n, p, gmres_scale_kernel<V, 1>, gmres_scale_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
            return launch(kern, g.blocks, s, n, p, (const V*)w, (const V*)hnorm, (V*)out, flags, inner, g.lpr, g.rpp);
        });
    });
}

int tsgu_gmres_scalar(int vtype, int phase, int j, int m, const void* partial, int64_t n_partial, void* fold, void* scal, int* flags,
                      double abstol, double reltol, int maxiter, int64_t p, int device, void* stream) {
    if (!scal || !flags || p <= 0 || phase < kGmresStart || phase > kGmresSolve || m < 1 || m > kGmresCap) return TSGU_ERR_BAD_ARG;
    const bool reads = phase != kGmresSolve;
    const bool step = phase >= kGmresH1 && phase <= kGmresRotate;
    if (reads && (!partial || n_partial < 1)) return TSGU_ERR_BAD_ARG;
    if (step && (j < 0 || j >= m)) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        const int64_t stride = (phase == kGmresH1 || phase == kGmresH2) ? (int64_t)(j + 2) * p : p;
        const V* src = nullptr;
        int64_t rows = 0;
        if (reads)
            if (const int rc = fold_partials<V>(partial, n_partial, stride, fold, true, flags, s, src, rows)) return rc;
        return launch(gmres_scalar_kernel<V>, 1, s, phase, j, m, src, rows, stride, p, (V*)scal, flags, (V)abstol, (V)reltol, maxiter);
    });
}

int tsgu_gmres_update(int vtype, int64_t n, int64_t p, int k, void* x, const void* basis, int64_t slab, const void* y,
                      const int* flags, int device, void* stream) {
    if (!block_args_ok(n, p, k, slab) || !x || !basis || !y || !flags) return TSGU_ERR_BAD_ARG;
    if (!(aligned16(x) && aligned16(basis))) return TSGU_ERR_BAD_ARG;
    if (const int rc = lanes_cover(vtype, n, p)) return rc;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        return launch_lanes<V>(n, p, gmres_update_kernel<V, 1>, gmres_update_kernel<V, wide>, [&](auto kern, const VecGeom& g) {
            return launch(kern, g.blocks, s, n, p, k, (V*)x, (const V*)basis, slab, (const V*)y, flags, g.lpr, g.rpp);
        });
    });
}

}  // extern "C"
