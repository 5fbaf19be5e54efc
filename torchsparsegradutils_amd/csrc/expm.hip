// K12: entry points of the Chebyshev recurrence of sparse_expm_mm (expm_impl.h; contracts in tsgu_hip_expm.h).
#include "expm_impl.h"
#include "tsgu_hip_expm.h"

using namespace tsgu;

namespace {

inline bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// The lane geometry of an [n][p] array of the value type, or the status that refuses it.
inline int probe_geometry(int vtype, int64_t n, int64_t p, VecGeom& g) {
    const bool ok = vtype == TSGU_F32 ? geom_for<float>(n, p, true, g) : geom_for<double>(n, p, true, g);
    return ok && g.blocks <= 0x7fffffffLL ? TSGU_OK : TSGU_ERR_TOO_LARGE;
}

// f(std::bool_constant<b>{}) for a run-time b
template <typename F>
inline int with_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace

extern "C" {

int tsgu_expm_geometry(int vtype, int64_t n, int64_t p, int* time_cap, int* chunk_cap, int* plane_align, int64_t* rows_per_workgroup,
                       int64_t* workgroups) {
    if (!time_cap || !chunk_cap || !plane_align || !rows_per_workgroup || !workgroups || n <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    VecGeom g;
    if (const int rc = probe_geometry(vtype, n, p, g)) return rc;
    *time_cap = kChebTimeCap;
    *chunk_cap = kChebChunkCap;
    *plane_align = vtype == TSGU_F32 ? 4 : 2;
    *rows_per_workgroup = (int64_t)g.rpp * kPasses;
    *workgroups = g.blocks;
    return TSGU_OK;
}

int tsgu_cheb_step(int vtype, int64_t n, int64_t p, const void* prod, const void* x, void* prev, double alpha, double beta, double gamma,
                   const void* src, int src_slots, int src_slot, void* chunk, int chunk_slots, int slot, const int* flags, int device,
                   void* stream) {
    if (!x || !prev || !flags || n <= 0 || p <= 0) return TSGU_ERR_BAD_ARG;
    if (!prod && alpha != 0.0) return TSGU_ERR_BAD_ARG;
    if (src && (src_slots < 1 || src_slot < 0 || src_slot >= src_slots)) return TSGU_ERR_BAD_ARG;
    if (chunk && (chunk_slots < 1 || slot < 0 || slot >= chunk_slots)) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (!(aligned16(prod) && aligned16(x) && aligned16(prev) && aligned16(src) && aligned16(chunk) && aligned_to(flags, 4)))
        return TSGU_ERR_BAD_ARG;
    if (n > INT64_MAX / p) return TSGU_ERR_BAD_ARG;
    if ((src && src_slots > kChebChunkCap) || (chunk && chunk_slots > kChebChunkCap)) return TSGU_ERR_TOO_LARGE;
    VecGeom probe;
    if (const int rc = probe_geometry(vtype, n, p, probe)) return rc;
    if (n * p > INT64_MAX / kChebChunkCap) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        auto go = [&](auto kern, const VecGeom& g) -> int {
            return launch(kern, g.blocks, s, n, p, (const V*)prod, (const V*)x, (V*)prev, (V)alpha, (V)beta, (V)gamma, (const V*)src,
                          (int64_t)src_slots * p, (int64_t)src_slot * p, (V*)chunk, (int64_t)chunk_slots * p, (int64_t)slot * p, flags,
                          g.lpr, g.rpp);
        };
        return with_bool(prod != nullptr, [&](auto hp) -> int {
            return with_bool(src != nullptr, [&](auto hs) -> int {
                return with_bool(chunk != nullptr, [&](auto hc) -> int {
                    constexpr bool P = decltype(hp)::value, S = decltype(hs)::value, C = decltype(hc)::value;
                    return launch_lanes<V>(n, p, cheb_step_kernel<V, 1, P, S, C>, cheb_step_kernel<V, wide, P, S, C>, go);
                });
            });
        });
    });
}

int tsgu_cheb_combine(int vtype, int mode, int accumulate, int64_t n, int64_t p, int m, int T, void* chunk, const void* coef,
                      void* planes, int64_t plane_stride, const int* flags, int device, void* stream) {
    if (!chunk || !coef || !planes || !flags || n <= 0 || p <= 0 || m < 1 || T < 1) return TSGU_ERR_BAD_ARG;
    if ((mode != 0 && mode != 1) || (accumulate != 0 && accumulate != 1) || (mode == 1 && accumulate)) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    const size_t elem = vtype == TSGU_F64 ? 8 : 4;
    if (!(aligned16(chunk) && aligned_to(coef, elem) && aligned16(planes) && aligned_to(flags, 4))) return TSGU_ERR_BAD_ARG;
    if (n > INT64_MAX / p || plane_stride < n * p || ((plane_stride * (int64_t)elem) & 15)) return TSGU_ERR_BAD_ARG;
    if (m > kChebChunkCap || T > kChebTimeCap) return TSGU_ERR_TOO_LARGE;
    VecGeom probe;
    if (const int rc = probe_geometry(vtype, n, p, probe)) return rc;
    if (n * p > INT64_MAX / kChebChunkCap) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int tt = 1;
    while (tt < T) tt *= 2;
    return with_value_type(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        constexpr int wide = VT<V>::kWide;
        auto go = [&](auto kern, const VecGeom& g) -> int {
            return launch(kern, g.blocks, s, n, p, m, T, accumulate, (V*)chunk, (const V*)coef, (V*)planes, plane_stride, flags, g.lpr,
                          g.rpp);
        };
        int rc = TSGU_ERR_TOO_LARGE;
        dispatch_pow2<1, kChebTimeCap>(tt, [&](auto width) {
            constexpr int TT = decltype(width)::value;
            rc = mode == 0 ? launch_lanes<V>(n, p, cheb_combine_kernel<V, 1, TT, 0>, cheb_combine_kernel<V, wide, TT, 0>, go)
                           : launch_lanes<V>(n, p, cheb_combine_kernel<V, 1, TT, 1>, cheb_combine_kernel<V, wide, TT, 1>, go);
        });
        return rc;
    });
}

}  // extern "C"
