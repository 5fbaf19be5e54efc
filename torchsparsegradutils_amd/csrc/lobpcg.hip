// Entry points of the tall-skinny dense kernels of the LOBPCG loop (tsgu_hip_lobpcg.h; kernels: lobpcg_impl.h).
#include "lobpcg_impl.h"

#include "tsgu_hip_lobpcg.h"

namespace tsgu {

// a device pointer: not NULL, aligned to the element
inline bool tall_ptr_ok(const void* p, int size) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(size - 1)) == 0; }

inline int tall_value_size(int vtype) { return vtype == TSGU_F32 ? 4 : (vtype == TSGU_F64 ? 8 : 0); }

// status of a width in [1, limit] with its leading dimension
inline int tall_width(int64_t w, int64_t ld, int64_t limit) {
    if (w <= 0) return TSGU_ERR_BAD_ARG;
    if (w > limit) return TSGU_ERR_TOO_LARGE;
    return ld < w ? TSGU_ERR_BAD_ARG : TSGU_OK;
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_tall_geometry(int vtype, int64_t n, int64_t a, int64_t b, int* kmax, int* wmax, int* rows_per_workgroup,
                       int64_t* workspace_bytes) {
    if (!kmax || !wmax || !rows_per_workgroup || !workspace_bytes) return TSGU_ERR_BAD_ARG;
    const int size = tall_value_size(vtype);
    if (size == 0) return TSGU_ERR_BAD_DTYPE;
    if (n < 0 || a < 0 || b < 0) return TSGU_ERR_BAD_ARG;
    if (a > kTallW || b > kTallW) return TSGU_ERR_TOO_LARGE;
    *kmax = kTallK;
    *wmax = kTallW;
    *rows_per_workgroup = kTallRows;
    *workspace_bytes = tall_partials(n) * a * b * size;
    return TSGU_OK;
}

int tsgu_tall_gram(int vtype, int64_t n, int64_t a, int64_t b, const void* y, int64_t ldy, const void* z, int64_t ldz, void* c,
                   int64_t ldc, void* workspace, int64_t workspace_bytes, int workgroups, int device, void* stream) {
    const int size = tall_value_size(vtype);
    if (size == 0) return TSGU_ERR_BAD_DTYPE;
    if (n <= 0 || workgroups < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = tall_width(a, ldy, kTallW)) return rc;
    if (const int rc = tall_width(b, ldz, kTallW)) return rc;
    if (ldc < b) return TSGU_ERR_BAD_ARG;
    if (!tall_ptr_ok(y, size) || !tall_ptr_ok(z, size) || !tall_ptr_ok(c, size) || !tall_ptr_ok(workspace, size)) return TSGU_ERR_BAD_ARG;
    if (workspace_bytes < tall_partials(n) * a * b * size) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    GramParams P{};
    P.n = n;
    P.chunks = tall_chunks(n);
    P.a = (int)a;
    P.b = (int)b;
    P.same = y == z && ldy == ldz && a == b;
    P.y = y;
    P.z = z;
    P.ldy = ldy;
    P.ldz = ldz;
    P.partial = workspace;
    const int64_t grid = tall_grid(P.chunks, workgroups, device);
    return with_value_type<float, double>(vtype, [&](auto v) {
        using V = decltype(v);
        const int rc = with_gram_tile(a > b ? a : b, [&](auto nt) { return launch(tall_gram_kernel<V, decltype(nt)::value>, grid, s, P); });
        if (rc) return rc;
        return tall_fold<V>(static_cast<V*>(workspace), P.chunks, a * b, static_cast<V*>(c), (int)b, ldc, s);
    });
}

int tsgu_tall_combine(int vtype, int64_t n, int n_in, const void* const* s, const int64_t* s_width, const int64_t* s_ld, int n_out,
                      void* const* out, const int64_t* out_width, const int64_t* out_ld, const double* beta, const void* const* coef,
                      const int64_t* coef_ld, int workgroups, int device, void* stream) {
    const int size = tall_value_size(vtype);
    if (size == 0) return TSGU_ERR_BAD_DTYPE;
    if (n <= 0 || workgroups < 0 || n_in < 1 || n_in > kTallIn || n_out < 1 || n_out > kTallOut) return TSGU_ERR_BAD_ARG;
    if (!s || !s_width || !s_ld || !out || !out_width || !out_ld || !coef || !coef_ld) return TSGU_ERR_BAD_ARG;
    CombineParams P{};
    P.n = n;
    P.n_in = n_in;
    P.n_out = n_out;
    for (int i = 0; i < n_in; ++i) {
        if (const int rc = tall_width(s_width[i], s_ld[i], kTallK)) return rc;
        if (!tall_ptr_ok(s[i], size)) return TSGU_ERR_BAD_ARG;
        P.s[i] = s[i];
        P.s_ld[i] = s_ld[i];
        P.s_w[i] = (int)s_width[i];
    }
    for (int t = 0; t < n_out; ++t) {
        if (const int rc = tall_width(out_width[t], out_ld[t], kTallK)) return rc;
        if (!tall_ptr_ok(out[t], size)) return TSGU_ERR_BAD_ARG;
        P.out[t] = out[t];
        P.out_ld[t] = out_ld[t];
        P.out_w[t] = (int)out_width[t];
        P.beta[t] = beta ? beta[t] : 0.0;
        P.has_beta[t] = P.beta[t] != 0.0;
        for (int i = 0; i < n_in; ++i)
            if (tall_views_meet(out[t], out_width[t], out_ld[t], s[i], s_width[i], s_ld[i], n, size)) return TSGU_ERR_BAD_ARG;
        for (int u = 0; u < t; ++u)
            if (tall_views_meet(out[t], out_width[t], out_ld[t], out[u], out_width[u], out_ld[u], n, size)) return TSGU_ERR_BAD_ARG;
    }
    for (int t = 0; t < n_out; ++t) {
        for (int i = 0; i < n_in; ++i) {
            const void* c = coef[t * n_in + i];
            const int64_t ld = coef_ld[t * n_in + i];
            P.slot[t][i] = -1;
            if (!c) continue;
            if (!tall_ptr_ok(c, size) || ld < out_width[t]) return TSGU_ERR_BAD_ARG;
            int u = 0;
            while (u < P.n_coef && !(P.coef[u] == c && P.coef_ld[u] == ld && P.coef_rows[u] == P.s_w[i] && P.coef_cols[u] == P.out_w[t])) ++u;
            if (u == P.n_coef) {
                if (u == kTallCoef) return TSGU_ERR_TOO_LARGE;
                P.coef[u] = c;
                P.coef_ld[u] = ld;
                P.coef_rows[u] = P.s_w[i];
                P.coef_cols[u] = P.out_w[t];
                ++P.n_coef;
            }
            P.slot[t][i] = u;
        }
    }
    if (const int rc = set_device(device)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_value_type<float, double>(vtype, [&](auto v) {
        using V = decltype(v);
        int64_t widest = 0;
        for (int i = 0; i < n_in; ++i) widest = s_width[i] > widest ? s_width[i] : widest;
        for (int t = 0; t < n_out; ++t) widest = out_width[t] > widest ? out_width[t] : widest;
        return with_row_lanes(widest, [&](auto wb) {
            constexpr int WB = decltype(wb)::value;
            constexpr int TILE = (kBlock / WB) * combine_rpt<V>();
            P.tiles = (n + TILE - 1) / TILE;
            return launch(tall_combine_kernel<V, WB>, tall_grid(P.tiles, workgroups, device), st, P);
        });
    });
}

int tsgu_lobpcg_residual(int vtype, int64_t n, int64_t k, const void* ax, int64_t ldax, const void* x, int64_t ldx, const void* lam,
                         void* r, int64_t ldr, void* sumsq, void* workspace, int64_t workspace_bytes, int workgroups, int device,
                         void* stream) {
    const int size = tall_value_size(vtype);
    if (size == 0) return TSGU_ERR_BAD_DTYPE;
    if (n <= 0 || workgroups < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = tall_width(k, ldax, kTallK)) return rc;
    if (ldx < k || ldr < k) return TSGU_ERR_BAD_ARG;
    if (!tall_ptr_ok(ax, size) || !tall_ptr_ok(x, size) || !tall_ptr_ok(lam, size) || !tall_ptr_ok(r, size) || !tall_ptr_ok(sumsq, size) || !tall_ptr_ok(workspace, size))
        return TSGU_ERR_BAD_ARG;
    if (workspace_bytes < tall_partials(n) * k * size) return TSGU_ERR_BAD_ARG;
    if (tall_views_meet(r, k, ldr, ax, k, ldax, n, size) || tall_views_meet(r, k, ldr, x, k, ldx, n, size)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    ResidualParams P{};
    P.n = n;
    P.chunks = tall_chunks(n);
    P.k = (int)k;
    P.ax = ax;
    P.x = x;
    P.lam = lam;
    P.r = r;
    P.ldax = ldax;
    P.ldx = ldx;
    P.ldr = ldr;
    P.partial = workspace;
    const int64_t grid = tall_grid(P.chunks, workgroups, device);
    return with_value_type<float, double>(vtype, [&](auto v) {
        using V = decltype(v);
        const int rc = with_row_lanes(k, [&](auto wb) { return launch(lobpcg_residual_kernel<V, decltype(wb)::value>, grid, s, P); });
        if (rc) return rc;
        return tall_fold<V>(static_cast<V*>(workspace), P.chunks, k, static_cast<V*>(sumsq), (int)k, k, s);
    });
}

}  // extern "C"
