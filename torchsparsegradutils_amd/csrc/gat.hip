// Graph attention over a sparse pattern: instantiations (fp32, fp64, bf16 × int32, int64 × GAT forward, GATv2 forward, row pass
// and column pass of both kinds, the datt fold) and the extern "C" entry points of tsgu_hip_gat.h.
#include "gat_impl.h"

#include "../../include/tsgu_hip_gat.h"

using namespace tsgu;

namespace {

constexpr int64_t kI31 = 0x7fffffffLL;

// A dense operand [rows, heads·d]; `needed`: false for an operand this kind (or a pattern without entries) never dereferences
struct Dense {
    const void* ptr;
    int64_t ld;
    bool needed = true;
};

int elem_bytes(int vtype) { return vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 8 : vtype == TSGU_BF16 ? 2 : 0; }

struct Geom {
    AttnGeom g;
    int stage, ht;
};

Geom geom_of(int vtype, int kind, int heads, int d) {
    Geom r;
    if (vtype == TSGU_F64) {
        r.g = attn_geom<double>(heads, d);
        r.ht = gat_tile_heads<double>(r.g, heads), r.stage = gat_stage<double>(r.g, heads);
    } else if (vtype == TSGU_BF16) {
        r.g = attn_geom<bf16_t>(heads, d);
        r.ht = gat_tile_heads<bf16_t>(r.g, heads), r.stage = gat_stage<bf16_t>(r.g, heads);
    } else {
        r.g = attn_geom<float>(heads, d);
        r.ht = gat_tile_heads<float>(r.g, heads), r.stage = gat_stage<float>(r.g, heads);
    }
    if (kind == kGatV2) r.stage = kAttnStage;
    return r;
}

// The host-side refusals the entries share; `n_groups`: the walked side.  `others`: arrays that must be there when the walked side
// is not empty.
int gat_check(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_groups, const void* ptr,
              const void* idx, int heads, int d, double slope, std::initializer_list<Dense> dense,
              std::initializer_list<const void*> others) {
    const int eb = elem_bytes(vtype);
    if (!eb || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (kind != kGatV1 && kind != kGatV2) return TSGU_ERR_BAD_ARG;
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || heads < 0 || d < 0 || !(slope == slope) || slope - slope != 0.0) return TSGU_ERR_BAD_ARG;
    if (!attn_supported(heads, d)) return TSGU_ERR_BAD_ARG;
    if (n_groups == 0) return TSGU_OK;
    if (!ptr || (nnz > 0 && !idx)) return TSGU_ERR_BAD_ARG;
    for (const void* p : others)
        if (!p) return TSGU_ERR_BAD_ARG;
    const int64_t width = (int64_t)heads * d;
    for (const Dense& o : dense) {
        if (!o.needed) continue;
        if (!o.ptr || o.ld < width) return TSGU_ERR_BAD_ARG;
        if (!aligned16(o.ptr) || (o.ld * eb) % 16) return TSGU_ERR_BAD_ARG;    // rows are read and written in 16-byte lanes
        if (o.ld > kI31) return TSGU_ERR_TOO_LARGE;
    }
    if (n_rows > kI31 || n_cols > kI31) return TSGU_ERR_TOO_LARGE;
    const int64_t rpb = geom_of(vtype, kind, heads, d).g.rows_per_block();
    if ((n_groups + rpb - 1) / rpb > kI31) return TSGU_ERR_TOO_LARGE;
    return TSGU_OK;
}

template <int MODE>
int gat_launch(int vtype, int itype, int kind, GatParams P, int device, void* stream) {
    if (P.n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        const AttnGeom g = attn_geom<V>(P.heads, P.d);
        P.cl = g.cl, P.ep = g.ep, P.dl = g.dl, P.tiles = g.tiles;
        P.ht = gat_tile_heads<V>(g, P.heads), P.stage = gat_stage<V>(g, P.heads);
        const int64_t rpb = g.rows_per_block(), blocks = (P.n_groups + rpb - 1) / rpb;
        if (kind == kGatV2) return launch(gat_pass_kernel<V, I, kGatV2, MODE>, blocks, s, P);
        if constexpr (MODE == kGatFwd) return launch(gat_fwd_kernel<V, I>, blocks, s, P);
        else return launch(gat_pass_kernel<V, I, kGatV1, MODE>, blocks, s, P);
    });
}

GatParams gat_params(int64_t n_groups, const void* ptr, const void* idx, const void* perm, const void* bias, const void* att, int heads,
                     int d, double slope) {
    GatParams P{};
    P.n_groups = n_groups;
    P.ptr = ptr, P.idx = idx, P.perm = perm, P.bias = bias, P.att = att;
    P.heads = heads, P.d = d, P.width = heads * d;
    P.slope = slope;
    return P;
}

}  // namespace

extern "C" {

int tsgu_gat_geometry(int vtype, int kind, int heads, int d, int* rows_per_block, int* stage_entries, int* tile_width) {
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if ((kind != kGatV1 && kind != kGatV2) || !attn_supported(heads, d) || !rows_per_block || !stage_entries || !tile_width)
        return TSGU_ERR_BAD_ARG;
    const Geom r = geom_of(vtype, kind, heads, d);
    *rows_per_block = r.g.rows_per_block();
    *stage_entries = r.stage;
    *tile_width = r.g.cl * (16 / elem_bytes(vtype));
    return TSGU_OK;
}

int tsgu_csr_gat_forward(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                         const void* perm, const void* bias, const void* s_dst, const void* s_src, const void* X_dst, int64_t ldxd,
                         const void* X_src, int64_t ldxs, const void* att, int heads, int d, double slope, void* O, int64_t ldo,
                         void* lse, int device, void* stream) {
    const bool far = nnz > 0, v2 = kind == kGatV2;
    if (const int rc = gat_check(vtype, itype, kind, n_rows, n_cols, nnz, n_rows, ptr, idx, heads, d, slope,
                                 {{X_dst, ldxd, v2}, {X_src, ldxs, far}, {att, heads * (int64_t)d, v2}, {O, ldo}},
                                 {lse, v2 ? lse : s_dst, v2 || !far ? lse : s_src}))
        return rc;
    GatParams P = gat_params(n_rows, ptr, idx, perm, bias, att, heads, d, slope);
    P.s_own = s_dst, P.s_far = s_src;
    P.x_own = X_dst, P.ld_x_own = ldxd;
    P.x_far = X_src, P.ld_x_far = ldxs;
    P.out0 = O, P.ld_out0 = ldo;
    P.lse = lse;
    return gat_launch<kGatFwd>(vtype, itype, kind, P, device, stream);
}

int tsgu_csr_gat_backward_rows(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                               const void* idx, const void* perm, const void* bias, const void* s_dst, const void* s_src,
                               const void* X_dst, int64_t ldxd, const void* X_src, int64_t ldxs, const void* att, const void* dO,
                               int64_t lddo, const void* lse, int heads, int d, double slope, void* d_dst, int64_t ldd, void* delta,
                               void* dA, void* partials, int64_t n_partials, int device, void* stream) {
    const bool far = nnz > 0, v2 = kind == kGatV2;
    if (const int rc = gat_check(vtype, itype, kind, n_rows, n_cols, nnz, n_rows, ptr, idx, heads, d, slope,
                                 {{X_dst, ldxd, v2}, {X_src, ldxs, far}, {att, heads * (int64_t)d, v2}, {dO, lddo}, {d_dst, ldd, v2}},
                                 {lse, delta, d_dst, v2 ? partials : s_dst, v2 || !far ? lse : s_src}))
        return rc;
    if (v2 && n_rows > 0) {
        const int64_t rpb = geom_of(vtype, kind, heads, d).g.rows_per_block();
        if (n_partials != (n_rows + rpb - 1) / rpb) return TSGU_ERR_BAD_ARG;
    }
    GatParams P = gat_params(n_rows, ptr, idx, perm, bias, att, heads, d, slope);
    P.s_own = s_dst, P.s_far = s_src;
    P.x_own = X_dst, P.ld_x_own = ldxd;
    P.x_far = X_src, P.ld_x_far = ldxs;
    P.g_own = dO, P.ld_g_own = lddo;
    P.out0 = v2 ? d_dst : nullptr, P.ld_out0 = ldd;
    P.out_s = v2 ? nullptr : d_dst;
    P.lse = const_cast<void*>(lse);
    P.delta = delta;
    P.dA = dA;
    P.partials = partials;
    return gat_launch<kGatBwdRows>(vtype, itype, kind, P, device, stream);
}

int tsgu_csr_gat_backward_cols(int vtype, int itype, int kind, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                               const void* tidx, const void* tperm, const void* bias, const void* s_dst, const void* s_src,
                               const void* X_dst, int64_t ldxd, const void* X_src, int64_t ldxs, const void* att, const void* dO,
                               int64_t lddo, const void* lse, const void* delta, int heads, int d, double slope, void* d_src,
                               int64_t ldds, void* ds_src, int device, void* stream) {
    const bool far = nnz > 0, v2 = kind == kGatV2;
    if (const int rc = gat_check(vtype, itype, kind, n_rows, n_cols, nnz, n_cols, tptr, tidx, heads, d, slope,
                                 {{X_src, ldxs}, {X_dst, ldxd, v2 && far}, {att, heads * (int64_t)d, v2}, {dO, lddo, far}, {d_src, ldds}},
                                 {far ? lse : tptr, far ? delta : tptr, v2 ? tptr : s_src, v2 ? tptr : ds_src,
                                  v2 || !far ? tptr : s_dst}))
        return rc;
    GatParams P = gat_params(n_cols, tptr, tidx, tperm, bias, att, heads, d, slope);
    P.s_own = s_src, P.s_far = s_dst;
    P.x_own = X_src, P.ld_x_own = ldxs;
    P.x_far = X_dst, P.ld_x_far = ldxd;
    P.g_far = dO, P.ld_g_far = lddo;
    P.out0 = d_src, P.ld_out0 = ldds;
    P.out_s = ds_src;
    P.lse = const_cast<void*>(lse);
    P.delta = const_cast<void*>(delta);
    return gat_launch<kGatBwdCols>(vtype, itype, kind, P, device, stream);
}

int tsgu_gat_fold(int vtype, const void* partials, int64_t n_partials, int heads, int d, void* datt, int device, void* stream) {
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (n_partials < 0 || !attn_supported(heads, d) || !datt || (n_partials > 0 && !partials)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int width = heads * d;
    const int64_t blocks = (width + kGatFoldCols - 1) / kGatFoldCols;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto v) {
        using V = decltype(v);
        using Acc = typename VT<V>::Acc;
        return launch(gat_fold_kernel<V>, blocks, s, static_cast<const Acc*>(partials), n_partials, width, static_cast<V*>(datt));
    });
}

}  // extern "C"
