// Attention over a sparse pattern: instantiations (fp32, fp64, bf16 × int32, int64 × forward, row pass, column pass) and the
// extern "C" entry points of include/tsgu_hip_attention.h.
#include "attention_impl.h"

#include "../../include/tsgu_hip_attention.h"

using namespace tsgu;

namespace {

constexpr int64_t kI31 = 0x7fffffffLL;

// A dense operand [rows, heads·d]; `needed`: false for the gathered side of a pattern without entries, which is never dereferenced
struct Dense {
    const void* ptr;
    int64_t ld;
    bool needed = true;
};

int elem_bytes(int vtype) { return vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 8 : vtype == TSGU_BF16 ? 2 : 0; }

AttnGeom geom_of(int vtype, int heads, int d) {
    if (vtype == TSGU_F64) return attn_geom<double>(heads, d);
    if (vtype == TSGU_BF16) return attn_geom<bf16_t>(heads, d);
    return attn_geom<float>(heads, d);
}

// The host-side refusals all three entries share, in the order of the header; `n_groups`: the walked side.
int attn_check(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_groups, const void* ptr, const void* idx,
               int heads, int d, std::initializer_list<Dense> dense, std::initializer_list<const void*> others) {
    const int eb = elem_bytes(vtype);
    if (!eb || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || heads < 0 || d < 0) return TSGU_ERR_BAD_ARG;
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
    const int64_t rpb = geom_of(vtype, heads, d).rows_per_block();
    if ((n_groups + rpb - 1) / rpb > kI31) return TSGU_ERR_TOO_LARGE;
    return TSGU_OK;
}

template <int MODE>
int attn_launch(int vtype, int itype, AttnParams P, int device, void* stream) {
    if (P.n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        const AttnGeom g = attn_geom<V>(P.heads, P.d);
        P.cl = g.cl;
        P.ep = g.ep;
        P.dl = g.dl;
        P.tiles = g.tiles;
        const int64_t rpb = g.rows_per_block();
        return launch(attn_kernel<V, I, MODE>, (P.n_groups + rpb - 1) / rpb, s, P);
    });
}

AttnParams attn_params(int64_t n_groups, const void* ptr, const void* idx, const void* perm, const void* bias, int heads, int d,
                       double scale) {
    AttnParams P{};
    P.n_groups = n_groups;
    P.ptr = ptr;
    P.idx = idx;
    P.perm = perm;
    P.bias = bias;
    P.heads = heads;
    P.d = d;
    P.width = heads * d;
    P.scale = scale;
    return P;
}

}  // namespace

extern "C" {

int tsgu_csr_attention_supported(int vtype, int heads, int d) { return elem_bytes(vtype) && attn_supported(heads, d) ? 1 : 0; }

int tsgu_csr_attention_geometry(int vtype, int heads, int d, int* entry_lanes, int* rows_per_block, int* stage_entries) {
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (!attn_supported(heads, d) || !entry_lanes || !rows_per_block || !stage_entries) return TSGU_ERR_BAD_ARG;
    const AttnGeom g = geom_of(vtype, heads, d);
    *entry_lanes = g.ep;
    *rows_per_block = g.rows_per_block();
    *stage_entries = kAttnStage;
    return TSGU_OK;
}

int tsgu_csr_attention(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                       const void* perm, const void* bias, const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V,
                       int64_t ldv, int heads, int d, double scale, void* O, int64_t ldo, void* lse, int device, void* stream) {
    const bool far = nnz > 0;
    if (const int rc = attn_check(vtype, itype, n_rows, n_cols, nnz, n_rows, ptr, idx, heads, d,
                                  {{Q, ldq}, {K, ldk, far}, {V, ldv, far}, {O, ldo}}, {lse}))
        return rc;
    AttnParams P = attn_params(n_rows, ptr, idx, perm, bias, heads, d, scale);
    P.own0 = Q, P.ld_own0 = ldq;
    P.far0 = K, P.ld_far0 = ldk;
    P.far1 = V, P.ld_far1 = ldv;
    P.out0 = O, P.ld_out0 = ldo;
    P.lse = lse;
    return attn_launch<kAttnFwd>(vtype, itype, P, device, stream);
}

int tsgu_csr_attention_backward_rows(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                     const void* idx, const void* perm, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* lse, int heads, int d, double scale, void* dQ, int64_t lddq, void* delta,
                                     void* dA, int device, void* stream) {
    const bool far = nnz > 0;
    if (const int rc = attn_check(vtype, itype, n_rows, n_cols, nnz, n_rows, ptr, idx, heads, d,
                                  {{Q, ldq}, {K, ldk, far}, {V, ldv, far}, {dO, lddo}, {dQ, lddq}},
                                  {lse, delta}))
        return rc;
    AttnParams P = attn_params(n_rows, ptr, idx, perm, bias, heads, d, scale);
    P.own0 = Q, P.ld_own0 = ldq;
    P.own1 = dO, P.ld_own1 = lddo;
    P.far0 = K, P.ld_far0 = ldk;
    P.far1 = V, P.ld_far1 = ldv;
    P.out0 = dQ, P.ld_out0 = lddq;
    P.lse = const_cast<void*>(lse);
    P.delta = delta;
    P.dA = dA;
    return attn_launch<kAttnBwdRows>(vtype, itype, P, device, stream);
}

int tsgu_csr_attention_backward_cols(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                     const void* tidx, const void* tperm, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* lse, const void* delta, int heads, int d, double scale, void* dK, int64_t lddk,
                                     void* dV, int64_t lddv, int device, void* stream) {
    const bool far = nnz > 0;
    if (const int rc = attn_check(vtype, itype, n_rows, n_cols, nnz, n_cols, tptr, tidx, heads, d,
                                  {{K, ldk}, {V, ldv}, {Q, ldq, far}, {dO, lddo, far}, {dK, lddk}, {dV, lddv}},
                                  {far ? lse : tptr, far ? delta : tptr}))
        return rc;
    AttnParams P = attn_params(n_cols, tptr, tidx, tperm, bias, heads, d, scale);
    P.own0 = K, P.ld_own0 = ldk;
    P.own1 = V, P.ld_own1 = ldv;
    P.far0 = Q, P.ld_far0 = ldq;
    P.far1 = dO, P.ld_far1 = lddo;
    P.out0 = dK, P.ld_out0 = lddk;
    P.out1 = dV, P.ld_out1 = lddv;
    P.lse = const_cast<void*>(lse);
    P.delta = const_cast<void*>(delta);
    return attn_launch<kAttnBwdCols>(vtype, itype, P, device, stream);
}

}  // extern "C"
