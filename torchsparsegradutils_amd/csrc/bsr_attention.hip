// Block-sparse attention: the extern "C" entry points of include/tsgu_hip_bsr_attention.h (kernels: bsr_attention_impl.h, one
// instantiation file per value type).
#include "bsr_attention_impl.h"
#include "bsr_host.h"

#include "../../include/tsgu_hip_bsr_attention.h"

using namespace tsgu;

namespace {

bool geometry_ok(int heads, int d, int64_t bh, int64_t bw) {
    return heads >= 1 && (d == 16 || d == 32 || d == 64 || d == 128) && bh >= 16 && bw >= 16 && bh % 16 == 0 && bw % 16 == 0;
}

void geometry_of(int vtype, int d, int* tile_rows, int* stage_keys) {
    if (vtype == TSGU_F64) bat_geometry<double>(d, tile_rows, stage_keys);
    else if (vtype == TSGU_BF16) bat_geometry<bf16_t>(d, tile_rows, stage_keys);
    else bat_geometry<float>(d, tile_rows, stage_keys);
}

// The host-side refusals the three launchers share, in the order the header states (the gathered dense operands are among
// `stored`: null is allowed there).
int bat_check(int vtype, int itype, int64_t nrb, int64_t ncb, int64_t nnzb, int64_t bh, int64_t bw, int heads, int d,
              std::initializer_list<const void*> always, std::initializer_list<const void*> stored, std::initializer_list<Dense> dense) {
    if (const int rc = bsr_check_args(vtype, itype, nnzb, always, stored)) return rc;
    if (nrb < 0 || ncb < 0 || nnzb < 0 || !geometry_ok(heads, d, bh, bw)) return TSGU_ERR_BAD_ARG;
    const int64_t width = (int64_t)heads * d;
    for (const Dense& o : dense) {
        if (!o.ptr) continue;
        if (o.ld < width) return TSGU_ERR_BAD_ARG;
        if (!aligned16(o.ptr) || (o.ld * elem_bytes(vtype)) % 16) return TSGU_ERR_BAD_ARG;      // rows are read in 16-byte lanes
    }
    return bsr_check_sizes(nrb, ncb, nnzb, bh, bw, dense, true);
}

struct Call {
    int mode, vtype, itype, heads, d;
    int64_t n_groups, bh, bw;
    const void *ptr, *idx, *perm, *bias, *Q, *K, *V, *dO, *O;
    void *out0, *out1, *Oacc, *lse, *delta, *dA;
    int64_t ldq, ldk, ldv, lddo, ldo, ld0, ld1;
    double scale;
};

int bat_run(const Call& c, int device, void* stream) {
    if (c.n_groups == 0) return TSGU_OK;
    int T = 0, S = 0;
    geometry_of(c.vtype, c.d, &T, &S);
    const bool cols = c.mode == kBatCols;
    const int64_t oh = cols ? c.bw : c.bh;
    const BsrSplit split = bsr_tile_split(oh, T, c.n_groups);
    const int heads_y = c.mode == kBatRows && c.dA ? 1 : c.heads;      // dA: the workgroup sums the heads itself
    if (split.tiles > kI31 / heads_y) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(c.vtype, [&](auto v) {
        using V = decltype(v);
        using Acc = typename MfmaT<V>::Part;
        BsrAttn<V> P{};
        P.ptr = c.ptr, P.idx = c.idx, P.perm = c.perm;
        P.val = static_cast<const V*>(c.bias);
        P.Q = static_cast<const V*>(c.Q), P.K = static_cast<const V*>(c.K), P.Vv = static_cast<const V*>(c.V);
        P.dO = static_cast<const V*>(c.dO), P.O = static_cast<const Acc*>(c.O);
        P.out0 = static_cast<V*>(c.out0), P.out1 = static_cast<V*>(c.out1);
        P.Oacc = static_cast<Acc*>(c.Oacc), P.lse = static_cast<Acc*>(c.lse), P.delta = static_cast<Acc*>(c.delta), P.dA = static_cast<Acc*>(c.dA);
        P.ldq = c.ldq, P.ldk = c.ldk, P.ldv = c.ldv, P.lddo = c.lddo, P.ldo = c.ldo, P.ld0 = c.ld0, P.ld1 = c.ld1;
        P.n_groups = c.n_groups, P.bh = c.bh, P.bw = c.bw;
        P.oh = oh, P.kb = cols ? c.bh : c.bw;
        P.per_tile = split.per_tile, P.pieces = split.pieces;
        P.heads = c.heads, P.heads_y = heads_y;
        P.i64 = c.itype == TSGU_I64;
        P.scale = (Acc)c.scale;
        return bat_dispatch<V>(c.mode, c.d, P, split.tiles * heads_y, s);
    });
}

}  // namespace

extern "C" {

int tsgu_bsr_attention_supported(int vtype, int heads, int d, int64_t bh, int64_t bw) {
    return elem_bytes(vtype) && geometry_ok(heads, d, bh, bw) ? 1 : 0;
}

int tsgu_bsr_attention_geometry(int vtype, int heads, int d, int64_t bh, int64_t bw, int* tile_rows, int* stage_keys) {
    if (!tile_rows || !stage_keys) return TSGU_ERR_BAD_ARG;
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (!geometry_ok(heads, d, bh, bw)) return TSGU_ERR_BAD_ARG;
    geometry_of(vtype, d, tile_rows, stage_keys);
    return TSGU_OK;
}

int tsgu_bsr_attention(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                       const void* ptr, const void* idx, const void* bias, const void* Q, int64_t ldq, const void* K, int64_t ldk,
                       const void* V, int64_t ldv, int heads, int d, double scale, void* O, int64_t ldo, void* lse, void* O_acc,
                       int device, void* stream) {
    if (const int rc = bat_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, heads, d, {ptr, Q, O, lse}, {idx, K, V},
                                 {{Q, ldq}, {K, ldk}, {V, ldv}, {O, ldo}}))
        return rc;
    Call c{};
    c.mode = kBatFwd, c.vtype = vtype, c.itype = itype, c.heads = heads, c.d = d;
    c.n_groups = n_block_rows, c.bh = bh, c.bw = bw;
    c.ptr = ptr, c.idx = idx, c.bias = bias, c.Q = Q, c.K = K, c.V = V;
    c.out0 = O, c.lse = lse, c.Oacc = O_acc;
    c.ldq = ldq, c.ldk = ldk, c.ldv = ldv, c.ld0 = ldo;
    c.scale = scale;
    return bat_run(c, device, stream);
}

int tsgu_bsr_attention_backward_rows(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh,
                                     int64_t bw, const void* ptr, const void* idx, const void* bias, const void* Q, int64_t ldq,
                                     const void* K, int64_t ldk, const void* V, int64_t ldv, const void* dO, int64_t lddo,
                                     const void* O_acc, int64_t ldo, const void* lse, int heads, int d, double scale, void* dQ,
                                     int64_t lddq, void* delta, void* dA, int device, void* stream) {
    if (const int rc = bat_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, heads, d, {ptr, Q, dO, O_acc, lse, dQ, delta},
                                 {idx, K, V}, {{Q, ldq}, {K, ldk}, {V, ldv}, {dO, lddo}, {O_acc, ldo}, {dQ, lddq}}))
        return rc;
    Call c{};
    c.mode = kBatRows, c.vtype = vtype, c.itype = itype, c.heads = heads, c.d = d;
    c.n_groups = n_block_rows, c.bh = bh, c.bw = bw;
    c.ptr = ptr, c.idx = idx, c.bias = bias, c.Q = Q, c.K = K, c.V = V, c.dO = dO, c.O = O_acc;
    c.out0 = dQ, c.lse = const_cast<void*>(lse), c.delta = delta, c.dA = dA;
    c.ldq = ldq, c.ldk = ldk, c.ldv = ldv, c.lddo = lddo, c.ldo = ldo, c.ld0 = lddq;
    c.scale = scale;
    return bat_run(c, device, stream);
}

int tsgu_bsr_attention_backward_cols(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh,
                                     int64_t bw, const void* tptr, const void* tidx, const void* perm, const void* bias,
                                     const void* Q, int64_t ldq, const void* K, int64_t ldk, const void* V, int64_t ldv,
                                     const void* dO, int64_t lddo, const void* lse, const void* delta, int heads, int d,
                                     double scale, void* dK, int64_t lddk, void* dV, int64_t lddv, int device, void* stream) {
    if (const int rc = bat_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, heads, d, {tptr, K, V, dK, dV},
                                 {tidx, perm, Q, dO, lse, delta}, {{Q, ldq}, {K, ldk}, {V, ldv}, {dO, lddo}, {dK, lddk}, {dV, lddv}}))
        return rc;
    Call c{};
    c.mode = kBatCols, c.vtype = vtype, c.itype = itype, c.heads = heads, c.d = d;
    c.n_groups = n_block_cols, c.bh = bh, c.bw = bw;
    c.ptr = tptr, c.idx = tidx, c.perm = perm, c.bias = bias, c.Q = Q, c.K = K, c.V = V, c.dO = dO;
    c.out0 = dK, c.out1 = dV, c.lse = const_cast<void*>(lse), c.delta = const_cast<void*>(delta);
    c.ldq = ldq, c.ldk = ldk, c.ldv = ldv, c.lddo = lddo, c.ld0 = lddk, c.ld1 = lddv;
    c.scale = scale;
    return bat_run(c, device, stream);
}

}  // extern "C"
