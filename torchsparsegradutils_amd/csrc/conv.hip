// neighbor_mm: the extern "C" entry points of include/tsgu_hip_conv.h (kernels: conv_impl.h).
#include "conv_impl.h"
#include "../../include/tsgu_hip_conv.h"

using namespace tsgu;

namespace {

constexpr int kGradWWorkgroups = 2048;     // split target of grad_w: about eight workgroups per compute unit
constexpr int64_t kGradWMinChunk = 256;    // rows; a multiple of every value type's stage

int64_t part_size(int vtype) { return vtype == TSGU_F64 ? 8 : 4; }

bool value_type_ok(int vtype) { return vtype == TSGU_F32 || vtype == TSGU_F64 || vtype == TSGU_BF16; }

// Rows of one grad_w chunk: the smallest power of two >= kGradWMinChunk at which the launch has at most kGradWWorkgroups workgroups.
int64_t gradw_chunk(int64_t n_out, int64_t k, int64_t d1, int64_t d2) {
    const int64_t per_chunk = k * ((d1 + kNmmGT - 1) / kNmmGT) * ((d2 + kNmmGT - 1) / kNmmGT);
    int64_t c = kGradWMinChunk;
    while (c < ((int64_t)1 << 40) && ((n_out + c - 1) / c) * per_chunk > kGradWWorkgroups) c <<= 1;
    return c;
}

}  // namespace

extern "C" {

int tsgu_neighbor_mm_geometry(int vtype, int64_t n_out, int64_t k, int64_t d1, int64_t d2, int64_t* tile_rows, int64_t* chunk_rows,
                              int64_t* chunks, int64_t* workspace_bytes) {
    if (n_out < 0 || k < 0 || d1 < 0 || d2 < 0 || !tile_rows || !chunk_rows || !chunks || !workspace_bytes) return TSGU_ERR_BAD_ARG;
    if (!value_type_ok(vtype)) return TSGU_ERR_BAD_DTYPE;
    const int64_t c = gradw_chunk(n_out, k, d1, d2);
    const int64_t nch = n_out > c ? (n_out + c - 1) / c : 1;
    const int64_t bytes = nch > 1 ? nch * k * d1 * d2 * part_size(vtype) : 0;
    *tile_rows = kNmmBM;
    *chunk_rows = c;
    *chunks = nch;
    *workspace_bytes = bytes > 16 ? bytes : 16;
    return TSGU_OK;
}

int tsgu_neighbor_mm(int vtype, int itype, int64_t n_in, int64_t n_out, int64_t k, int64_t d1, int64_t d2, const void* nbr,
                     const void* x, int64_t ldx, const void* w, int64_t w_stride0, int64_t w_stride1, int64_t w_stride2,
                     const void* bias, void* out, int64_t ldo, int device, void* stream) {
    if (n_in < 0 || n_out < 0 || k < 0 || d1 < 0 || d2 < 0) return TSGU_ERR_BAD_ARG;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (!value_type_ok(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (n_out == 0 || d2 == 0) return TSGU_OK;
    if (k == 0 || d1 == 0 || n_in == 0) return TSGU_ERR_BAD_ARG;                      // bias-only results need no launch
    if (!nbr || !x || !w || !out || ldx < d1 || ldo < d2) return TSGU_ERR_BAD_ARG;
    if (w_stride1 != 1 && w_stride2 != 1) return TSGU_ERR_BAD_ARG;                     // one of w[k]'s axes is contiguous
    if (w_stride0 < 0 || w_stride1 < 0 || w_stride2 < 0) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        NmmFwd<V> P{};
        P.nbr = nbr;
        P.x = static_cast<const V*>(x);
        P.w = static_cast<const V*>(w);
        P.bias = static_cast<const V*>(bias);
        P.out = static_cast<V*>(out);
        P.ldx = ldx;
        P.ldo = ldo;
        P.ws0 = w_stride0;
        P.ws1 = w_stride1;
        P.ws2 = w_stride2;
        P.n_in = n_in;
        P.n_out = n_out;
        P.K = k;
        P.d1 = d1;
        P.d2 = d2;
        return nmm_fwd_launch<V, decltype(i)>(P, s);
    });
}

int tsgu_neighbor_mm_grad_w(int vtype, int itype, int64_t n_in, int64_t n_out, int64_t k, int64_t d1, int64_t d2, const void* nbr,
                            const void* x, int64_t ldx, const void* g, int64_t ldg, void* grad_w, void* workspace,
                            int64_t workspace_bytes, int device, void* stream) {
    if (n_in < 0 || n_out < 0 || k < 0 || d1 < 0 || d2 < 0) return TSGU_ERR_BAD_ARG;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (k == 0 || d1 == 0 || d2 == 0) return value_type_ok(vtype) ? TSGU_OK : TSGU_ERR_BAD_DTYPE;
    int64_t tile = 0, c = 0, nch = 0, need = 0;
    if (const int rc = tsgu_neighbor_mm_geometry(vtype, n_out, k, d1, d2, &tile, &c, &nch, &need)) return rc;
    if (n_out == 0 || n_in == 0) return TSGU_ERR_BAD_ARG;                              // zeros need no launch
    if (!nbr || !x || !g || !grad_w || ldx < d1 || ldg < d2) return TSGU_ERR_BAD_ARG;
    if (nch > 1 && (!workspace || workspace_bytes < need)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        NmmGradW<V> P{};
        P.nbr = nbr;
        P.x = static_cast<const V*>(x);
        P.g = static_cast<const V*>(g);
        P.gw = static_cast<V*>(grad_w);
        P.part = static_cast<typename MfmaT<V>::Part*>(workspace);
        P.ldx = ldx;
        P.ldg = ldg;
        P.n_in = n_in;
        P.n_out = n_out;
        P.K = k;
        P.d1 = d1;
        P.d2 = d2;
        P.chunk = c;
        P.chunks = nch;
        return nmm_gradw_launch<V, decltype(i)>(P, s);
    });
}

}  // extern "C"
