// K13: entry points of sparse_topk_mm (topk_impl.h; contracts in tsgu_hip_topk.h).
#include <cmath>

#include "topk_impl.h"
#include "tsgu_hip_topk.h"

using namespace tsgu;

static_assert(TSGU_TOPK_CAUSAL == kTopkCausal && TSGU_TOPK_EXCLUDE_SELF == kTopkExcludeSelf, "the header's flag bits");

namespace {

inline bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

}  // namespace

extern "C" {

int tsgu_topk_geometry(int vtype, int64_t d, int k, int* k_cap, int* rows_per_workgroup, int* keys_per_tile, int* stage_columns,
                       int* lds_bytes) {
    if (!k_cap || !rows_per_workgroup || !keys_per_tile || !stage_columns || !lds_bytes || d < 1 || k < 1) return TSGU_ERR_BAD_ARG;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using L = TopkLds<decltype(tag)>;
        *k_cap = kTopkCap;
        *rows_per_workgroup = L::R;
        *keys_per_tile = L::T;
        *stage_columns = L::KC;
        *lds_bytes = 0;
        if (k > kTopkCap) return TSGU_ERR_TOO_LARGE;
        *lds_bytes = L::bytes(k);
        return TSGU_OK;
    });
}

int tsgu_topk_mm(int vtype, const void* Q, const void* K, const void* key_bias, int64_t n, int64_t m, int64_t d, int k, double scale,
                 int flags, int64_t causal_offset, const void* crow, void* col, void* val, int itype, int64_t batch, int64_t q_stride,
                 int64_t k_stride, int64_t bias_stride, int64_t out_stride, int device, void* stream) {
    if (!Q || !K || !crow || !col || !val || n < 0 || m < 0 || d < 1 || k < 1 || batch < 0) return TSGU_ERR_BAD_ARG;
    if (q_stride < 0 || k_stride < 0 || bias_stride < 0 || out_stride < 0) return TSGU_ERR_BAD_ARG;
    if ((flags & ~(kTopkCausal | kTopkExcludeSelf)) || !std::isfinite(scale)) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64 && vtype != TSGU_BF16) return TSGU_ERR_BAD_DTYPE;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    const size_t ve = vtype == TSGU_F64 ? 8 : vtype == TSGU_F32 ? 4 : 2, ie = itype == TSGU_I64 ? 8 : 4;
    if (!(aligned_to(Q, ve) && aligned_to(K, ve) && aligned_to(key_bias, ve) && aligned_to(val, ve) && aligned_to(crow, ie) && aligned_to(col, ie)))
        return TSGU_ERR_BAD_ARG;
    if (k > kTopkCap || n >= 0x7fffffffLL || m >= 0x7fffffffLL) return TSGU_ERR_TOO_LARGE;
    static_assert(TopkLds<bf16_t>::R == TopkLds<float>::R, "one tile height for the fp32 accumulators");
    const int64_t rows = vtype == TSGU_F64 ? TopkLds<double>::R : TopkLds<float>::R, tiles = (n + rows - 1) / rows;
    if (batch > 0 && tiles > 0x7fffffffLL / batch) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (n == 0 || m == 0 || batch == 0) return TSGU_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto vtag, auto itag) -> int {
        using V = decltype(vtag);
        using I = decltype(itag);
        TopkParams<V> P;
        P.Q = static_cast<const V*>(Q);
        P.K = static_cast<const V*>(K);
        P.bias = static_cast<const V*>(key_bias);
        P.crow = crow;
        P.col = col;
        P.val = static_cast<V*>(val);
        P.n = n;
        P.m = m;
        P.d = d;
        P.off = causal_offset;
        P.q_stride = q_stride;
        P.k_stride = k_stride;
        P.bias_stride = bias_stride;
        P.out_stride = out_stride;
        P.tiles = tiles;
        P.k = k;
        P.flags = flags;
        P.scale = (typename TopkParams<V>::Acc)scale;
        return topk_launch<V, I>(P, P.tiles * batch, s);
    });
}

}  // extern "C"
