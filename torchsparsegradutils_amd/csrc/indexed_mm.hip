// gather_mm / segment_mm: the extern "C" entry points (kernels: indexed_mm_impl.h, one instantiation file per value type).
#include "indexed_mm_impl.h"

using namespace tsgu;

namespace {

constexpr int kGradBWorkgroups = 2048;     // split-K target: about eight workgroups per compute unit

int64_t part_size(int vtype) { return vtype == TSGU_F64 ? 8 : 4; }

int64_t gradb_chunk(int64_t n, int64_t d1, int64_t d2) {
    const int64_t tiles = ((d1 + kImmGT - 1) / kImmGT) * ((d2 + kImmGT - 1) / kImmGT);
    const int64_t want = (n * (tiles > 0 ? tiles : 1) + kGradBWorkgroups - 1) / kGradBWorkgroups;
    int64_t c = 256;
    while (c < want && c < (int64_t)1 << 16) c <<= 1;
    return c;
}

template <typename V>
ImmFwd<V> fwd_params(const void* offsets, const void* tile_ptr, const void* perm, const void* a, int64_t lda, const void* b,
                     int64_t bs0, int64_t bs1, int64_t bs2, void* out, int64_t ldo, int64_t n_seg, int64_t d1, int64_t d2) {
    ImmFwd<V> P{};
    P.offsets = offsets;
    P.tile_ptr = tile_ptr;
    P.perm = perm;
    P.a = static_cast<const V*>(a);
    P.b = static_cast<const V*>(b);
    P.out = static_cast<V*>(out);
    P.lda = lda;
    P.ldo = ldo;
    P.bs0 = bs0;
    P.bs1 = bs1;
    P.bs2 = bs2;
    P.n_seg = n_seg;
    P.d1 = d1;
    P.d2 = d2;
    return P;
}

template <typename V>
ImmGradB<V> gradb_params(const void* offsets, const void* chunk_ptr, const void* part_ptr, const void* perm, const void* a,
                         int64_t lda, const void* g, int64_t ldg, void* grad_b, void* ws, int64_t n_seg, int64_t d1, int64_t d2,
                         int64_t chunk) {
    ImmGradB<V> P{};
    P.offsets = offsets;
    P.chunk_ptr = chunk_ptr;
    P.part_ptr = part_ptr;
    P.perm = perm;
    P.a = static_cast<const V*>(a);
    P.g = static_cast<const V*>(g);
    P.gb = static_cast<V*>(grad_b);
    P.part = static_cast<typename MfmaT<V>::Part*>(ws);
    P.lda = lda;
    P.ldg = ldg;
    P.n_seg = n_seg;
    P.d1 = d1;
    P.d2 = d2;
    P.chunk = chunk;
    return P;
}

}  // namespace

extern "C" {

int tsgu_segment_mm_tile_rows(void) { return kImmBM; }

int tsgu_segment_mm(int vtype, int itype, int64_t n, int64_t d1, int64_t d2, int64_t n_seg, const void* offsets,
                    const void* tile_ptr, int64_t max_tiles, const void* perm, const void* a, int64_t lda, const void* b,
                    int64_t b_stride0, int64_t b_stride1, int64_t b_stride2, void* out, int64_t ldo, int device, void* stream) {
    if (n < 0 || d1 < 0 || d2 < 0 || n_seg < 0 || max_tiles < 0) return TSGU_ERR_BAD_ARG;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n == 0 || d2 == 0) return TSGU_OK;
    if (!offsets || !tile_ptr || !out || ldo < d2 || (d1 > 0 && (!a || lda < d1 || (n_seg > 0 && !b)))) return TSGU_ERR_BAD_ARG;
    if (d1 > 0 && n_seg > 0 && b_stride1 != 1 && b_stride2 != 1) return TSGU_ERR_BAD_ARG;   // one of b[r]'s axes is contiguous
    if (max_tiles < (n + kImmBM - 1) / kImmBM + (n_seg < n ? n_seg : n) + 2) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto v) {
        using V = decltype(v);
        return imm_fwd_dispatch<V>(itype, fwd_params<V>(offsets, tile_ptr, perm, a, lda, b, b_stride0, b_stride1, b_stride2, out, ldo, n_seg, d1, d2),
                                   max_tiles, s);
    });
}

int tsgu_segment_mm_grad_b_workspace(int vtype, int64_t n, int64_t n_seg, int64_t d1, int64_t d2, int64_t* chunk_rows,
                                     int64_t* max_chunks, int64_t* bytes) {
    if (n < 0 || n_seg < 0 || d1 < 0 || d2 < 0 || !chunk_rows || !max_chunks || !bytes) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64 && vtype != TSGU_BF16) return TSGU_ERR_BAD_DTYPE;
    const int64_t c = gradb_chunk(n, d1, d2);
    const int64_t full = (n + c - 1) / c;
    *chunk_rows = c;
    *max_chunks = full + (n_seg < n ? n_seg : n);
    // a segment of two or more chunks is longer than one chunk, so those segments hold at most 2 * ceil(n / c) chunks in all
    const int64_t b = 2 * full * d1 * d2 * part_size(vtype);
    *bytes = b > 16 ? b : 16;
    return TSGU_OK;
}

int tsgu_segment_mm_grad_b(int vtype, int itype, int64_t n, int64_t d1, int64_t d2, int64_t n_seg, const void* offsets,
                           const void* chunk_ptr, const void* part_ptr, int64_t chunk_rows, int64_t max_chunks, const void* perm,
                           const void* a, int64_t lda, const void* g, int64_t ldg, void* grad_b, void* workspace,
                           int64_t workspace_bytes, int device, void* stream) {
    if (n < 0 || d1 < 0 || d2 < 0 || n_seg < 0 || max_chunks < 0) return TSGU_ERR_BAD_ARG;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    if (n_seg == 0 || d1 == 0 || d2 == 0) return TSGU_OK;
    int64_t c = 0, mc = 0, need = 0;
    if (const int rc = tsgu_segment_mm_grad_b_workspace(vtype, n, n_seg, d1, d2, &c, &mc, &need)) return rc;
    if (chunk_rows != c || max_chunks < mc || workspace_bytes < need) return TSGU_ERR_BAD_ARG;
    if (!offsets || !chunk_ptr || !part_ptr || !grad_b || !workspace) return TSGU_ERR_BAD_ARG;
    if (n > 0 && (!a || !g || lda < d1 || ldg < d2)) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t launched = n > 0 ? max_chunks : 0;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto v) {
        using V = decltype(v);
        return imm_gradb_dispatch<V>(itype, gradb_params<V>(offsets, chunk_ptr, part_ptr, perm, a, lda, g, ldg, grad_b, workspace, n_seg, d1, d2, c),
                                     launched, s);
    });
}

}  // extern "C"
