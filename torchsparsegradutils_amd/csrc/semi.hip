// K14: entry points of the 2:4 semi-structured operand (semi_impl.h; contracts in tsgu_hip_semi.h).
#include "semi_impl.h"
#include "tsgu_hip_semi.h"

using namespace tsgu;

static_assert(TSGU_SEMI_DENSE_T == kSemiDenseT && TSGU_SEMI_OUT_T == kSemiOutT, "the header's flag bits");

namespace {

constexpr int64_t kSemiMax = 0x7fffffffLL;

inline bool aligned_to(const void* p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
inline bool is_vtype(int vtype) { return vtype == TSGU_F32 || vtype == TSGU_F64 || vtype == TSGU_BF16; }
inline size_t vbytes(int vtype) { return vtype == TSGU_F64 ? 8 : vtype == TSGU_F32 ? 4 : 2; }

// The operand's own arguments: sizes, the value rows and the position words.
inline int check_operand(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, int64_t m, int64_t k) {
    if (!val || !meta || m < 0 || k < 0 || k % 4 || ldv < k / 2 || ldm < semi_meta_words(k) || ldm % 4) return TSGU_ERR_BAD_ARG;
    if (!is_vtype(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (!aligned_to(val, vbytes(vtype)) || !aligned_to(meta, 16)) return TSGU_ERR_BAD_ARG;
    if (m >= kSemiMax || k >= kSemiMax) return TSGU_ERR_TOO_LARGE;
    return TSGU_OK;
}

// A dense (rows, cols) matrix with row stride ld, or its transpose.
inline bool dense_ok(int vtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols, bool transposed) {
    return ptr && ld >= (transposed ? rows : cols) && aligned_to(ptr, vbytes(vtype));
}

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename V>
SemiParams<V> params(const void* val, int64_t ldv, const void* meta, int64_t ldm, int64_t m, int64_t k, int64_t p, int flags) {
    SemiParams<V> P{};
    P.val = static_cast<const V*>(val);
    P.meta = static_cast<const uint32_t*>(meta);
    P.m = m;
    P.k = k;
    P.p = p;
    P.ldv = ldv;
    P.ldm = ldm;
    P.flags = flags;
    return P;
}

}  // namespace

extern "C" {

int tsgu_semi_geometry(int vtype, int64_t k, int64_t* meta_words, int* tile_rows, int* tile_cols, int* stage_columns,
                       int* sparse_instruction) {
    if (!meta_words || !tile_rows || !tile_cols || !stage_columns || !sparse_instruction || k < 0 || k % 4) return TSGU_ERR_BAD_ARG;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        *meta_words = semi_meta_words(k);
        *tile_rows = kSemiTile;
        *tile_cols = kSemiTile;
        *stage_columns = MfmaT<V>::KC;
        *sparse_instruction = std::is_same<V, bf16_t>::value ? 1 : 0;
        return TSGU_OK;
    });
}

int tsgu_semi_prune(int vtype, const void* W, int64_t ldw, int64_t m, int64_t k, void* val, int64_t ldv, void* meta, int64_t ldm,
                    int device, void* stream) {
    if (const int rc = check_operand(vtype, val, ldv, meta, ldm, m, k)) return rc;
    if (!dense_ok(vtype, W, ldw, m, k, false)) return TSGU_ERR_BAD_ARG;
    const int64_t units = 4 * semi_meta_words(k);
    if (units > 0 && m > (kSemiMax * kBlock) / units) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (m == 0 || k == 0) return TSGU_OK;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        SemiConvParams<V> P{};
        P.dense_in = static_cast<const V*>(W);
        P.val_out = static_cast<V*>(val);
        P.meta_out = static_cast<uint32_t*>(meta);
        P.m = m;
        P.k = k;
        P.ldd = ldw;
        P.ldv = ldv;
        P.ldm = ldm;
        P.units = units;
        return launch(semi_prune_kernel<V>, cdiv(m * units, kBlock), static_cast<hipStream_t>(stream), P);
    });
}

int tsgu_semi_expand(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, int64_t m, int64_t k, void* out,
                     int64_t ldo, int device, void* stream) {
    if (const int rc = check_operand(vtype, val, ldv, meta, ldm, m, k)) return rc;
    if (!dense_ok(vtype, out, ldo, m, k, false)) return TSGU_ERR_BAD_ARG;
    const int64_t units = cdiv(k, 8);
    if (units > 0 && m > (kSemiMax * kBlock) / units) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (m == 0 || k == 0) return TSGU_OK;
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        SemiConvParams<V> P{};
        P.val_in = static_cast<const V*>(val);
        P.meta_in = static_cast<const uint32_t*>(meta);
        P.dense_out = static_cast<V*>(out);
        P.m = m;
        P.k = k;
        P.ldd = ldo;
        P.ldv = ldv;
        P.ldm = ldm;
        P.units = units;
        return launch(semi_expand_kernel<V>, cdiv(m * units, kBlock), static_cast<hipStream_t>(stream), P);
    });
}

int tsgu_semi_mm(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, const void* Y, int64_t ldy, const void* bias,
                 void* C, int64_t ldc, int64_t m, int64_t k, int64_t p, int flags, int path, int device, void* stream) {
    if (const int rc = check_operand(vtype, val, ldv, meta, ldm, m, k)) return rc;
    if (p < 0 || (flags & ~(kSemiDenseT | kSemiOutT)) || (path != 0 && path != 1) || (path == 1 && vtype != TSGU_BF16)) return TSGU_ERR_BAD_ARG;
    if (!dense_ok(vtype, Y, ldy, p, k, flags & kSemiDenseT) || !dense_ok(vtype, C, ldc, m, p, flags & kSemiOutT)) return TSGU_ERR_BAD_ARG;
    if (!aligned_to(bias, vbytes(vtype))) return TSGU_ERR_BAD_ARG;
    if (p >= kSemiMax) return TSGU_ERR_TOO_LARGE;
    const int64_t tiles_m = cdiv(m, kSemiTile), tiles_n = cdiv(p, kSemiTile);
    if (tiles_n > 0 && tiles_m > kSemiMax / tiles_n) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (m == 0 || p == 0) return TSGU_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        SemiParams<V> P = params<V>(val, ldv, meta, ldm, m, k, p, flags);
        P.Y = static_cast<const V*>(Y);
        P.ldy = ldy;
        P.bias = static_cast<const V*>(bias);
        P.out = static_cast<V*>(C);
        P.ldo = ldc;
        P.tiles_x = tiles_n;
        if constexpr (std::is_same<V, bf16_t>::value)
            if (path == 1) return launch(semi_mm_kernel<V, true>, tiles_m * tiles_n, s, P);
        return launch(semi_mm_kernel<V, false>, tiles_m * tiles_n, s, P);
    });
}

int tsgu_semi_mm_t(int vtype, const void* val, int64_t ldv, const void* meta, int64_t ldm, const void* G, int64_t ldg, void* D,
                   int64_t ldd, int64_t m, int64_t k, int64_t p, int flags, int device, void* stream) {
    if (const int rc = check_operand(vtype, val, ldv, meta, ldm, m, k)) return rc;
    if (p < 0 || (flags & ~(kSemiDenseT | kSemiOutT))) return TSGU_ERR_BAD_ARG;
    if (!dense_ok(vtype, G, ldg, m, p, flags & kSemiDenseT) || !dense_ok(vtype, D, ldd, k, p, flags & kSemiOutT)) return TSGU_ERR_BAD_ARG;
    if (p >= kSemiMax) return TSGU_ERR_TOO_LARGE;
    const int64_t tiles_c = cdiv(k, kSemiStage), tiles_n = cdiv(p, kSemiTile);
    if (tiles_n > 0 && tiles_c > kSemiMax / tiles_n) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (k == 0 || p == 0) return TSGU_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        SemiParams<V> P = params<V>(val, ldv, meta, ldm, m, k, p, flags);
        P.Y = static_cast<const V*>(G);
        P.ldy = ldg;
        P.out = static_cast<V*>(D);
        P.ldo = ldd;
        P.tiles_x = tiles_n;
        return launch(semi_mm_t_kernel<V>, tiles_c * tiles_n, s, P);
    });
}

int tsgu_semi_sddmm(int vtype, const void* G, int64_t ldg, const void* Y, int64_t ldy, const void* meta, int64_t ldm, void* out,
                    int64_t ldo, int64_t m, int64_t k, int64_t p, int flags, int device, void* stream) {
    if (const int rc = check_operand(vtype, out, ldo, meta, ldm, m, k)) return rc;
    if (p < 0 || (flags & ~kSemiDenseT)) return TSGU_ERR_BAD_ARG;
    if (!dense_ok(vtype, G, ldg, m, p, flags & kSemiDenseT) || !dense_ok(vtype, Y, ldy, k, p, flags & kSemiDenseT)) return TSGU_ERR_BAD_ARG;
    if (p >= kSemiMax) return TSGU_ERR_TOO_LARGE;
    const int64_t tiles_m = cdiv(m, kSemiTile), tiles_c = cdiv(k, kSemiTile);
    if (tiles_c > 0 && tiles_m > kSemiMax / tiles_c) return TSGU_ERR_TOO_LARGE;
    if (const int rc = set_device(device)) return rc;
    if (m == 0 || k == 0) return TSGU_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto tag) -> int {
        using V = decltype(tag);
        SemiParams<V> P = params<V>(nullptr, 0, meta, ldm, m, k, p, flags);
        P.G = static_cast<const V*>(G);
        P.ldg = ldg;
        P.Y = static_cast<const V*>(Y);
        P.ldy = ldy;
        P.out = static_cast<V*>(out);
        P.ldo = ldo;
        P.tiles_x = tiles_c;
        return launch(semi_sddmm_kernel<V>, tiles_m * tiles_c, s, P);
    });
}

}  // extern "C"
