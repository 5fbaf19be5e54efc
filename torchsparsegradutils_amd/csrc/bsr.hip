// Block-sparse × dense products: the extern "C" entry points of include/tsgu_hip_bsr.h (kernels: bsr_impl.h, one instantiation
// file per value type).
#include "bsr_impl.h"
#include "bsr_host.h"

#include "../../include/tsgu_hip_bsr.h"

using namespace tsgu;

namespace {

// Whole aligned 16-byte lanes: a base on a 16-byte boundary and every listed count a multiple of the lane's elements.
bool whole_lanes(int vtype, std::initializer_list<const void*> bases, std::initializer_list<int64_t> counts) {
    const int w = vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 2 : 8;
    for (const void* q : bases)
        if (!aligned16(q)) return false;
    for (const int64_t c : counts)
        if (c % w) return false;
    return true;
}

// The host-side refusals the three launchers share, in the order the header states.
int bsr_check(int vtype, int itype, int64_t nrb, int64_t ncb, int64_t nnzb, int64_t bh, int64_t bw, int64_t p,
              std::initializer_list<const void*> always, std::initializer_list<const void*> stored, std::initializer_list<Dense> dense) {
    if (const int rc = bsr_check_args(vtype, itype, nnzb, always, stored)) return rc;
    if (p < 1 || bh < 1 || bw < 1 || nrb < 0 || ncb < 0 || nnzb < 0) return TSGU_ERR_BAD_ARG;
    for (const Dense& o : dense) {
        if (o.ld < p) return TSGU_ERR_BAD_ARG;
        if (reinterpret_cast<uintptr_t>(o.ptr) % elem_bytes(vtype)) return TSGU_ERR_BAD_ARG;      // whole elements
    }
    return bsr_check_sizes(nrb, ncb, nnzb, bh, bw, dense, false);
}

// Forward (trans = false: walks block rows, sums over bw) and transposed product (walks block columns, sums over bh).
int bsr_mm(int vtype, int itype, bool trans, int64_t n_groups, int64_t bh, int64_t bw, const void* ptr, const void* idx,
           const void* perm, const void* val, const void* D, int64_t ldd, int64_t p, void* out, int64_t ldo, int device, void* stream) {
    if (n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t oh = trans ? bw : bh;
    const BsrSplit split = bsr_tile_split(oh, kBsrTM, n_groups);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto v) {
        using V = decltype(v);
        BsrMM<V> P{};
        P.ptr = ptr, P.idx = idx, P.perm = perm;
        P.val = static_cast<const V*>(val), P.D = static_cast<const V*>(D), P.out = static_cast<V*>(out);
        P.ldd = ldd, P.ldo = ldo, P.n_groups = n_groups, P.p = p, P.bh = bh, P.bw = bw;
        P.oh = oh, P.kb = trans ? bh : bw;
        P.per_tile = split.per_tile, P.pieces = split.pieces;
        P.lanes = whole_lanes(vtype, {val, D}, {bw, ldd, p});
        return bsr_mm_dispatch<V>(itype, trans, P, s);
    });
}

}  // namespace

extern "C" {

int tsgu_bsr_mm_geometry(int vtype, int64_t bh, int64_t bw, int64_t p, int* tile_rows, int* tile_cols, int* k_stage) {
    if (!tile_rows || !tile_cols || !k_stage) return TSGU_ERR_BAD_ARG;
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (p < 1 || bh < 1 || bw < 1) return TSGU_ERR_BAD_ARG;
    *tile_rows = kBsrTM;
    *tile_cols = vtype == TSGU_F64 ? bsr_tile_cols<double>(p) : bsr_tile_cols<float>(p);
    *k_stage = vtype == TSGU_F32 ? MfmaT<float>::KC : vtype == TSGU_F64 ? MfmaT<double>::KC : MfmaT<bf16_t>::KC;
    return TSGU_OK;
}

int tsgu_bsr_spmm(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                  const void* ptr, const void* idx, const void* val, const void* B, int64_t ldb, int64_t p, void* C, int64_t ldc,
                  int device, void* stream) {
    if (const int rc = bsr_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, p, {ptr, C}, {idx, val, B}, {{B, ldb}, {C, ldc}}))
        return rc;
    return bsr_mm(vtype, itype, false, n_block_rows, bh, bw, ptr, idx, nullptr, val, B, ldb, p, C, ldc, device, stream);
}

int tsgu_bsr_sddmm(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                   const void* ptr, const void* idx, const void* G, int64_t ldg, const void* B, int64_t ldb, int64_t p, void* dval,
                   int device, void* stream) {
    if (const int rc = bsr_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, p, {ptr}, {idx, G, B, dval}, {{G, ldg}, {B, ldb}}))
        return rc;
    if (nnzb == 0 || n_block_rows == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_value_type<float, double, bf16_t>(vtype, [&](auto v) {
        using V = decltype(v);
        BsrSddmm<V> P{};
        P.ptr = ptr, P.idx = idx;
        P.G = static_cast<const V*>(G), P.B = static_cast<const V*>(B), P.dval = static_cast<V*>(dval);
        P.ldg = ldg, P.ldb = ldb, P.n_block_rows = n_block_rows, P.p = p, P.bh = bh, P.bw = bw;
        P.pieces_n = (bw + kBsrTM - 1) / kBsrTM;
        P.lanes = whole_lanes(vtype, {G, B}, {ldg, ldb, p});
        return bsr_sddmm_dispatch<V>(itype, P, nnzb, s);
    });
}

int tsgu_bsr_spmm_t(int vtype, int itype, int64_t n_block_rows, int64_t n_block_cols, int64_t nnzb, int64_t bh, int64_t bw,
                    const void* tptr, const void* tidx, const void* perm, const void* val, const void* G, int64_t ldg, int64_t p,
                    void* dB, int64_t lddb, int device, void* stream) {
    if (const int rc = bsr_check(vtype, itype, n_block_rows, n_block_cols, nnzb, bh, bw, p, {tptr, dB}, {tidx, perm, val, G},
                                 {{G, ldg}, {dB, lddb}}))
        return rc;
    return bsr_mm(vtype, itype, true, n_block_cols, bh, bw, tptr, tidx, perm, val, G, ldg, p, dB, lddb, device, stream);
}

}  // extern "C"
