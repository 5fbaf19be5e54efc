// Products in the log and tropical semirings over a sparse pattern: instantiations (fp32, fp64, bf16 × int32, int64 × three
// semirings × forward, values pass, dense pass) and the extern "C" entry points of tsgu_hip_semiring.h.
#include "semiring_impl.h"

#include "../../include/tsgu_hip_semiring.h"

using namespace tsgu;

namespace {

constexpr int64_t kI31 = 0x7fffffffLL;

// A dense operand of p columns: `bytes` per element (the value type's, 4 for arg, the accumulator's for C_acc).
struct Dense {
    const void* ptr;
    int64_t ld;
    int bytes;
    bool needed = true;     // false: an operand this semiring (or a pattern without entries) never dereferences
};

int elem_bytes(int vtype) { return vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 8 : vtype == TSGU_BF16 ? 2 : 0; }
int acc_bytes(int vtype) { return vtype == TSGU_F64 ? 8 : 4; }

RowGeom geom_of(int vtype, int64_t p, bool can_wide) {
    if (vtype == TSGU_F64) return mm_reduce_geom<double>(p, can_wide);
    if (vtype == TSGU_BF16) return mm_reduce_geom<bf16_t>(p, can_wide);
    return mm_reduce_geom<float>(p, can_wide);
}

// The host-side refusals the three launchers share; `n_groups`: the walked side.  `wide` comes back true when every dense operand
// that is read or written can be touched in aligned lanes of 16 / sizeof(value) elements.
int semiring_check(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_groups, int64_t p,
                   std::initializer_list<const void*> index_arrays, std::initializer_list<const void*> others,
                   std::initializer_list<Dense> dense, bool* wide) {
    if (!elem_bytes(vtype) || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
    if (semiring != kSemiringLog && semiring != kSemiringMax && semiring != kSemiringMin) return TSGU_ERR_BAD_ARG;
    if (n_rows < 0 || n_cols < 0 || nnz < 0 || p < 1) return TSGU_ERR_BAD_ARG;
    if (nnz > kI31) return TSGU_ERR_TOO_LARGE;                  // arg holds stored positions as int32
    if (n_rows > kI31 || n_cols > kI31) return TSGU_ERR_TOO_LARGE;
    if (n_groups == 0) return TSGU_OK;
    bool first = true;
    for (const void* q : index_arrays) {                        // ptr, then the arrays of nnz entries
        if (!q && (first || nnz > 0)) return TSGU_ERR_BAD_ARG;
        first = false;
    }
    for (const void* q : others)
        if (!q && nnz > 0) return TSGU_ERR_BAD_ARG;
    const int w = 16 / elem_bytes(vtype);
    bool can = true;
    for (const Dense& o : dense) {
        if (!o.needed) continue;
        if (!o.ptr || o.ld < p) return TSGU_ERR_BAD_ARG;
        if (reinterpret_cast<uintptr_t>(o.ptr) % o.bytes) return TSGU_ERR_BAD_ARG;      // whole elements
        if (o.ld > 0xffffffffLL) return TSGU_ERR_TOO_LARGE;
        can = can && lanes_of(o.ptr, o.ld, w);
    }
    *wide = can;
    return TSGU_OK;
}

template <int KIND>
int launch_kind(int vtype, int itype, int semiring, const SemiringParams& P, bool wide, int device, void* stream) {
    if (P.n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        return semiring_launch<decltype(v), decltype(i), KIND>(P, semiring, wide, s);
    });
}

}  // namespace

extern "C" {

int tsgu_semiring_geometry(int vtype, int64_t p, int* rows_per_block, int* stage_entries, int* cols_per_slice) {
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (p < 1 || !rows_per_block || !stage_entries || !cols_per_slice) return TSGU_ERR_BAD_ARG;
    const RowGeom g = geom_of(vtype, p, true);
    *rows_per_block = (int)spmm_rows_per_block(g);
    *stage_entries = kStageCap;
    *cols_per_slice = g.cl * g.vec;
    return TSGU_OK;
}

int tsgu_csr_semiring_mm(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                         const void* idx, const void* val, const void* B, int64_t ldb, int64_t p, void* C, int64_t ldc, void* C_acc,
                         int64_t ldacc, int* arg, int64_t ldarg, int device, void* stream) {
    bool wide = false;
    const bool log = semiring == kSemiringLog;
    if (const int rc = semiring_check(vtype, itype, semiring, n_rows, n_cols, nnz, n_rows, p, {ptr, idx, val}, {},
                                      {{B, ldb, elem_bytes(vtype), nnz > 0},
                                       {C, ldc, elem_bytes(vtype)},
                                       {C_acc, ldacc, acc_bytes(vtype), log && C_acc != nullptr},
                                       {arg, ldarg, 4, !log}},
                                      &wide))
        return rc;
    SemiringParams P{};
    P.n_groups = n_rows, P.p = p, P.ptr = ptr, P.idx = idx, P.val = val;
    P.B = B, P.ldb = ldb, P.out = C, P.ldout = ldc, P.cacc = log ? C_acc : nullptr, P.ldacc = ldacc, P.arg = arg, P.ldarg = ldarg;
    return launch_kind<kSemiringFwd>(vtype, itype, semiring, P, wide, device, stream);
}

int tsgu_csr_semiring_mm_bwd_values(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                    const void* idx, const void* val, const void* B, int64_t ldb, const void* C_acc, int64_t ldacc,
                                    const int* arg, int64_t ldarg, const void* G, int64_t ldg, int64_t p, void* dval, int device,
                                    void* stream) {
    bool wide = false;
    const bool log = semiring == kSemiringLog;
    if (const int rc = semiring_check(vtype, itype, semiring, n_rows, n_cols, nnz, n_rows, p, {ptr, idx}, {dval, log ? val : dval},
                                      {{G, ldg, elem_bytes(vtype), nnz > 0},
                                       {B, ldb, elem_bytes(vtype), log && nnz > 0},
                                       {C_acc, ldacc, acc_bytes(vtype), log && nnz > 0},
                                       {arg, ldarg, 4, !log && nnz > 0}},
                                      &wide))
        return rc;
    if (nnz == 0) return TSGU_OK;
    SemiringParams P{};
    P.n_groups = n_rows, P.p = p, P.ptr = ptr, P.idx = idx, P.val = val, P.B = B, P.ldb = ldb, P.G = G, P.ldg = ldg;
    P.out = dval, P.cacc = const_cast<void*>(C_acc), P.ldacc = ldacc, P.arg = const_cast<int*>(arg), P.ldarg = ldarg;
    return launch_kind<kSemiringBwdValues>(vtype, itype, semiring, P, wide, device, stream);
}

int tsgu_csr_semiring_mm_bwd_dense(int vtype, int itype, int semiring, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                   const void* tidx, const void* perm, const void* val, const void* B, int64_t ldb, const void* C_acc,
                                   int64_t ldacc, const int* arg, int64_t ldarg, const void* G, int64_t ldg, int64_t p, void* dB,
                                   int64_t lddb, int device, void* stream) {
    bool wide = false;
    const bool log = semiring == kSemiringLog, far = nnz > 0;
    if (const int rc = semiring_check(vtype, itype, semiring, n_rows, n_cols, nnz, n_cols, p, {tptr, tidx, perm}, {log ? val : tidx},
                                      {{G, ldg, elem_bytes(vtype), far},
                                       {dB, lddb, elem_bytes(vtype)},
                                       {B, ldb, elem_bytes(vtype), log},
                                       {C_acc, ldacc, acc_bytes(vtype), log && far},
                                       {arg, ldarg, 4, !log && far}},
                                      &wide))
        return rc;
    SemiringParams P{};
    P.n_groups = n_cols, P.p = p, P.ptr = tptr, P.idx = tidx, P.perm = perm, P.val = val, P.B = B, P.ldb = ldb, P.G = G, P.ldg = ldg;
    P.out = dB, P.ldout = lddb, P.cacc = const_cast<void*>(C_acc), P.ldacc = ldacc, P.arg = const_cast<int*>(arg), P.ldarg = ldarg;
    return launch_kind<kSemiringBwdDense>(vtype, itype, semiring, P, wide, device, stream);
}

}  // extern "C"
