// Max / min products over a sparse pattern: instantiations (fp32, fp64, bf16 × int32, int64 × forward, values pass, dense pass) and
// the extern "C" entry points of include/tsgu_hip_mm_reduce.h.
#include "mm_reduce_impl.h"

#include "../../include/tsgu_hip_mm_reduce.h"

using namespace tsgu;

namespace {

constexpr int64_t kI31 = 0x7fffffffLL;

struct Dense {
    const void* ptr;
    int64_t ld;
    bool needed = true;     // false: the gathered side of a pattern without entries, never dereferenced
};

int elem_bytes(int vtype) { return vtype == TSGU_F32 ? 4 : vtype == TSGU_F64 ? 8 : vtype == TSGU_BF16 ? 2 : 0; }
int wide_of(int vtype) { return 16 / elem_bytes(vtype); }

RowGeom geom_of(int vtype, int64_t p, bool can_wide) {
    if (vtype == TSGU_F64) return mm_reduce_geom<double>(p, can_wide);
    if (vtype == TSGU_BF16) return mm_reduce_geom<bf16_t>(p, can_wide);
    return mm_reduce_geom<float>(p, can_wide);
}

// The host-side refusals the three launchers share; `n_groups`: the walked side.  `wide` comes back true when every dense operand
// (arg included) can be touched in aligned 16-byte lanes.
int reduce_check(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_groups, int64_t p,
                 std::initializer_list<const void*> index_arrays, std::initializer_list<const void*> others,
                 std::initializer_list<Dense> dense, const void* arg, int64_t ldarg, bool* wide) {
    if (!elem_bytes(vtype) || (itype != TSGU_I32 && itype != TSGU_I64)) return TSGU_ERR_BAD_DTYPE;
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
    const int w = wide_of(vtype);
    bool can = true;
    for (const Dense& o : dense) {
        if (!o.needed) continue;
        if (!o.ptr || o.ld < p) return TSGU_ERR_BAD_ARG;
        if (reinterpret_cast<uintptr_t>(o.ptr) % elem_bytes(vtype)) return TSGU_ERR_BAD_ARG;      // whole elements
        if (o.ld > 0xffffffffLL) return TSGU_ERR_TOO_LARGE;
        can = can && lanes_of(o.ptr, o.ld, w);
    }
    if (!arg || ldarg < p) return TSGU_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(arg) & 3u) return TSGU_ERR_BAD_ARG;      // int32 entries
    if (ldarg > 0xffffffffLL) return TSGU_ERR_TOO_LARGE;
    *wide = can && lanes_of(arg, ldarg, w);
    return TSGU_OK;
}

template <int KIND>
int reduce_launch(int vtype, int itype, const MmReduceParams& P, bool wide, int device, void* stream) {
    if (P.n_groups == 0) return TSGU_OK;
    if (const int rc = set_device(device)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double, bf16_t>(vtype, itype, [&](auto v, auto i) {
        return mm_reduce_launch<decltype(v), decltype(i), KIND>(P, wide, s);
    });
}

}  // namespace

extern "C" {

int tsgu_csr_spmm_reduce_geometry(int vtype, int64_t p, int* rows_per_block, int* stage_entries, int* cols_per_slice) {
    if (!elem_bytes(vtype)) return TSGU_ERR_BAD_DTYPE;
    if (p < 1 || !rows_per_block || !stage_entries || !cols_per_slice) return TSGU_ERR_BAD_ARG;
    const RowGeom g = geom_of(vtype, p, true);
    *rows_per_block = (int)spmm_rows_per_block(g);
    *stage_entries = kStageCap;
    *cols_per_slice = g.cl * g.vec;
    return TSGU_OK;
}

int tsgu_csr_spmm_reduce(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr, const void* idx,
                         const void* val, const void* B, int64_t ldb, int64_t p, int op, void* C, int64_t ldc, int* arg,
                         int64_t ldarg, int device, void* stream) {
    bool wide = false;
    if (const int rc = reduce_check(vtype, itype, n_rows, n_cols, nnz, n_rows, p, {ptr, idx, val}, {}, {{B, ldb, nnz > 0}, {C, ldc}},
                                    arg, ldarg, &wide))
        return rc;
    if (op != 0 && op != 1) return TSGU_ERR_BAD_ARG;
    MmReduceParams P{};
    P.n_groups = n_rows, P.p = p, P.ptr = ptr, P.idx = idx, P.val = val;
    P.B = B, P.ldb = ldb, P.C = C, P.ldc = ldc, P.arg = arg, P.ldarg = ldarg, P.op = op;
    return reduce_launch<kMmReduceFwd>(vtype, itype, P, wide, device, stream);
}

int tsgu_csr_spmm_reduce_backward_values(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* ptr,
                                         const void* idx, const int* arg, int64_t ldarg, const void* G, int64_t ldg, const void* B,
                                         int64_t ldb, int64_t p, void* dval, int device, void* stream) {
    bool wide = false;
    if (const int rc = reduce_check(vtype, itype, n_rows, n_cols, nnz, n_rows, p, {ptr, idx}, {dval}, {{G, ldg}, {B, ldb, nnz > 0}}, arg,
                                    ldarg, &wide))
        return rc;
    if (nnz == 0) return TSGU_OK;
    MmReduceParams P{};
    P.n_groups = n_rows, P.p = p, P.ptr = ptr, P.idx = idx;
    P.B = B, P.ldb = ldb, P.G = G, P.ldg = ldg, P.C = dval, P.arg = const_cast<int*>(arg), P.ldarg = ldarg;
    return reduce_launch<kMmReduceBwdValues>(vtype, itype, P, wide, device, stream);
}

int tsgu_csr_spmm_reduce_backward_dense(int vtype, int itype, int64_t n_rows, int64_t n_cols, int64_t nnz, const void* tptr,
                                        const void* tidx, const void* perm, const void* val, const int* arg, int64_t ldarg,
                                        const void* G, int64_t ldg, int64_t p, void* dB, int64_t lddb, int device, void* stream) {
    bool wide = false;
    const bool far = nnz > 0;
    if (const int rc = reduce_check(vtype, itype, n_rows, n_cols, nnz, n_cols, p, {tptr, tidx, perm, val}, {}, {{G, ldg, far}, {dB, lddb}},
                                    far ? arg : static_cast<const void*>(tptr), far ? ldarg : p, &wide))
        return rc;
    MmReduceParams P{};
    P.n_groups = n_cols, P.p = p, P.ptr = tptr, P.idx = tidx, P.perm = perm, P.val = val;
    P.G = G, P.ldg = ldg, P.C = dB, P.ldc = lddb, P.arg = const_cast<int*>(arg), P.ldarg = ldarg;
    return reduce_launch<kMmReduceBwdDense>(vtype, itype, P, wide, device, stream);
}

}  // extern "C"
