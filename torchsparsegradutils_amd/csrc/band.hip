// Entry points of the banded triangular solve (include/tsgu_hip_band.h; kernels and geometry: band_impl.h).
#include "band_impl.h"

#include "../../include/tsgu_hip_band.h"

namespace tsgu {

template <typename V, typename I, int W, bool ASC, bool COLREAD>
int band_chunk_launch(BandParams P, hipStream_t s) {
    band_shape(P, W, COLREAD, (int)sizeof(V));
    const int64_t gx = (P.nch + P.CPB - 1) / P.CPB, gy = (P.ncols + P.CT - 1) / P.CT;
    if (gx > 0x7fffffffll || gy > 65535) return TSGU_ERR_BAD_ARG;
    const size_t lds = (size_t)P.CPB * P.bstride * sizeof(V);
    hipLaunchKernelGGL((band_chunk_kernel<V, I, W, ASC, COLREAD>), dim3((unsigned)gx, (unsigned)gy), dim3(kBlock), lds, s, P);
    return check_launch();
}

template <typename V, int W>
int band_carry_launch(const BandCarryParams& Q, hipStream_t s) {
    const int64_t lanes = Q.ng * (Q.apply ? Q.p : Q.p + W);
    return launch(band_carry_kernel<V, W>, (lanes + kBlock - 1) / kBlock, s, Q);
}

// reduce, carry up, the top walk, carry down, apply
template <typename V, typename I, int W, bool ASC, bool COLREAD>
int band_solve(BandParams P, const BandLevels& lv, void* work, hipStream_t s) {
    V* sum[kBandMaxLevels];
    V* st[kBandMaxLevels];
    V* w = static_cast<V*>(work);
    for (int l = 0; l < lv.L; ++l) {
        sum[l] = w;
        w += lv.m[l] * W * (P.p + W);
        st[l] = w;
        w += lv.m[l] * W * P.p;
    }
    P.apply = 0;
    P.ncols = P.p + W;
    P.sum = sum[0];
    if (const int rc = band_chunk_launch<V, I, W, ASC, COLREAD>(P, s)) return rc;
    BandCarryParams Q{};
    Q.p = P.p;
    Q.G = lv.G;
    for (int l = 0; l + 1 < lv.L; ++l) {
        Q.apply = 0;
        Q.src = sum[l];
        Q.dst = sum[l + 1];
        Q.m = lv.m[l];
        Q.ng = lv.m[l + 1];
        if (const int rc = band_carry_launch<V, W>(Q, s)) return rc;
    }
    for (int l = lv.L - 1; l >= 0; --l) {
        const bool top = l == lv.L - 1;
        Q.apply = 1;
        Q.src = sum[l];
        Q.dst = nullptr;
        Q.m = lv.m[l];
        Q.G = top ? lv.m[l] : lv.G;
        Q.ng = top ? 1 : lv.m[l + 1];
        Q.st_up = top ? nullptr : st[l + 1];
        Q.st = st[l];
        if (const int rc = band_carry_launch<V, W>(Q, s)) return rc;
    }
    P.apply = 1;
    P.ncols = P.p;
    P.sum = nullptr;
    P.st = st[0];
    return band_chunk_launch<V, I, W, ASC, COLREAD>(P, s);
}

template <typename V, typename I, int W>
int band_solve_mode(const BandParams& P, const BandLevels& lv, bool asc, bool colread, void* work, hipStream_t s) {
    if (asc) return colread ? band_solve<V, I, W, true, true>(P, lv, work, s) : band_solve<V, I, W, true, false>(P, lv, work, s);
    return colread ? band_solve<V, I, W, false, true>(P, lv, work, s) : band_solve<V, I, W, false, false>(P, lv, work, s);
}

}  // namespace tsgu

using namespace tsgu;

extern "C" {

int tsgu_csr_band_geometry(int vtype, int64_t n, int64_t p, int w, int chunk_rows, int group_chunks, int* rows, int* group, int* top) {
    if (!rows || !group || !top || p < 0) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    BandLevels lv;
    if (!band_levels(n, w, chunk_rows, group_chunks, lv)) return TSGU_ERR_BAD_ARG;
    *rows = lv.R;
    *group = lv.G;
    *top = lv.top;
    return TSGU_OK;
}

int64_t tsgu_csr_band_sptrsm_work_bytes(int vtype, int64_t n, int64_t p, int w, int chunk_rows, int group_chunks) {
    BandLevels lv;
    if (p < 0 || (vtype != TSGU_F32 && vtype != TSGU_F64) || !band_levels(n, w, chunk_rows, group_chunks, lv)) return 0;
    return band_work_values(lv, p) * (vtype == TSGU_F32 ? 4 : 8);
}

int tsgu_csr_band_sptrsm(int vtype, int itype, int64_t n, int64_t nnz, const void* ptr, const void* idx, const void* val, int w, int lower,
                         int unit, int transpose, const void* B, int64_t ldb, void* X, int64_t ldx, int64_t p, void* work,
                         int chunk_rows, int group_chunks, int device, void* stream) {
    if (n < 0 || nnz < 0 || p < 0 || p > (1 << 22) || ldb < p || ldx < p) return TSGU_ERR_BAD_ARG;
    if (vtype != TSGU_F32 && vtype != TSGU_F64) return TSGU_ERR_BAD_DTYPE;
    if (itype != TSGU_I32 && itype != TSGU_I64) return TSGU_ERR_BAD_DTYPE;
    BandLevels lv;
    if (!band_levels(n, w, chunk_rows, group_chunks, lv)) return TSGU_ERR_BAD_ARG;
    if (n == 0 || p == 0) return TSGU_OK;
    if (!ptr || !B || !X || !work || (nnz > 0 && (!idx || !val))) return TSGU_ERR_BAD_ARG;
    if (const int rc = set_device(device)) return rc;
    BandParams P{};
    P.n = n;
    P.nnz = nnz;
    P.nch = lv.m[0];
    P.ptr = ptr;
    P.idx = idx;
    P.val = val;
    P.B = B;
    P.X = X;
    P.ldb = ldb;
    P.ldx = ldx;
    P.p = (int)p;
    P.a_lower = lower ? 1 : 0;
    P.unit = unit ? 1 : 0;
    P.R = lv.R;
    const bool asc = (lower != 0) != (transpose != 0);          // op(A) is lower: the rows are walked upwards
    hipStream_t s = static_cast<hipStream_t>(stream);
    return with_types<float, double>(vtype, itype, [&](auto v, auto i) {
        using V = decltype(v);
        using I = decltype(i);
        switch (lv.Wt) {
            case 1: return band_solve_mode<V, I, 1>(P, lv, asc, transpose != 0, work, s);
            case 2: return band_solve_mode<V, I, 2>(P, lv, asc, transpose != 0, work, s);
            case 4: return band_solve_mode<V, I, 4>(P, lv, asc, transpose != 0, work, s);
            default: return band_solve_mode<V, I, 8>(P, lv, asc, transpose != 0, work, s);
        }
    });
}

}  // extern "C"
