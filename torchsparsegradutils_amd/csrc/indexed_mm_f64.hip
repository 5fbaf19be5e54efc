// gather_mm / segment_mm kernels for value type double (index types int32 / int64).
#include "indexed_mm_impl.h"

namespace tsgu {
int imm_fwd_dispatch_f64(int itype, const ImmFwd<double>& P, int64_t max_tiles, hipStream_t s) {
    if (itype == TSGU_I32) return imm_fwd_launch<double, int32_t>(P, max_tiles, s);
    if (itype == TSGU_I64) return imm_fwd_launch<double, int64_t>(P, max_tiles, s);
    return TSGU_ERR_BAD_DTYPE;
}
int imm_gradb_dispatch_f64(int itype, const ImmGradB<double>& P, int64_t max_chunks, hipStream_t s) {
    if (itype == TSGU_I32) return imm_gradb_launch<double, int32_t>(P, max_chunks, s);
    if (itype == TSGU_I64) return imm_gradb_launch<double, int64_t>(P, max_chunks, s);
    return TSGU_ERR_BAD_DTYPE;
}
}  // namespace tsgu
