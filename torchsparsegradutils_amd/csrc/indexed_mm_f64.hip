// gather_mm / segment_mm kernels for value type double (index types int32 / int64).
#include "indexed_mm_impl.h"

template int tsgu::imm_fwd_dispatch<double>(int, const tsgu::ImmFwd<double>&, int64_t, hipStream_t);
template int tsgu::imm_gradb_dispatch<double>(int, const tsgu::ImmGradB<double>&, int64_t, hipStream_t);
