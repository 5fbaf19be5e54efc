// gather_mm / segment_mm kernels for value type float (index types int32 / int64).
#include "indexed_mm_impl.h"

template int tsgu::imm_fwd_dispatch<float>(int, const tsgu::ImmFwd<float>&, int64_t, hipStream_t);
template int tsgu::imm_gradb_dispatch<float>(int, const tsgu::ImmGradB<float>&, int64_t, hipStream_t);
