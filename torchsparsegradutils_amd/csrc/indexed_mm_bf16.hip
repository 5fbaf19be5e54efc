// gather_mm / segment_mm kernels for value type bf16_t (index types int32 / int64).
#include "indexed_mm_impl.h"

template int tsgu::imm_fwd_dispatch<tsgu::bf16_t>(int, const tsgu::ImmFwd<tsgu::bf16_t>&, int64_t, hipStream_t);
template int tsgu::imm_gradb_dispatch<tsgu::bf16_t>(int, const tsgu::ImmGradB<tsgu::bf16_t>&, int64_t, hipStream_t);
