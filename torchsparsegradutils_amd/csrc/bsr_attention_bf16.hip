// Block-sparse attention kernels for value type bf16 (every supported head width; index types at run time).
#include "bsr_attention_impl.h"

template int tsgu::bat_dispatch<tsgu::bf16_t>(int, int, const tsgu::BsrAttn<tsgu::bf16_t>&, int64_t, hipStream_t);
