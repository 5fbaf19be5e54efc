// Block-sparse attention kernels for value type float (every supported head width; index types at run time).
#include "bsr_attention_impl.h"

template int tsgu::bat_dispatch<float>(int, int, const tsgu::BsrAttn<float>&, int64_t, hipStream_t);
