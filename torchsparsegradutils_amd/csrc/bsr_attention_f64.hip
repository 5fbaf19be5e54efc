// Block-sparse attention kernels for value type double (every supported head width; index types at run time).
#include "bsr_attention_impl.h"

template int tsgu::bat_dispatch<double>(int, int, const tsgu::BsrAttn<double>&, int64_t, hipStream_t);
