// Block-sparse × dense kernels for value type float (index types int32 / int64).
#include "bsr_impl.h"

template int tsgu::bsr_mm_dispatch<float>(int, bool, const tsgu::BsrMM<float>&, hipStream_t);
template int tsgu::bsr_sddmm_dispatch<float>(int, const tsgu::BsrSddmm<float>&, int64_t, hipStream_t);
