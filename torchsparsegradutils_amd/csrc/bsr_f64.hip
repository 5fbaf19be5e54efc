// Block-sparse × dense kernels for value type double (index types int32 / int64).
#include "bsr_impl.h"

template int tsgu::bsr_mm_dispatch<double>(int, bool, const tsgu::BsrMM<double>&, hipStream_t);
template int tsgu::bsr_sddmm_dispatch<double>(int, const tsgu::BsrSddmm<double>&, int64_t, hipStream_t);
