// Block-sparse × dense kernels for value type bf16_t (index types int32 / int64).
#include "bsr_impl.h"

template int tsgu::bsr_mm_dispatch<tsgu::bf16_t>(int, bool, const tsgu::BsrMM<tsgu::bf16_t>&, hipStream_t);
template int tsgu::bsr_sddmm_dispatch<tsgu::bf16_t>(int, const tsgu::BsrSddmm<tsgu::bf16_t>&, int64_t, hipStream_t);
