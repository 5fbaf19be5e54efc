// Row-pair gather kernels: bf16 instantiations (values and dense operands bf16, accumulation fp32) (one translation unit per value type for build parallelism).
#include "rowpack_impl.h"

template int tsgu::rp_dispatch<tsgu::bf16_t>(int, bool, int, const tsgu::RpParams&, hipStream_t);
