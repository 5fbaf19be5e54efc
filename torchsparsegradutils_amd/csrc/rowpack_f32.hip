// Row-pair gather kernels: fp32 instantiations (one translation unit per value type for build parallelism).
#include "rowpack_impl.h"

template int tsgu::rp_dispatch<float>(int, bool, int, const tsgu::RpParams&, hipStream_t);
