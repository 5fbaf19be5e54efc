// K1/K2 instantiations for value type double (index types int32 / int64).
#include "spmm_impl.h"

template int tsgu::spmm_dispatch<double>(int, const tsgu::SpmmParams&, int64_t, hipStream_t);
