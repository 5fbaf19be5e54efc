// K3 instantiations for value type float (index types int32 / int64).
#include "sddmm_impl.h"

template int tsgu::sddmm_dispatch<float>(int, const tsgu::SddmmParams&, int64_t, hipStream_t);
template int tsgu::coo_sddmm_dispatch<float>(int, const tsgu::CooSddmmParams&, hipStream_t);
