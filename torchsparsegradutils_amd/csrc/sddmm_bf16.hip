// K3 instantiations for value type bf16_t (index types int32 / int64).
#include "sddmm_impl.h"

template int tsgu::sddmm_dispatch<tsgu::bf16_t>(int, const tsgu::SddmmParams&, int64_t, hipStream_t);
template int tsgu::coo_sddmm_dispatch<tsgu::bf16_t>(int, const tsgu::CooSddmmParams&, hipStream_t);
