// bf16 instantiations of the lattice plane-sweep kernels (fp32 accumulation).
#include "lattice_impl.h"

template int tsgu::lat_dispatch<tsgu::bf16_t>(int, int, int, const tsgu::LatParams&, hipStream_t);
