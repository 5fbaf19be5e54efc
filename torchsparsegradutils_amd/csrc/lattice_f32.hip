// fp32 instantiations of the lattice plane-sweep kernels (own translation unit: compiles in parallel with the others).
#include "lattice_impl.h"

template int tsgu::lat_dispatch<float>(int, int, int, const tsgu::LatParams&, hipStream_t);
