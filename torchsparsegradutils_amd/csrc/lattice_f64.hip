// fp64 instantiations of the lattice plane-sweep kernels (own translation unit: compiles in parallel with the others).
// Dense rows of p doubles = p/2 chunks of 16 bytes: p in {4, 8, 16, 32}.
#include "lattice_impl.h"

template int tsgu::lat_dispatch<double>(int, int, int, const tsgu::LatParams&, hipStream_t);
