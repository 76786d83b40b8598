// Airframe-gradient kernels of the default, linear and cubic-fit models: explicit instantiations (see the declarations at the end
// of ac_agrad.hpp).
#define AC_AGRAD_INSTANTIATE 1
#include "ac_agrad.hpp"
