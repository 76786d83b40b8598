// Coefficient-gradient kernels of the linear and cubic-fit models: explicit instantiations (see the declarations at the end of
// ac_cgrad.hpp).
#define AC_CGRAD_INSTANTIATE 1
#include "ac_cgrad.hpp"
