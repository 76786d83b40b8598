// Fused reverse-mode kernels of the default / linear / cubic-fit models: explicit instantiations (see the declarations at the
// end of ac_vjp.hpp).
#define AC_VJP_INSTANTIATE 1
#include "ac_vjp.hpp"
