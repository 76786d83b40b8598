// Steady-flight trim: k_trim_assemble and k_trim_update (see the declarations at the end of ac_trim.hpp).
#define AC_TRIM_INSTANTIATE 1
#include "ac_trim.hpp"
