// The box-constrained (control-limited) Riccati pass: k_ilqr_backward<NODE, NEWTON, true> and
// k_ilqr_backward_rate<NODE, NEWTON, true>, all eight, and their launcher (see ac_ilqr.hpp, ac_ilqr_rate.hpp, ac_boxqp.hpp).
#include "ac_ilqr_rate.hpp"

namespace ac {

hipError_t ilqr_box_launch_backward(const IlqrCost& C, const NodeCost& N, const float* X, const float* U, const float* A,
                                    const float* Bm, const float* Hz, const float* rate_g, const float* rate_h, long B, long H,
                                    float* K, float* Kp, float* kff, float* dV, signed char* act, int* stat, hipStream_t st) {
    const int grid = (int)B;  // one wave per instance
    const IlqrBoxOut<true> box{act, stat};
#define AC_BACKWARD_BOX(NODE_, NEWTON_)                                                                                           \
    do {                                                                                                                          \
        if (rate_g)                                                                                                               \
            hipLaunchKernelGGL((k_ilqr_backward_rate<NODE_, NEWTON_, true>), grid, 64, 0, st, C, N, X, U, A, Bm, Hz, rate_g, rate_h, \
                               B, H, K, Kp, kff, dV, box);                                                                        \
        else                                                                                                                      \
            hipLaunchKernelGGL((k_ilqr_backward<NODE_, NEWTON_, true>), grid, 64, 0, st, C, N, X, U, A, Bm, Hz, B, H, K, kff, dV,  \
                               box);                                                                                              \
    } while (0)
    const bool node = N.q != nullptr;
    if (node && Hz) AC_BACKWARD_BOX(true, true);
    else if (node) AC_BACKWARD_BOX(true, false);
    else if (Hz) AC_BACKWARD_BOX(false, true);
    else AC_BACKWARD_BOX(false, false);
#undef AC_BACKWARD_BOX
    return hipGetLastError();
}

}  // namespace ac
