// The Riccati backward pass: all 24 kernels of the one body (ac_ilqr_backward_body.hpp) — k_ilqr_backward, k_ilqr_backward_shoot
// and k_ilqr_backward_rate, each <NODE, NEWTON, BOX> — and their one launcher (see ac_ilqr.hpp, ac_ilqr_rate.hpp, ac_boxqp.hpp).
#include "ac_ilqr_rate.hpp"

namespace ac {

template <bool NODE, bool NEWTON, bool BOX> static void launch_family(const IlqrBackwardArgs& a, hipStream_t st) {
    const int grid = (int)a.B;  // one wave per instance
    IlqrBoxOut<BOX> box;
    if constexpr (BOX) box = {a.act, a.stat};
    if (a.F)
        hipLaunchKernelGGL((k_ilqr_backward_shoot<NODE, NEWTON, BOX>), grid, 64, 0, st, a.C, a.N, a.X, a.U, a.A, a.Bm, a.Hz, a.B, a.H,
                           a.K, a.kff, a.dV, IlqrShootIn<true>{a.F, a.Vx, a.Vxx}, box);
    else if (a.rate_g)
        hipLaunchKernelGGL((k_ilqr_backward_rate<NODE, NEWTON, BOX>), grid, 64, 0, st, a.C, a.N, a.X, a.U, a.A, a.Bm, a.Hz, a.rate_g,
                           a.rate_h, a.B, a.H, a.K, a.Kp, a.kff, a.dV, box);
    else
        hipLaunchKernelGGL((k_ilqr_backward<NODE, NEWTON, BOX>), grid, 64, 0, st, a.C, a.N, a.X, a.U, a.A, a.Bm, a.Hz, a.B, a.H, a.K,
                           a.kff, a.dV, box);
}

template <bool NODE, bool NEWTON> static void launch(const IlqrBackwardArgs& a, hipStream_t st) {
    if (a.box) launch_family<NODE, NEWTON, true>(a, st);
    else launch_family<NODE, NEWTON, false>(a, st);
}

hipError_t ilqr_launch_backward(const IlqrBackwardArgs& a, hipStream_t st) {
    const bool node = a.N.q != nullptr;
    if (node && a.Hz) launch<true, true>(a, st);
    else if (node) launch<true, false>(a, st);
    else if (a.Hz) launch<false, true>(a, st);
    else launch<false, false>(a, st);
    return hipGetLastError();
}

}  // namespace ac
