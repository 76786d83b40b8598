// ac_shoot.hpp — Gauss-Newton multiple shooting on top of the Riccati pass (Giftthaler et al. 2018, "A family of iterative
// Gauss-Newton shooting methods"): launchers of the kernels of ilqr_shoot_inst.hip.
//
// The iterate is (X, U) with X[0] = x0; node k has the gap  d_k = F(x_k, u_k) - x_{k+1}  (ac_shoot_defect_f32 returns R_k = -d_k).
//   backward   k_ilqr_backward_shoot<NODE, NEWTON, BOX> (ac_ilqr.hpp, ilqr_backward_inst.hip): node k reads  v = V'_x + V'_xx d_k  in place of V'_x
//   direction  dx_0 = 0,  du_k = kff_k + K_k dx_k (optionally clipped so that U + du stays in the box),
//              dx_{k+1} = A_k dx_k + B_k du_k + d_k,  lam_k = V_x^{k+1} + V_xx^{k+1} dx_{k+1}
//              — the solution of the equality-constrained QP and the multipliers of its defect rows
//   candidates X + alpha dX, clip(U + alpha dU) for every alpha: all their nodes are independent (ONE ac_shoot_defect_f32 launch)
//   merit      phi = J + mu_b sum |R|,  mu_b <- max(mu_b, factor max |lam|)  (the exact L1 penalty)
#pragma once
#include "ac_ilqr.hpp"

namespace ac {

hipError_t shoot_launch_direction(const IlqrCost& C, bool clip, const float* X, const float* U, const float* F, const float* A,
                                  const float* Bm, const float* K, const float* kff, const float* Vx, const float* Vxx, long B, long H,
                                  float* dX, float* dU, float* Lam, hipStream_t st, int* grid);
hipError_t shoot_launch_merit_weight(const float* Lam, float factor, long B, long H, float* mu, hipStream_t st, int* grid);
hipError_t shoot_launch_candidates(const IlqrCost& C, const float* X, const float* U, const float* dX, const float* dU,
                                   const AlphaSet& al, long B, long H, float* Xc, float* Uc, hipStream_t st, int* grid);
hipError_t shoot_launch_merit(const float* J, const float* mu, long Bn, const float* R, const float* F, const float* X, long B, long H,
                              float* phi, float* defect_inf, hipStream_t st, int* grid);

}  // namespace ac
