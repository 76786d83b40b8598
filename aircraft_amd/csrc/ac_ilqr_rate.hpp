// ac_ilqr_rate.hpp — the control-RATE term  sum_k rho_k(u_k - u_{k-1})  modelled exactly in the Riccati pass.
//
// The value function carries the previous control: V_k(x_k, p_k), p_k = u_{k-1}.  The 13 states and the 7 previous
// controls form a 20-wide augmented state z with  A_z = [[A, 0], [0, 0]],  B_z = [[B], [I]]; the structure is exploited,
// the 20-wide matrices are never formed.  Per node the kernel receives  g = rho_k'(d_k),  h = rho_k''(d_k) >= 0 (diagonal),
// both [H][7][B], d_k = u_k - u_{k-1}; row 0 is the term against the control applied before the window (zeros: none).
// A primed symbol is the value of node k + 1:
//
//   Qx  = l_x + A'V'x                       Qu  = l_u + B'V'x + V'p + g             Qp  = -g
//   Qxx = diag(q) + A'V'xx A [+ Hz_xx]      Qux = (B'V'xx + V'px) A [+ Hz_ux]       Qxp = 0
//   Quu = diag(r + reg) + B'V'xx B + B'V'xp + V'px B + V'pp + diag(h) [+ Hz_uu]     (symmetrised)
//   Qup = -diag(h)                          Qpp = diag(h)
//   [Kx | Kp | k] = -Quu^-1 [Qux | Qup | Qu]
//   Vx  = Qx + Kx'(Quu k + Qu) + Qux'k      Vp  = Qp + Kp'(Quu k + Qu) + Qup'k
//   Vxx = Qxx + Kx'Quu Kx + Kx'Qux + Qux'Kx         Vxp = Kx'Quu Kp + Kx'Qup + Qux'Kp
//   Vpp = Qpp + Kp'Quu Kp + Kp'Qup + Qup'Kp         (Vxx, Vpp symmetrised);  terminal: Vp = 0, Vxp = 0, Vpp = 0
//
// and the closed loop applies  u_k = clip(U_k + alpha k_k + Kx_k (x - Xnom_k) + Kp_k (u_applied_{k-1} - U_{k-1}))
// (Policy::Kp, ac_ilqr.hpp).  Built the way k_ilqr_backward is: one wave per instance, node inputs gathered by LDS-DMA
// into a counted-vmcnt ring; g and h (14 floats) travel in the ring as one more 14-lane instruction per node.
// The kernel IS k_ilqr_backward's body (ac_ilqr_backward_body.hpp) under its AC_ILQR_RATE switch: the terms above are the
// switched blocks, everything else (ring, Cholesky, BOX hook, V_x / V_xx) is the one copy.
#pragma once
#include "ac_ilqr.hpp"

namespace ac {

template <bool NODE, bool NEWTON, bool BOX = false>  // BOX: the control box as a QP per node (IlqrBoxNode, ac_ilqr.hpp)
__global__ __launch_bounds__(64) void k_ilqr_backward_rate(const IlqrCost C, const NodeCost N, const float* __restrict__ X,
                                                           const float* __restrict__ U, const float* __restrict__ A,
                                                           const float* __restrict__ Bm, const float* __restrict__ Hz,
                                                           const float* __restrict__ rate_g, const float* __restrict__ rate_h,
                                                           long B, long H, float* __restrict__ K, float* __restrict__ Kp,
                                                           float* __restrict__ kff, float* __restrict__ dV,
                                                           const IlqrBoxOut<BOX> box = {}) {
#define AC_ILQR_SHOOT 0
#define AC_ILQR_RATE 1
#include "ac_ilqr_backward_body.hpp"
#undef AC_ILQR_RATE
#undef AC_ILQR_SHOOT
}

// ---- quadratic rate cost  1/2 sum_k sum_i w_i (u_{k,i} - u_{k-1,i})^2,  u_{-1} = u_prev [7][Bn] (NULL: no k = 0 term) ----
struct RateWeights {
    float w[7];
};

// its model for the pass above: g = w d, h = w; one lane per (node, instance); row 0 all zeros without u_prev
__global__ __launch_bounds__(kBlock) void k_ilqr_rate_model(const RateWeights W, const float* __restrict__ U,
                                                            const float* __restrict__ u_prev, long B, long H,
                                                            float* __restrict__ rate_g, float* __restrict__ rate_h);
// cost[o] += the term of column o of a candidate batch U [H][7][B] (instance o % Bn owns the previous control)
__global__ __launch_bounds__(kBlock) void k_ilqr_rate_cost(const RateWeights W, const float* __restrict__ U,
                                                           const float* __restrict__ u_prev, long Bn, long B, long H,
                                                           float* __restrict__ cost);

hipError_t ilqr_rate_launch_model(const RateWeights& W, const float* U, const float* u_prev, long B, long H, float* rate_g,
                                  float* rate_h, hipStream_t st, int* grid);
hipError_t ilqr_rate_launch_cost(const RateWeights& W, const float* U, const float* u_prev, long Bn, long B, long H, float* cost,
                                 hipStream_t st, int* grid);

}  // namespace ac
