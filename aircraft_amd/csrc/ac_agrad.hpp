// ac_agrad.hpp — gradients of step and rollout losses with respect to the AIRFRAME CONSTANTS: mass, inertia, inertia_inv and
// the centre of mass.
//
// The raw parameters are the 22 floats of ac_params that enter f, each treated as an independent number:
//   phi = [ mass | inertia[9] row-major | inertia_inv[9] row-major | com[3] ]          (AC_AIRFRAME_GRAD_FLOATS)
// (that inertia depends on mass and com, and inertia_inv on inertia, is the caller's chain rule: autodiff.AirframeParameters).
// For L = lambda . F(x, u, dt; phi) the fused reverse sweep (step_vjp_unit, ac_vjp.hpp) visits every RK4 stage of every sub-step
// once; f_vjp hands a provider that declares kRecordsAirframe the factors it holds there (w: the stage cotangent):
//   v_dot = Fn / m + g                         mass_bar        += -(Fn . w[3:6]) / m^2
//   I omega enters y = omega x (I omega)       I_bar[i][j]     += c2[i] omega[j]        c2 = y_bar x omega
//   omega_dot = I^-1 rhs                       Iinv_bar[i][j]  += w[10 + i] rhs[j]
//   M = Ma + com x F                           com_bar         += F x M_bar
// The accumulators, their reduction and the grid are those of the coefficient gradient (ac_cgrad.hpp): one LDS column of 22
// words per lane in front of the VjpColumn words, columns added per workgroup in a fixed order (cgrad_store_partial), partials
// added in workgroup order (k_wgrad_reduce).  No floating-point atomics.  This header holds the provider (RecAirframe) and the
// kernels' instantiations; the sweeps themselves are cgrad_step_sweep / cgrad_rollout_sweep of ac_cgrad.hpp.
#pragma once
#include "ac_cgrad.hpp"

namespace ac {

constexpr int kAgradFloats = 22;
// LDS words per lane: 22 + 30 + 13 ns <= 640 would allow ns = 45; the sweep itself stops at kVjpMaxSubsteps = 40.
constexpr int kAgradMaxSubsteps = kVjpMaxSubsteps;

template <int MODEL, class Sink> struct RecAirframe : AdjAnalyticCoeffs<MODEL> {
    static constexpr bool kRecordsAirframe = true;
    Sink sink;
    AC_DI explicit RecAirframe(const Sink& s) : sink(s) {}
    // f_vjp's locals at one stage: Fn = R F, w [13] the stage cotangent, om = omega, c2 = y_bar x omega, rhs = M - omega x I omega,
    // F the body force, Mb the cotangent of M
    AC_DI void record_airframe(const DevParams& P, const float Fn[3], const float w[13], const float om[3], const float c2[3],
                               const float rhs[3], const float F[3], const float Mb[3]) const {
        const float im = 1.0f / P.p.mass;
        sink.add(0, -(im * im) * (Fn[0] * w[3] + Fn[1] * w[4] + Fn[2] * w[5]));
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                sink.add(1 + 3 * i + j, c2[i] * om[j]);
                sink.add(10 + 3 * i + j, w[10 + i] * rhs[j]);
            }
        }
        float cb[3];
        cross3(F, Mb, cb);
#pragma unroll
        for (int k = 0; k < 3; ++k) sink.add(19 + k, cb[k]);
    }
};

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {

// The sweeps of ac_cgrad.hpp with the airframe provider: partial [gridDim.x][22]; Xbar / X0bar, Ubar, dtbar nullable.  Dynamic
// LDS: cgrad_lane_words(22, ns) floats per lane.
template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_step_agrad(const DevParams P, const float* __restrict__ X, const float* __restrict__ U,
                                                          float dt, const float* __restrict__ dt_per_unit,
                                                          const float* __restrict__ Lam, long n, float* __restrict__ Xbar,
                                                          float* __restrict__ Ubar, float* __restrict__ dtbar,
                                                          float* __restrict__ partial) {
    cgrad_step_sweep<kAgradFloats, RecAirframe<MODEL, CgradColumn>>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, partial);
}
template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_rollout_agrad(const DevParams P, const float* __restrict__ Xtraj,
                                                             const float* __restrict__ U, float dt, long B, long H,
                                                             const float* __restrict__ G, float* __restrict__ X0bar,
                                                             float* __restrict__ Ubar, float* __restrict__ dtbar,
                                                             float* __restrict__ partial) {
    cgrad_rollout_sweep<kAgradFloats, RecAirframe<MODEL, CgradColumn>>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, partial);
}

// The kernels are compiled in a translation unit of their own (an_inst_agrad.hip); every other unit only refers to them.
#define AC_AGRAD_MODEL(EXT, M)                                         \
    EXT template __global__ void k_step_agrad<M>(AC_CGRAD_STEP_ARGS);  \
    EXT template __global__ void k_rollout_agrad<M>(AC_CGRAD_ROLL_ARGS);
#ifdef AC_AGRAD_INSTANTIATE
AC_AGRAD_MODEL(, AC_MODEL_DEFAULT) AC_AGRAD_MODEL(, AC_MODEL_LINEAR) AC_AGRAD_MODEL(, AC_MODEL_POLY)
#else
AC_AGRAD_MODEL(extern, AC_MODEL_DEFAULT) AC_AGRAD_MODEL(extern, AC_MODEL_LINEAR) AC_AGRAD_MODEL(extern, AC_MODEL_POLY)
#endif
#undef AC_AGRAD_MODEL

}  // namespace ac
#endif  // AC_HOST_CHECK
