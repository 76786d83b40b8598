// cgrad_host.cpp — the recording coefficient provider and the sub-step reverse sweep of the coefficient gradient
// (aircraft_amd/csrc/ac_cgrad.hpp: RecCoeffs in step_vjp_lane / rollout_vjp_lane, the kernels' own lane code) compiled for the HOST
// (g++, -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` checks the parameter gradient against the float64 oracle without a GPU.  Every sample of
// every unit is added into ONE fp32 chain per parameter (the least favourable summation order; the kernels' per-lane partials
// are shorter chains).  TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_cgrad.hpp"
#include "../host_params.hpp"

using namespace ac;

namespace {

// (k_step_cgrad's lane over every unit)
template <int MODEL>
void run_step(const DevParams& P, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
              float* Xbar, float* Ubar, float* dtbar, float* Thetabar) {
    for (int i = 0; i < CgradFloats<MODEL>::value; ++i) Thetabar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecCoeffs<MODEL, CgradColumn> coeffs(CgradColumn{Thetabar, 1});
    for (long i = 0; i < n; ++i) step_vjp_lane(P, coeffs, col, X, U, dt[0], dt_per_unit ? dt : nullptr, Lam, n, i, Xbar, Ubar, dtbar);
}

// (k_rollout_cgrad's lane over every instance of a saved trajectory)
template <int MODEL>
void run_rollout(const DevParams& P, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                 float* Ubar, float* dtbar, float* Thetabar) {
    for (int i = 0; i < CgradFloats<MODEL>::value; ++i) Thetabar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecCoeffs<MODEL, CgradColumn> coeffs(CgradColumn{Thetabar, 1});
    for (long i = 0; i < B; ++i) rollout_vjp_lane(P, coeffs, col, Xtraj, U, dt, B, H, G, i, X0bar, Ubar, dtbar);
}

}  // namespace

// Arrays component-major like the device ABI: X [13][n], ...; dt [1] or, with dt_per_unit, [n].  Thetabar [210] (poly: coef
// [6][34], intercept [6]) or [36] (linear).  Returns 0, -1 (too many sub-steps) or -2 (no coefficient gradient for the model).
extern "C" int host_step_cgrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                               const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
                               float* Xbar, float* Ubar, float* dtbar, float* Thetabar) {
    const DevParams P = host_dev_params(p, linear_W, poly_coef, poly_intercept);
    if (P.p.substeps > kCgradMaxSubsteps) return -1;
    if (P.p.model_kind == AC_MODEL_LINEAR) { run_step<AC_MODEL_LINEAR>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Thetabar); return 0; }
    if (P.p.model_kind == AC_MODEL_POLY) { run_step<AC_MODEL_POLY>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Thetabar); return 0; }
    return -2;
}

// Xtraj [H+1][13][B], U [H][7][B], G [H+1][13][B] -> X0bar [13][B], Ubar [H][7][B], dtbar [B], Thetabar
extern "C" int host_rollout_cgrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                                  const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                                  float* Ubar, float* dtbar, float* Thetabar) {
    const DevParams P = host_dev_params(p, linear_W, poly_coef, poly_intercept);
    if (P.p.substeps > kCgradMaxSubsteps) return -1;
    if (P.p.model_kind == AC_MODEL_LINEAR) { run_rollout<AC_MODEL_LINEAR>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Thetabar); return 0; }
    if (P.p.model_kind == AC_MODEL_POLY) { run_rollout<AC_MODEL_POLY>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Thetabar); return 0; }
    return -2;
}
