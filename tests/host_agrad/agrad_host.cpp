// agrad_host.cpp — the recording airframe provider and the sub-step reverse sweep of the airframe gradient
// (aircraft_amd/csrc/ac_agrad.hpp: RecAirframe in step_vjp_lane / rollout_vjp_lane, the kernels' own lane code) compiled for the HOST
// (g++, -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` checks the gradient over mass, inertia and com against the float64 oracle without a GPU.
// Every sample of every unit is added into ONE fp32 chain per parameter (the least favourable summation order; the kernels'
// per-lane partials are shorter chains).  TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_agrad.hpp"
#include "../host_params.hpp"

using namespace ac;

namespace {

// (k_step_agrad's lane over every unit)
template <int MODEL>
void run_step(const DevParams& P, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
              float* Xbar, float* Ubar, float* dtbar, float* Phibar) {
    for (int i = 0; i < kAgradFloats; ++i) Phibar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecAirframe<MODEL, CgradColumn> coeffs(CgradColumn{Phibar, 1});
    for (long i = 0; i < n; ++i) step_vjp_lane(P, coeffs, col, X, U, dt[0], dt_per_unit ? dt : nullptr, Lam, n, i, Xbar, Ubar, dtbar);
}

// (k_rollout_agrad's lane over every instance of a saved trajectory)
template <int MODEL>
void run_rollout(const DevParams& P, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                 float* Ubar, float* dtbar, float* Phibar) {
    for (int i = 0; i < kAgradFloats; ++i) Phibar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecAirframe<MODEL, CgradColumn> coeffs(CgradColumn{Phibar, 1});
    for (long i = 0; i < B; ++i) rollout_vjp_lane(P, coeffs, col, Xtraj, U, dt, B, H, G, i, X0bar, Ubar, dtbar);
}

}  // namespace

#define AC_AGRAD_HOST_DISPATCH(FN, ...)                                                            \
    switch (P.p.model_kind) {                                                                      \
        case AC_MODEL_DEFAULT: FN<AC_MODEL_DEFAULT>(__VA_ARGS__); return 0;                        \
        case AC_MODEL_LINEAR: FN<AC_MODEL_LINEAR>(__VA_ARGS__); return 0;                          \
        case AC_MODEL_POLY: FN<AC_MODEL_POLY>(__VA_ARGS__); return 0;                              \
        default: return -2;                                                                        \
    }

// Arrays component-major like the device ABI: X [13][n], ...; dt [1] or, with dt_per_unit, [n].  Phibar [22]: mass, inertia [9],
// inertia_inv [9], com [3].  Returns 0, -1 (too many sub-steps) or -2 (no airframe gradient for the model).
extern "C" int host_step_agrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                               const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
                               float* Xbar, float* Ubar, float* dtbar, float* Phibar) {
    const DevParams P = host_dev_params(p, linear_W, poly_coef, poly_intercept);
    if (P.p.substeps > kAgradMaxSubsteps) return -1;
    AC_AGRAD_HOST_DISPATCH(run_step, P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Phibar)
}

// Xtraj [H+1][13][B], U [H][7][B], G [H+1][13][B] -> X0bar [13][B], Ubar [H][7][B], dtbar [B], Phibar [22]
extern "C" int host_rollout_agrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                                  const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                                  float* Ubar, float* dtbar, float* Phibar) {
    const DevParams P = host_dev_params(p, linear_W, poly_coef, poly_intercept);
    if (P.p.substeps > kAgradMaxSubsteps) return -1;
    AC_AGRAD_HOST_DISPATCH(run_rollout, P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Phibar)
}
