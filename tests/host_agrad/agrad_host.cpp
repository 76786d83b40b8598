// agrad_host.cpp — the recording airframe provider and the sub-step reverse sweep of the airframe gradient
// (aircraft_amd/csrc/ac_agrad.hpp: RecAirframe over step_vjp_unit) compiled for the HOST (g++, -DAC_HOST_CHECK) behind a small C
// API, so that `pytest -m "not gpu"` checks the gradient over mass, inertia and com against the float64 oracle without a GPU.
// Every sample of every unit is added into ONE fp32 chain per parameter (the least favourable summation order; the kernels'
// per-lane partials are shorter chains).  TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_agrad.hpp"

using namespace ac;

namespace {

bool setup(DevParams& P, const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept) {
    P.p = *p;
    if (linear_W) for (int i = 0; i < 36; ++i) P.linear_W[i] = linear_W[i];
    alignas(64) static thread_local float tab[kPolyTabFloats];
    if (poly_coef && poly_intercept) {
        float grad[6 * 4 * 15], hess[6 * 10 * 5];
        poly_gradient_tables(poly_coef, grad);
        poly_hessian_tables(grad, hess);
        poly_pack_tables(poly_coef, poly_intercept, grad, hess, tab);
        P.poly_tab = tab;
    }
    return P.p.substeps <= kAgradMaxSubsteps;
}

template <int MODEL>
void run_step(const DevParams& P, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
              float* Xbar, float* Ubar, float* dtbar, float* Phibar) {
    for (int i = 0; i < kAgradFloats; ++i) Phibar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecAirframe<MODEL, CgradColumn> coeffs(CgradColumn{Phibar, 1});
    for (long k = 0; k < n; ++k) {
        float xv[13], uv[7], lam[13], gx[13], gu[7], gdt = 0.f;
        for (int i = 0; i < 13; ++i) { xv[i] = X[i * n + k]; lam[i] = Lam[i * n + k]; }
        for (int i = 0; i < 7; ++i) uv[i] = U[i * n + k];
        step_vjp_unit(P, coeffs, xv, uv, dt_per_unit ? dt[k] : dt[0], lam, col, gx, gu, gdt);
        for (int i = 0; i < 13; ++i) Xbar[i * n + k] = gx[i];
        for (int i = 0; i < 7; ++i) Ubar[i * n + k] = gu[i];
        dtbar[k] = gdt;
    }
}

// k_rollout_agrad's recurrence over a saved trajectory: lambda_H = G_H, lambda_k = G_k + A_k' lambda_{k+1}
template <int MODEL>
void run_rollout(const DevParams& P, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                 float* Ubar, float* dtbar, float* Phibar) {
    for (int i = 0; i < kAgradFloats; ++i) Phibar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecAirframe<MODEL, CgradColumn> coeffs(CgradColumn{Phibar, 1});
    for (long b = 0; b < B; ++b) {
        float lam[13], gsum = 0.f;
        for (int i = 0; i < 13; ++i) lam[i] = G[(H * 13 + i) * B + b];
        for (long k = H - 1; k >= 0; --k) {
            float xv[13], uv[7], gx[13], gu[7], gdt = 0.f;
            for (int i = 0; i < 13; ++i) xv[i] = Xtraj[(k * 13 + i) * B + b];
            for (int i = 0; i < 7; ++i) uv[i] = U[(k * 7 + i) * B + b];
            step_vjp_unit(P, coeffs, xv, uv, dt, lam, col, gx, gu, gdt);
            for (int i = 0; i < 7; ++i) Ubar[(k * 7 + i) * B + b] = gu[i];
            gsum += gdt;
            for (int i = 0; i < 13; ++i) lam[i] = G[(k * 13 + i) * B + b] + gx[i];
        }
        for (int i = 0; i < 13; ++i) X0bar[i * B + b] = lam[i];
        dtbar[b] = gsum;
    }
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
    DevParams P{};
    if (!setup(P, p, linear_W, poly_coef, poly_intercept)) return -1;
    AC_AGRAD_HOST_DISPATCH(run_step, P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Phibar)
}

// Xtraj [H+1][13][B], U [H][7][B], G [H+1][13][B] -> X0bar [13][B], Ubar [H][7][B], dtbar [B], Phibar [22]
extern "C" int host_rollout_agrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                                  const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                                  float* Ubar, float* dtbar, float* Phibar) {
    DevParams P{};
    if (!setup(P, p, linear_W, poly_coef, poly_intercept)) return -1;
    AC_AGRAD_HOST_DISPATCH(run_rollout, P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Phibar)
}
