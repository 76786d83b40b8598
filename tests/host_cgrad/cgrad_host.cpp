// cgrad_host.cpp — the recording coefficient provider and the sub-step reverse sweep of the coefficient gradient
// (aircraft_amd/csrc/ac_cgrad.hpp: RecCoeffs over step_vjp_unit) compiled for the HOST (g++, -DAC_HOST_CHECK) behind a small C
// API, so that `pytest -m "not gpu"` checks the parameter gradient against the float64 oracle without a GPU.  Every sample of
// every unit is added into ONE fp32 chain per parameter (the least favourable summation order; the kernels' per-lane partials
// are shorter chains).  TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_cgrad.hpp"

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
    return P.p.substeps <= kCgradMaxSubsteps;
}

template <int MODEL>
void run_step(const DevParams& P, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
              float* Xbar, float* Ubar, float* dtbar, float* Thetabar) {
    constexpr int PF = CgradFloats<MODEL>::value;
    for (int i = 0; i < PF; ++i) Thetabar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecCoeffs<MODEL, CgradColumn> coeffs(CgradColumn{Thetabar, 1});
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

// k_rollout_cgrad's recurrence over a saved trajectory: lambda_H = G_H, lambda_k = G_k + A_k' lambda_{k+1}
template <int MODEL>
void run_rollout(const DevParams& P, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                 float* Ubar, float* dtbar, float* Thetabar) {
    constexpr int PF = CgradFloats<MODEL>::value;
    for (int i = 0; i < PF; ++i) Thetabar[i] = 0.f;
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    RecCoeffs<MODEL, CgradColumn> coeffs(CgradColumn{Thetabar, 1});
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

// Arrays component-major like the device ABI: X [13][n], ...; dt [1] or, with dt_per_unit, [n].  Thetabar [210] (poly: coef
// [6][34], intercept [6]) or [36] (linear).  Returns 0, -1 (too many sub-steps) or -2 (no coefficient gradient for the model).
extern "C" int host_step_cgrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                               const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
                               float* Xbar, float* Ubar, float* dtbar, float* Thetabar) {
    DevParams P{};
    if (!setup(P, p, linear_W, poly_coef, poly_intercept)) return -1;
    if (P.p.model_kind == AC_MODEL_LINEAR) { run_step<AC_MODEL_LINEAR>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Thetabar); return 0; }
    if (P.p.model_kind == AC_MODEL_POLY) { run_step<AC_MODEL_POLY>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar, Thetabar); return 0; }
    return -2;
}

// Xtraj [H+1][13][B], U [H][7][B], G [H+1][13][B] -> X0bar [13][B], Ubar [H][7][B], dtbar [B], Thetabar
extern "C" int host_rollout_cgrad(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                                  const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                                  float* Ubar, float* dtbar, float* Thetabar) {
    DevParams P{};
    if (!setup(P, p, linear_W, poly_coef, poly_intercept)) return -1;
    if (P.p.model_kind == AC_MODEL_LINEAR) { run_rollout<AC_MODEL_LINEAR>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Thetabar); return 0; }
    if (P.p.model_kind == AC_MODEL_POLY) { run_rollout<AC_MODEL_POLY>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Thetabar); return 0; }
    return -2;
}
