// vjp_host.cpp — the fused reverse-mode kernels' per-unit code (aircraft_amd/csrc/ac_vjp.hpp: step_vjp_unit, deriv_vjp_unit)
// compiled for the HOST (g++, -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` checks the sub-step
// composition and the single normalisation adjoint against the float64 oracle without a GPU.  TEST INFRASTRUCTURE: nothing
// in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_vjp.hpp"

using namespace ac;

namespace {

template <int MODEL>
void run(const DevParams& P, int what, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
         float* Xbar, float* Ubar, float* dtbar) {
    std::vector<float> col((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn c{col.data(), 1};
    for (long u = 0; u < n; ++u) {
        float xv[13], uv[7], lam[13], gx[13], gu[7], gdt = 0.f;
        for (int i = 0; i < 13; ++i) { xv[i] = X[i * n + u]; lam[i] = Lam[i * n + u]; }
        for (int i = 0; i < 7; ++i) uv[i] = U[i * n + u];
        if (what == 0) step_vjp_unit<MODEL>(P, xv, uv, dt_per_unit ? dt[u] : dt[0], lam, c, gx, gu, gdt);
        else deriv_vjp_unit<MODEL>(P, xv, uv, lam, gx, gu);
        for (int i = 0; i < 13; ++i) Xbar[i * n + u] = gx[i];
        for (int i = 0; i < 7; ++i) Ubar[i * n + u] = gu[i];
        dtbar[u] = gdt;
    }
}

}  // namespace

// what: 0 = state_update (any number of sub-steps), 1 = f.  Arrays component-major like the device ABI: X [13][n], ...
// dt: [1] or, with dt_per_unit, [n].
extern "C" int host_vjp(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept, int what,
                        const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n, float* Xbar,
                        float* Ubar, float* dtbar) {
    DevParams P{};
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
    if (P.p.substeps > kVjpMaxSubsteps) return -1;
#define AC_CASE(M_) if (P.p.model_kind == M_) { run<M_>(P, what, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar); return 0; }
    AC_CASE(AC_MODEL_DEFAULT) AC_CASE(AC_MODEL_LINEAR) AC_CASE(AC_MODEL_POLY)
#undef AC_CASE
    return -2;
}
