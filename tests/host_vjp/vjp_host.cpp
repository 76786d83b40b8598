// vjp_host.cpp — the fused reverse-mode kernels' lane code (aircraft_amd/csrc/ac_vjp.hpp: step_vjp_lane, deriv_vjp_unit)
// compiled for the HOST (g++, -DAC_HOST_CHECK) behind a small C API, so that `pytest -m "not gpu"` checks the sub-step
// composition and the single normalisation adjoint against the float64 oracle without a GPU.  TEST INFRASTRUCTURE: nothing
// in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include <vector>

#include "../../aircraft_amd/csrc/ac_vjp.hpp"
#include "../host_params.hpp"

using namespace ac;

namespace {

template <int MODEL>
void run(const DevParams& P, int what, const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n,
         float* Xbar, float* Ubar, float* dtbar) {
    std::vector<float> colv((size_t)vjp_lane_words(P.p.substeps));
    const VjpColumn col{colv.data(), 1};
    AdjAnalyticCoeffs<MODEL> coeffs;
    for (long i = 0; i < n; ++i) {
        if (what == 0) {  // (k_step_vjp's lane)
            step_vjp_lane(P, coeffs, col, X, U, dt[0], dt_per_unit ? dt : nullptr, Lam, n, i, Xbar, Ubar, dtbar);
            continue;
        }
        float x[13], u[7], w[13], gx[13], gu[7];
        load_rows<13>(X, n, i, x);
        load_rows<7>(U, n, i, u);
        load_rows<13>(Lam, n, i, w);
        deriv_vjp_unit<MODEL>(P, x, u, w, gx, gu);
        store_rows<13>(Xbar, n, i, gx);
        store_rows<7>(Ubar, n, i, gu);
        dtbar[i] = 0.f;
    }
}

}  // namespace

// what: 0 = state_update (any number of sub-steps), 1 = f.  Arrays component-major like the device ABI: X [13][n], ...
// dt: [1] or, with dt_per_unit, [n].
extern "C" int host_vjp(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept, int what,
                        const float* X, const float* U, const float* dt, int dt_per_unit, const float* Lam, long n, float* Xbar,
                        float* Ubar, float* dtbar) {
    const DevParams P = host_dev_params(p, linear_W, poly_coef, poly_intercept);
    if (P.p.substeps > kVjpMaxSubsteps) return -1;
#define AC_CASE(M_) if (P.p.model_kind == M_) { run<M_>(P, what, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar); return 0; }
    AC_CASE(AC_MODEL_DEFAULT) AC_CASE(AC_MODEL_LINEAR) AC_CASE(AC_MODEL_POLY)
#undef AC_CASE
    return -2;
}
