// host_params.hpp — the DevParams of a host twin (tests/host_vjp, host_cgrad, host_agrad) from the arguments their C APIs
// share: ac_params, the linear model's W [36] and the cubic fits' coef [6][34] / intercept [6] (each nullable).  Include after
// the csrc header under test, with AC_HOST_CHECK defined.  TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#pragma once

namespace ac {

inline DevParams host_dev_params(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept) {
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
    return P;
}

}  // namespace ac
