// trim_host.cpp — the trim's per-unit code (aircraft_amd/csrc/ac_trim.hpp) compiled for the HOST (g++, -DAC_HOST_CHECK)
// together with the host-compilable state_derivative of the analytic models, behind a small C API, so that
// `pytest -m "not gpu"` checks the assembly, the Jacobian J_z and the whole LM loop against the float64 oracle without a
// GPU.  The derivative sensitivities are formed like the device's k_deriv_sens (state_derivative in Dual<4> lane groups).
// For the step-by-step tests (tests/test_trim_steps_ref.py, tests/test_gpu_trim_steps.py): trim_residual_jacobian on given
// sensitivities, trim_step and trim_final_status on given inputs (the fp32 side of e32), and the whole solve with what
// the device's workspace holds after it.
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#include "../../aircraft_amd/csrc/ac_trim.hpp"

using namespace ac;

namespace {

DevParams make_params(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept) {
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

// f, df/dx [13][13], df/du [13][7] of one unit (directions: struct SeedsT in ac_dynamics.hpp)
template <int MODEL> void unit_deriv_sens(const DevParams& P, const float xv[13], const float uv[7], float xd[13], float Fx[169],
                                          float Fu[91]) {
    constexpr int N = 4;
    for (int i = 0; i < 169; ++i) Fx[i] = 0.f;
    for (int i = 0; i < 91; ++i) Fu[i] = 0.f;
    AnalyticCoeffs<MODEL> coeffs;
    for (int g = 0; g < 16 / N; ++g) {
        Dual<N> xs[13], u[7], k[13];
        for (int i = 0; i < 13; ++i) xs[i] = SeedsT<N>::state(g, i, xv[i]);
        SeedsT<N>::template controls<false>(g, uv, u);
        state_derivative(P, coeffs, xs, u, k);
        for (int j = 0; j < N; ++j) {
            const int d = N * g + j;
            for (int i = 0; i < 13; ++i) {
                if (d < 10) Fx[i * 13 + 3 + d] = k[i].d[j];
                else if (d < 13) Fu[i * 7 + (d - 10)] = k[i].d[j];
                else if (d == 13) Fu[i * 7 + 6] = k[i].d[j];
            }
        }
        for (int i = 0; i < 13; ++i) xd[i] = k[i].v;
    }
}

void load_unit(const float* target, const float* Uhold, long n, long u, TrimTarget& t, float uh[4]) {
    t = trim_target(target, n, u);
    for (int k = 0; k < 4; ++k) uh[k] = Uhold[(3 + k) * n + u];
}

template <int MODEL> void jac(const DevParams& P, int lateral, const float* target, const float* Uhold, const float* Z, long n,
                              float* R, float* J) {
    for (long u = 0; u < n; ++u) {
        TrimTarget t;
        float uh[4], z[6], x[13], uv[7], xd[13], fx[169], fu[91], r[6], jz[36];
        load_unit(target, Uhold, n, u, t, uh);
        for (int j = 0; j < 6; ++j) z[j] = Z[j * n + u];
        trim_assemble(t, lateral, z, uh, x, uv);
        unit_deriv_sens<MODEL>(P, x, uv, xd, fx, fu);
        trim_residual_jacobian(t, lateral, z, TrimSens{xd, fx, fu, 1}, r, jz);
        for (int i = 0; i < 6; ++i) R[i * n + u] = r[i];
        for (int k = 0; k < 36; ++k) J[k * n + u] = jz[k];
    }
}

// The device's launch sequence for one instance: assemble (init on the first iteration), f-sensitivities, update.
// `ws` (optional): the device workspace of the same call, six arrays of [rows][n] (Xw, Uw, Xdot, Fx, Fu, LM state).
struct TraceOut {
    float *Xw, *Uw, *Xd, *Fx, *Fu, *St;
};
template <int MODEL> void loop(const DevParams& P, const ac_trim_opts& o, const float* target, const float* Uhold, const float* Z0,
                               int iters, long n, float* X, float* U, float* Z, float* R, int* status, const TraceOut* ws = nullptr) {
    for (long u = 0; u < n; ++u) {
        TrimTarget t;
        float uh[4], z0[6], st[kTrimStateWords], x[13], uv[7], xd[13], fx[169], fu[91], zo[6], ro[6];
        load_unit(target, Uhold, n, u, t, uh);
        for (int j = 0; j < 6; ++j) z0[j] = Z0[j * n + u];
        const TrimCol c{st, 1};
        trim_init_unit(o, t, uh, z0, c);
        int s = AC_TRIM_MAXITER;
        for (int k = 0; k < iters; ++k) {
            if (trim_assemble_unit(o, t, uh, c, k == 0, x, uv)) unit_deriv_sens<MODEL>(P, x, uv, xd, fx, fu);
            trim_update_unit(o, t, TrimSens{xd, fx, fu, 1}, c, k == iters - 1, zo, ro, s);
        }
        if (ws) {
            for (int i = 0; i < 13; ++i) { ws->Xw[i * n + u] = x[i]; ws->Xd[i * n + u] = xd[i]; }
            for (int i = 0; i < 7; ++i) ws->Uw[i * n + u] = uv[i];
            for (int i = 0; i < 169; ++i) ws->Fx[i * n + u] = fx[i];
            for (int i = 0; i < 91; ++i) ws->Fu[i * n + u] = fu[i];
            for (int i = 0; i < kTrimStateWords; ++i) ws->St[i * n + u] = st[i];
        }
        trim_assemble(t, o.lateral, zo, uh, x, uv);
        for (int i = 0; i < 13; ++i) X[i * n + u] = x[i];
        for (int i = 0; i < 7; ++i) U[i * n + u] = uv[i];
        for (int j = 0; j < 6; ++j) { Z[j * n + u] = zo[j]; R[j * n + u] = ro[j]; }
        status[u] = s;
    }
}

}  // namespace

// z [6][n] -> X [13][n], U [7][n] (trim_assemble)
extern "C" int host_trim_assemble(int lateral, const float* target, const float* Uhold, const float* Z, long n, float* X, float* U) {
    for (long u = 0; u < n; ++u) {
        TrimTarget t;
        float uh[4], z[6], x[13], uv[7];
        load_unit(target, Uhold, n, u, t, uh);
        for (int j = 0; j < 6; ++j) z[j] = Z[j * n + u];
        trim_assemble(t, lateral, z, uh, x, uv);
        for (int i = 0; i < 13; ++i) X[i * n + u] = x[i];
        for (int i = 0; i < 7; ++i) U[i * n + u] = uv[i];
    }
    return 0;
}

#define AC_TRIM_MODELS(CALL) \
    if (P.p.model_kind == AC_MODEL_DEFAULT) { CALL(AC_MODEL_DEFAULT); return 0; } \
    if (P.p.model_kind == AC_MODEL_LINEAR) { CALL(AC_MODEL_LINEAR); return 0; } \
    if (P.p.model_kind == AC_MODEL_POLY) { CALL(AC_MODEL_POLY); return 0; } \
    return -2;

// r [6][n] and J_z [6][6][n] at z [6][n]
extern "C" int host_trim_jacobian(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                                  int lateral, const float* target, const float* Uhold, const float* Z, long n, float* R, float* J) {
    const DevParams P = make_params(p, linear_W, poly_coef, poly_intercept);
#define AC_CALL(M_) jac<M_>(P, lateral, target, Uhold, Z, n, R, J)
    AC_TRIM_MODELS(AC_CALL)
#undef AC_CALL
}

// the whole solve, as ac_trim_f32 runs it
extern "C" int host_trim(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                         const ac_trim_opts* o, const float* target, const float* Uhold, const float* Z0, int iters, long n, float* X,
                         float* U, float* Z, float* R, int* status) {
    const DevParams P = make_params(p, linear_W, poly_coef, poly_intercept);
#define AC_CALL(M_) loop<M_>(P, *o, target, Uhold, Z0, iters, n, X, U, Z, R, status)
    AC_TRIM_MODELS(AC_CALL)
#undef AC_CALL
}

// the whole solve, and what the device's workspace holds after it: Xw [13][n], Uw [7][n], Xdot [13][n], Fx [169][n], Fu [91][n],
// the LM state [kTrimStateWords][n]
extern "C" int host_trim_trace(const ac_params* p, const float* linear_W, const float* poly_coef, const float* poly_intercept,
                               const ac_trim_opts* o, const float* target, const float* Uhold, const float* Z0, int iters, long n, float* X,
                               float* U, float* Z, float* R, int* status, float* Xw, float* Uw, float* Xd, float* Fx, float* Fu,
                               float* St) {
    const DevParams P = make_params(p, linear_W, poly_coef, poly_intercept);
    const TraceOut ws{Xw, Uw, Xd, Fx, Fu, St};
#define AC_CALL(M_) loop<M_>(P, *o, target, Uhold, Z0, iters, n, X, U, Z, R, status, &ws)
    AC_TRIM_MODELS(AC_CALL)
#undef AC_CALL
}

// trim_residual_jacobian on GIVEN sensitivities Xdot [13][n], Fx [13][13][n], Fu [13][7][n] (the strided read of the device):
// r [6][n], J_z [6][6][n] at z [6][n]
extern "C" int host_trim_chain(int lateral, const float* target, const float* Z, const float* Xd, const float* Fx, const float* Fu,
                               long n, float* R, float* J) {
    for (long u = 0; u < n; ++u) {
        const TrimTarget t = trim_target(target, n, u);
        float z[6], r[6], jz[36];
        for (int j = 0; j < 6; ++j) z[j] = Z[j * n + u];
        trim_residual_jacobian(t, lateral, z, TrimSens{Xd + u, Fx + u, Fu + u, n}, r, jz);
        for (int i = 0; i < 6; ++i) R[i * n + u] = r[i];
        for (int k = 0; k < 36; ++k) J[k * n + u] = jz[k];
    }
    return 0;
}

// trim_step: z [6][n], r [6][n], J [6][6][n], lambda [n] -> the next candidate [6][n]
extern "C" int host_trim_step(const ac_trim_opts* o, const float* Z, const float* R, const float* J, const float* lam, long n,
                              float* Zn) {
    for (long u = 0; u < n; ++u) {
        float z[6], r[6], jz[36], zn[6];
        for (int j = 0; j < 6; ++j) { z[j] = Z[j * n + u]; r[j] = R[j * n + u]; }
        for (int k = 0; k < 36; ++k) jz[k] = J[k * n + u];
        trim_step(*o, z, r, jz, lam[u], zn);
        for (int j = 0; j < 6; ++j) Zn[j * n + u] = zn[j];
    }
    return 0;
}

// trim_final_status of a still-active instance
extern "C" int host_trim_final_status(const ac_trim_opts* o, const float* Z, const float* R, const float* J, long n, int* status) {
    for (long u = 0; u < n; ++u) {
        float z[6], r[6], jz[36];
        for (int j = 0; j < 6; ++j) { z[j] = Z[j * n + u]; r[j] = R[j * n + u]; }
        for (int k = 0; k < 36; ++k) jz[k] = J[k * n + u];
        status[u] = trim_final_status(*o, z, r, jz);
    }
    return 0;
}
