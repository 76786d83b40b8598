// lqg_host.cpp — the per-lane code of the closed loop through the estimator (aircraft_amd/csrc/ac_lqg.hpp) compiled for the
// HOST (g++, -DAC_HOST_CHECK -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` checks the noise
// definition, the schedule, the control law and the score against their restatements without a GPU.  AC_LQG_HEADER names the
// header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_LQG_HEADER
#define AC_LQG_HEADER "../../aircraft_amd/csrc/ac_lqg.hpp"
#endif
#include AC_LQG_HEADER

using namespace ac;

extern "C" {

// out [4][m] = philox4x32_10 of the counters c [4][m] and keys k [2][m]
int host_lqg_philox(const unsigned* c, const unsigned* k, long m, unsigned* out) {
    for (long i = 0; i < m; ++i) {
        const Philox4 p = philox4x32_10(c[i], c[m + i], c[2 * m + i], c[3 * m + i], k[i], k[m + i]);
        for (int j = 0; j < 4; ++j) out[j * m + i] = p.x[j];
    }
    return 0;
}

// the bits of the reporting rows of instances 0 .. n-1 at the steps step .. step + T - 1: out [T][n]
int host_lqg_schedule(const ac_sense_opts* o, int step, long T, long n, int* out) {
    for (long t = 0; t < T; ++t)
        for (long i = 0; i < n; ++i) out[t * n + i] = lqg_report_mask(*o, (unsigned long long)(o->instance_offset + i), step + (int)t);
    return 0;
}

int host_lqg_sense(const ac_sense_opts* o, float eps, int step, const float* X, const float* sigma_r, long n, float* Z, int* mask) {
    for (long i = 0; i < n; ++i) lqg_sense_unit(*o, eps, step, X, sigma_r, n, i, Z, mask);
    return 0;
}

int host_lqg_disturb(const ac_sense_opts* o, int step, const float* X, const float* sigma_q, long n, float* Xo) {
    for (long i = 0; i < n; ++i) lqg_disturb_unit(*o, step, X, sigma_q, n, i, Xo);
    return 0;
}

int host_lqg_policy(const float* u_min, const float* u_max, const float* Fb, const float* Xnom, const float* Unom, const float* Kx,
                    long n, float* U) {
    LqgLimits lim;
    for (int r = 0; r < 7; ++r) {
        lim.u_min[r] = u_min[r];
        lim.u_max[r] = u_max[r];
    }
    for (long i = 0; i < n; ++i) lqg_control_unit(lim, Fb, Xnom, Unom, Kx, n, i, U);
    return 0;
}

int host_lqg_score(const float* X, const float* Xh, const float* P, long n, float* e, float* nees, int* status) {
    for (long i = 0; i < n; ++i) lqg_score_unit(X, Xh, P, n, i, e, nees, status);
    return 0;
}

}  // extern "C"
