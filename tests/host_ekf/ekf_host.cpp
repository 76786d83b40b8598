// ekf_host.cpp — the EKF's per-lane code (aircraft_amd/csrc/ac_ekf.hpp) compiled for the HOST (g++, -DAC_HOST_CHECK
// -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32 arithmetic of the time update,
// the fifteen scalar updates and the injection against float64 without a GPU.  The 16 lanes of an instance's group run one
// after the other, phase by phase (GroupHost, ac_group.hpp), on the same code the device runs.  AC_EKF_HEADER names the header (the
// tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_EKF_HEADER
#define AC_EKF_HEADER "../../aircraft_amd/csrc/ac_ekf.hpp"
#endif
#include AC_EKF_HEADER

using namespace ac;

extern "C" {

// one filter step of every instance; Xp, A: the step and its state Jacobian (ignored when o->predict == 0); the optional
// pointers may be NULL
int host_ekf_step(const ac_ekf_opts* o, float eps, const float* X, const float* P, const float* Xp, const float* A, const float* Z,
                  const int* mask, const float* Qd, const float* Rd, const float* ll_in, long n, float* Xo, float* Po, float* nu,
                  float* S, float* nis, float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar) {
    const EkfIo io{X, P, Xp, A, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
    for (long i = 0; i < n; ++i) {
        GroupHost<EkfLane, kEkfLanes> grp{};
        EkfShared s{};
        if (o->predict) ekf_step_group<true>(grp, s, *o, eps, io, i, true);
        else ekf_step_group<false>(grp, s, *o, eps, io, i, true);
    }
    return 0;
}

int host_ekf_measure(const ac_ekf_opts* o, float eps, const float* X, long n, float* Z) {
    for (long i = 0; i < n; ++i) ekf_measure_unit(*o, eps, X, n, i, Z);
    return 0;
}

}  // extern "C"
