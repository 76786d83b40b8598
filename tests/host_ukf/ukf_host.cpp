// ukf_host.cpp — the UKF's per-lane code (aircraft_amd/csrc/ac_ukf.hpp) compiled for the HOST (g++, -DAC_HOST_CHECK
// -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32 arithmetic of the two kernels
// against float64 without a GPU.  The 16 lanes of an instance's group run one after the other, phase by phase (GroupHost, ac_group.hpp), on the same
// code the device runs.  AC_UKF_HEADER names the header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_UKF_HEADER
#define AC_UKF_HEADER "../../aircraft_amd/csrc/ac_ukf.hpp"
#endif
#include AC_UKF_HEADER

using namespace ac;

extern "C" {

// phase 1: the factor of P, the 25 n points (position rows relative to p^) and the replicated controls
int host_ukf_sigma(const ac_ukf_opts* o, const float* X, const float* P, const float* U, long n, float* Xw, float* Uw, float* Lw,
                   int* flag) {
    const UkfWeights w = ukf_weights(o->kappa);
    const UkfSigIo io{X, P, U, Xw, Uw, Lw, flag, n};
    for (long i = 0; i < n; ++i) {
        GroupHost<UkfSigLane, kEkfLanes> grp{};
        UkfSigShared s{};
        ukf_sigma_group(grp, s, w, io, i, true);
    }
    return 0;
}

// phase 2: everything after the forward step, from the images Fw of the points (ignored when o->predict == 0); the optional
// pointers may be NULL
int host_ukf_update(const ac_ukf_opts* o, float eps, const float* X, const float* P, const float* Fw, const float* Lw,
                    const int* flag, const float* Z, const int* mask, const float* Qd, const float* Rd, const float* ll_in, long n,
                    float* Xo, float* Po, float* nu, float* S, float* nis, float* ll, int* used, int* status, float* Xpred,
                    float* Ppred, float* Abar) {
    const UkfWeights w = ukf_weights(o->kappa);
    const UkfIo io{X, P, Fw, Lw, flag, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
    for (long i = 0; i < n; ++i) {
        GroupHost<UkfLane, kEkfLanes> grp{};
        UkfShared s{};
        if (o->predict) ukf_update_group<true>(grp, s, *o, w, eps, io, i, true);
        else ukf_update_group<false>(grp, s, *o, w, eps, io, i, true);
    }
    return 0;
}

}  // extern "C"
