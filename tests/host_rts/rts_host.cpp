// rts_host.cpp — the RTS smoother's per-lane code (aircraft_amd/csrc/ac_rts.hpp) compiled for the HOST (g++, -DAC_HOST_CHECK
// -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32 arithmetic of the Cholesky, the
// triangular solves, the chart and the covariance recursion against float64 without a GPU.  The 16 lanes of an instance's
// group run one after the other, phase by phase (GroupHost, ac_group.hpp), on the same code the device runs.  AC_RTS_HEADER names the
// header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_RTS_HEADER
#define AC_RTS_HEADER "../../aircraft_amd/csrc/ac_rts.hpp"
#endif
#include AC_RTS_HEADER

using namespace ac;

extern "C" {

// the backward sweep of every instance; X0, P0, Xs0, Ps0 all given or all NULL; Cg may be NULL
int host_rts_smooth(const float* X0, const float* P0, const float* Xf, const float* Pf, const float* Xpred, const float* Ppred,
                    const float* Abar, long n, long T, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Cg, int* status) {
    const RtsIo io{X0, P0, Xf, Pf, Xpred, Ppred, Abar, Xs, Ps, Xs0, Ps0, Cg, status, n, T};
    for (long i = 0; i < n; ++i) {
        GroupHost<RtsLane, kEkfLanes> grp{};
        RtsShared s{};
        rts_sweep_group(grp, s, io, i, true);
    }
    return 0;
}

}  // extern "C"
