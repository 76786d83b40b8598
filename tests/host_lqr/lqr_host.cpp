// lqr_host.cpp — the LQR's per-lane code (aircraft_amd/csrc/ac_lqr.hpp) compiled for the HOST (g++, -DAC_HOST_CHECK) behind a
// small C API, so that `pytest -m "not gpu"` measures the float32 arithmetic of the projection, the Riccati solve, the gain
// expansion and the chart against float64 without a GPU.  The 16 lanes of an instance's group run one after the other,
// phase by phase (GroupHost, ac_group.hpp), on the same code the device runs.  AC_LQR_HEADER names the header (the tests also build
// mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_LQR_HEADER
#define AC_LQR_HEADER "../../aircraft_amd/csrc/ac_lqr.hpp"
#endif
#include AC_LQR_HEADER

using namespace ac;

extern "C" {

int host_lqr_project(const float* X, const float* Xp, const float* A, const float* B, long n, float* Axi, float* Bxi) {
    const float U[7] = {0, 0, 0, 0, 0, 0, 0};
    for (long i = 0; i < n; ++i)
        lqr_project_unit(LqrCCol{X + i, n}, LqrCCol{U, 1}, LqrCCol{Xp + i, n}, LqrCCol{A + i, n}, LqrCCol{B + i, n},
                         LqrCol{Axi + i, n}, LqrCol{Bxi + i, n});
    return 0;
}

int host_lqr_dare(const ac_lqr_opts* o, const float* Axi, const float* Bxi, int iters, long n, float* P, float* K, float* resid,
                  int* status, int* used_iters) {
    for (long i = 0; i < n; ++i) {
        GroupHost<LqrLane, kLqrLanes> grp{};
        LqrShared s{};
        lqr_dare_group(grp, s, *o, iters, LqrCCol{Axi + i, n}, LqrCCol{Bxi + i, n}, LqrCol{P + i, n}, LqrCol{K + i, n}, resid + i,
                       status + i, used_iters + i, true);
    }
    return 0;
}

int host_lqr_gains(const float* Xnom, const float* K, long n, long H, float* Kx) {
    for (long k = 0; k < H; ++k)
        for (long i = 0; i < n; ++i)
            lqr_gains_unit(LqrCCol{Xnom + k * 13 * n + i, n}, LqrCCol{K + i, n}, LqrCol{Kx + k * 91 * n + i, n});
    return 0;
}

int host_steady_error(const float* X, const float* Xnom, long n, float* xi) {
    for (long i = 0; i < n; ++i) lqr_error_unit(LqrCCol{X + i, n}, LqrCCol{Xnom + i, n}, LqrCol{xi + i, n});
    return 0;
}

// the group elimination alone: W [12][12], RHS [12][24] row-major -> X = W^-1 RHS [12][24]
int host_lqr_gj(const float* W, const float* RHS, float* X, int* bad) {
    GroupHost<LqrLane, kLqrLanes> grp{};
    LqrShared s{};
    for (int r = 0; r < kLqrN; ++r) {
        for (int j = 0; j < 12; ++j) grp.L[r].w[j] = W[r * 12 + j];
        for (int j = 0; j < 24; ++j) grp.L[r].x[j] = RHS[r * 24 + j];
    }
    lqr_solve_rows<12, 24>(grp, s);
    *bad = 0;
    for (int r = 0; r < kLqrN; ++r) {
        for (int j = 0; j < 24; ++j) X[grp.L[r].piv * 24 + j] = (float)grp.L[r].x[j];
        if (grp.L[r].bad) *bad = 1;
    }
    return 0;
}

}  // extern "C"
