// modes_host.cpp — the eigenvalue chain and the flight-mode unit (aircraft_amd/csrc/ac_eig.hpp) compiled for the HOST (g++,
// -DAC_HOST_CHECK -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32 balancing,
// Hessenberg reduction and QR iteration against float64 without a GPU.  One instance after the other, on the code a lane
// of the device runs; the instance's memory is a plain array.  AC_EIG_HEADER names the header (the tests also build mutated
// copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_EIG_HEADER
#define AC_EIG_HEADER "../../aircraft_amd/csrc/ac_eig.hpp"
#endif
#include AC_EIG_HEADER

using namespace ac;

namespace {

struct EigHostMem {
    double b[kEigMaxM * (kEigMaxM + 2)];
    double& operator[](int w) { return b[w]; }
};

}  // namespace

extern "C" {

int host_eig(const float* M, int m, int max_iters, long n, float* wr, float* wi, int* status, int* iters) {
    for (long i = 0; i < n; ++i) {
        EigHostMem a{};
        eig_unit(a, EigCCol{M + i, n}, m, max_iters, EigCol{wr + i, n}, EigCol{wi + i, n}, status + i, iters + i);
    }
    return 0;
}

int host_modes_eig(const float* Axi, const float* Bxi, const float* K, unsigned coords, int m, int max_iters, float dt, long n,
                   float* wr, float* wi, float* sigma, float* omega, int* status, int* iters) {
    for (long i = 0; i < n; ++i) {
        EigHostMem a{};
        modes_unit(a, EigCCol{Axi + i, n}, EigCCol{Bxi + i, n}, EigCCol{K ? K + i : nullptr, n}, coords, m, max_iters, dt,
                   EigCol{wr + i, n}, EigCol{wi + i, n}, EigCol{sigma + i, n}, EigCol{omega + i, n}, status + i, iters + i);
    }
    return 0;
}

// the dynamic LDS request of k_eig / k_modes_eig for order m
int host_eig_lds_bytes(int m) { return eig_lds_bytes(m); }

}  // extern "C"
