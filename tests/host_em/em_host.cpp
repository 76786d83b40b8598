// em_host.cpp — the per-lane code of the EM statistics for the EKF's noise variances (aircraft_amd/csrc/ac_em.hpp) compiled for
// the HOST (g++, -DAC_HOST_CHECK -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32
// arithmetic of the Cholesky, the triangular solves and the per-node terms against float64 without a GPU.  The 16 lanes of an
// instance's group run one after the other, phase by phase (GroupHost, ac_group.hpp), on the same code the device runs; the chunks and
// the reduction are the device's too.  AC_EM_HEADER names the header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_EM_HEADER
#define AC_EM_HEADER "../../aircraft_amd/csrc/ac_em.hpp"
#endif
#include AC_EM_HEADER

#include <vector>

using namespace ac;

extern "C" {

int host_em_chunk() { return kEmChunk; }

// the statistics of every instance; Qn, Rn may be NULL
int host_em_stats(const float* mag, float floor_rel, float eps, const float* Xpred, const float* Ppred, const float* Xs,
                  const float* Ps, const float* Z, const int* used, const float* Qd, const float* Rd, long n, long T, float* Qsum,
                  float* Rsum, int* nq, int* nr, int* status, float* Qn, float* Rn) {
    const long chunks = em_chunks(T);
    std::vector<double> part((size_t)chunks * kEmRows * n + 1);
    std::vector<int> cnt((size_t)chunks * kEmCounts * n + 1);
    const EmIo io{Xpred, Ppred, Xs, Ps, Z, used, Qd, Rd, part.data(), cnt.data(), Qsum, Rsum, nq, nr, status, Qn, Rn,
                  {mag[0], mag[1], mag[2]}, eps, floor_rel, n, T};
    for (long c = 0; c < chunks; ++c)
        for (long i = 0; i < n; ++i) {
            GroupHost<EmLane, kEkfLanes> grp{};
            EmShared s{};
            em_nodes_group(grp, s, io, i, c, true);
        }
    for (int row = 0; row < kEmRows; ++row)
        for (long i = 0; i < n; ++i) em_reduce_unit(io, row, i);
    return 0;
}

}  // extern "C"
