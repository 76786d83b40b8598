// ieks_host.cpp — the iterated Kalman smoother's per-lane code (aircraft_amd/csrc/ac_ieks.hpp) compiled for the HOST (g++,
// -DAC_HOST_CHECK -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures the float32 arithmetic of the
// forward recursion, the cost, the candidates and the accept decision against float64 without a GPU.  The 16 lanes of an
// instance's group run one after the other, phase by phase (GroupHost, ac_group.hpp), on the same code the device runs.
// AC_IEKS_HEADER names the header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_IEKS_HEADER
#define AC_IEKS_HEADER "../../aircraft_amd/csrc/ac_ieks.hpp"
#endif
#include AC_IEKS_HEADER

#include <vector>

using namespace ac;

extern "C" {

// the forward recursion of every instance; F [T][13][n], A [T][13][13][n]: the steps and their state Jacobians on Xbar[0 .. T-1]
int host_ieks_pass(const ac_ekf_opts* o, float eps, const float* X0, const float* P0, const float* Xbar, const float* F, const float* A,
                   const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps, float* ll,
                   float* nu, float* S, float* nis, int* used, int* status, float* Xpred, float* Ppred, float* Abar) {
    const IeksIo io{X0, P0, Xbar, F, A, Z, Qd, Rd, mask, Xs, Ps, ll, nu, S, nis, used, status, Xpred, Ppred, Abar, n, T};
    for (long i = 0; i < n; ++i) {
        GroupHost<IeksLane, kEkfLanes> grp{};
        IeksShared s{};
        ieks_filter_group(grp, s, *o, eps, io, i, true);
    }
    return 0;
}

// J of reps n trajectories; Ft [T][13][reps n] = F(Xt[k], U[k], dt)
int host_ieks_cost(const ac_ekf_opts* o, float eps, const float* X0, const float* P0, const float* Xt, const float* Ft, const float* Z,
                   const int* mask, const float* Qd, const float* Rd, long n, long reps, long T, float* J, float* Jprior, float* Jproc,
                   float* Jmeas, int* status) {
    const long cols = n * reps, chunks = ieks_chunks(T);
    std::vector<double> part((size_t)chunks * 2 * cols + 1);
    std::vector<int> pst((size_t)chunks * cols + 1);
    const IeksCostIo io{X0, P0, Xt, Ft, Z, Qd, Rd, mask, part.data(), pst.data(), J, Jprior, Jproc, Jmeas, status,
                        {o->mag_ned[0], o->mag_ned[1], o->mag_ned[2]}, eps, n, reps, T};
    for (long c = 0; c < chunks; ++c)
        for (long col = 0; col < cols; ++col) ieks_cost_nodes_unit(io, col, c);
    for (long col = 0; col < cols; ++col) ieks_cost_reduce_unit(io, col);
    return 0;
}

int host_ieks_candidates(const float* Xbar, const float* Xs0, const float* Xs, const float* U, const float* ladder, int count, long n,
                         long T, float* Xc, float* Uc) {
    IeksLadder lad{};
    lad.count = count;
    for (int c = 0; c < count; ++c) lad.a[c] = ladder[c];
    const IeksCandIo io{Xbar, Xs0, Xs, U, Xc, Uc, lad, n, T};
    for (long k = 0; k <= T; ++k)
        for (int c = 0; c < count; ++c)
            for (long i = 0; i < n; ++i) ieks_candidate_unit(io, k, c, i);
    return 0;
}

int host_ieks_accept(const float* Jcur, const float* Jc, const int* stc, const float* Xc, const float* ladder, int count, long n, long T,
                     float* Xbar, float* alpha, float* Jout, int* status) {
    IeksLadder lad{};
    lad.count = count;
    for (int c = 0; c < count; ++c) lad.a[c] = ladder[c];
    const IeksAcceptIo io{Jcur, Jc, stc, Xc, Xbar, alpha, Jout, status, lad, n, T};
    for (long k = T; k >= 0; --k)  // (node 0 writes the status: last, as no unit reads what another writes)
        for (long i = 0; i < n; ++i) ieks_accept_unit(io, k, i);
    return 0;
}

}  // extern "C"
