// Unscented Kalman filter beside the EKF bank: k_ukf_sigma, k_ukf_update and their launchers (ac_ukf.hpp).
#include "ac_ukf.hpp"

namespace ac {
namespace {

// One lane of a 16-lane group: a phase, then the workgroup's barrier (it orders the LDS traffic of the phase).
template <class Lane>
struct UkfGroupDev {
    Lane L;
    int r;
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f(L, r);
        __syncthreads();
    }
};

}  // namespace

// A group past the end of the batch works on the last instance again and stores nothing: every lane of the workgroup
// reaches every barrier.
__global__ __launch_bounds__(kUkfGroups* kEkfLanes) void k_ukf_sigma(const UkfWeights w, const UkfSigIo io) {
    __shared__ UkfSigShared sh[kUkfGroups];
    const int g = threadIdx.x / kEkfLanes;
    long i = (long)blockIdx.x * kUkfGroups + g;
    const bool store = i < io.n;
    if (!store) i = io.n - 1;
    UkfGroupDev<UkfSigLane> grp;
    grp.r = threadIdx.x % kEkfLanes;
    ukf_sigma_group(grp, sh[g], w, io, i, store);
}

template <bool PREDICT>
__global__ __launch_bounds__(kUkfGroups* kEkfLanes) void k_ukf_update(const ac_ukf_opts o, const UkfWeights w, float eps,
                                                                     const UkfIo io) {
    __shared__ UkfShared sh[kUkfGroups];
    const int g = threadIdx.x / kEkfLanes;
    long i = (long)blockIdx.x * kUkfGroups + g;
    const bool store = i < io.n;
    if (!store) i = io.n - 1;
    UkfGroupDev<UkfLane> grp;
    grp.r = threadIdx.x % kEkfLanes;
    ukf_update_group<PREDICT>(grp, sh[g], o, w, eps, io, i, store);
}

hipError_t ukf_launch_sigma(const UkfWeights& w, const UkfSigIo& io, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((io.n + kUkfGroups - 1) / kUkfGroups);
    *lds = (int)(kUkfGroups * sizeof(UkfSigShared));
    hipLaunchKernelGGL(k_ukf_sigma, *grid, kUkfGroups * kEkfLanes, 0, st, w, io);
    return hipGetLastError();
}

hipError_t ukf_launch_update(const ac_ukf_opts& o, const UkfWeights& w, float eps, const UkfIo& io, hipStream_t st, int* grid,
                             int* lds) {
    *grid = (int)((io.n + kUkfGroups - 1) / kUkfGroups);
    *lds = (int)(kUkfGroups * sizeof(UkfShared));
    if (o.predict) hipLaunchKernelGGL(k_ukf_update<true>, *grid, kUkfGroups * kEkfLanes, 0, st, o, w, eps, io);
    else hipLaunchKernelGGL(k_ukf_update<false>, *grid, kUkfGroups * kEkfLanes, 0, st, o, w, eps, io);
    return hipGetLastError();
}

}  // namespace ac
