// Unscented Kalman filter beside the EKF bank: k_ukf_sigma, k_ukf_update and their launchers (ac_ukf.hpp).
#include "ac_ukf.hpp"

namespace ac {

__global__ __launch_bounds__(kUkfGroups* kEkfLanes) void k_ukf_sigma(const UkfWeights w, const UkfSigIo io) {
    __shared__ UkfSigShared sh[kUkfGroups];
    AC_GROUP_SLOT(kEkfLanes, kUkfGroups, blockIdx.x, io.n);
    GroupDev<UkfSigLane> grp;
    grp.r = r;
    ukf_sigma_group(grp, sh[g], w, io, i, store);
}

template <bool PREDICT>
__global__ __launch_bounds__(kUkfGroups* kEkfLanes) void k_ukf_update(const ac_ukf_opts o, const UkfWeights w, float eps,
                                                                     const UkfIo io) {
    __shared__ UkfShared sh[kUkfGroups];
    AC_GROUP_SLOT(kEkfLanes, kUkfGroups, blockIdx.x, io.n);
    GroupDev<UkfLane> grp;
    grp.r = r;
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
