// Extended Kalman filter over the step sensitivities: k_ekf_step, k_ekf_measure and their launchers (ac_ekf.hpp).
#include "ac_ekf.hpp"

namespace ac {

template <bool PREDICT>
__global__ __launch_bounds__(kEkfGroups* kEkfLanes) void k_ekf_step(const ac_ekf_opts o, float eps, const EkfIo io) {
    __shared__ EkfShared sh[kEkfGroups];
    AC_GROUP_SLOT(kEkfLanes, kEkfGroups, blockIdx.x, io.n);
    GroupDev<EkfLane> grp;
    grp.r = r;
    ekf_step_group<PREDICT>(grp, sh[g], o, eps, io, i, store);
}

__global__ __launch_bounds__(kEkfBlock) void k_ekf_measure(const ac_ekf_opts o, float eps, const float* __restrict__ X, long n,
                                                           float* __restrict__ Z) {
    const long i = (long)blockIdx.x * kEkfBlock + threadIdx.x;
    if (i >= n) return;
    ekf_measure_unit(o, eps, X, n, i, Z);
}

hipError_t ekf_launch_step(const ac_ekf_opts& o, float eps, const EkfIo& io, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((io.n + kEkfGroups - 1) / kEkfGroups);
    *lds = (int)(kEkfGroups * sizeof(EkfShared));
    if (o.predict) hipLaunchKernelGGL(k_ekf_step<true>, *grid, kEkfGroups * kEkfLanes, 0, st, o, eps, io);
    else hipLaunchKernelGGL(k_ekf_step<false>, *grid, kEkfGroups * kEkfLanes, 0, st, o, eps, io);
    return hipGetLastError();
}

hipError_t ekf_launch_measure(const ac_ekf_opts& o, float eps, const float* X, long n, float* Z, hipStream_t st, int* grid) {
    *grid = (int)((n + kEkfBlock - 1) / kEkfBlock);
    hipLaunchKernelGGL(k_ekf_measure, *grid, kEkfBlock, 0, st, o, eps, X, n, Z);
    return hipGetLastError();
}

}  // namespace ac
