// RTS smoother over the EKF trace: k_ekf_smooth and its launcher (ac_rts.hpp).
#include "ac_rts.hpp"

namespace ac {

// (T is the same for every group of the workgroup: AC_GROUP_SLOT's rule holds)
__global__ __launch_bounds__(kRtsGroups* kEkfLanes) void k_ekf_smooth(const RtsIo io) {
    __shared__ RtsShared sh[kRtsGroups];
    AC_GROUP_SLOT(kEkfLanes, kRtsGroups, blockIdx.x, io.n);
    GroupDev<RtsLane> grp;
    grp.r = r;
    rts_sweep_group(grp, sh[g], io, i, store);
}

hipError_t rts_launch_smooth(const RtsIo& io, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((io.n + kRtsGroups - 1) / kRtsGroups);
    *lds = (int)(kRtsGroups * sizeof(RtsShared));
    hipLaunchKernelGGL(k_ekf_smooth, *grid, kRtsGroups * kEkfLanes, 0, st, io);
    return hipGetLastError();
}

}  // namespace ac
