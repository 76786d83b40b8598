// EM statistics for the EKF's noise variances: k_ekf_em_nodes, k_ekf_em_reduce and their launcher (ac_em.hpp).
#include "ac_em.hpp"

namespace ac {

// Workgroup b works on chunk b / gb of the instances (b % gb) * 16 .. + 15 (gb: workgroups per chunk), so that neighbouring
// workgroups read neighbouring columns of the same nodes (the chunk is the same for every group of the workgroup:
// AC_GROUP_SLOT's rule holds).
__global__ __launch_bounds__(kEmGroups* kEkfLanes) void k_ekf_em_nodes(const EmIo io, const long gb) {
    __shared__ EmShared sh[kEmGroups];
    AC_GROUP_SLOT(kEkfLanes, kEmGroups, (long)blockIdx.x % gb, io.n);
    const long c = (long)blockIdx.x / gb;
    GroupDev<EmLane> grp;
    grp.r = r;
    em_nodes_group(grp, sh[g], io, i, c, store);
}

__global__ __launch_bounds__(kEmBlock) void k_ekf_em_reduce(const EmIo io) {
    const long t = (long)blockIdx.x * kEmBlock + threadIdx.x;  // row-major over [27][n]: neighbouring lanes, neighbouring instances
    if (t >= (long)kEmRows * io.n) return;
    em_reduce_unit(io, (int)(t / io.n), t % io.n);
}

hipError_t em_launch(const EmIo& io, hipStream_t st, int* grid, int* lds) {
    const long gb = (io.n + kEmGroups - 1) / kEmGroups, chunks = em_chunks(io.T);
    *grid = (int)(gb * chunks);
    *lds = (int)(kEmGroups * sizeof(EmShared));
    if (chunks > 0) {
        hipLaunchKernelGGL(k_ekf_em_nodes, *grid, kEmGroups * kEkfLanes, 0, st, io, gb);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const long lanes = (long)kEmRows * io.n;
    hipLaunchKernelGGL(k_ekf_em_reduce, (int)((lanes + kEmBlock - 1) / kEmBlock), kEmBlock, 0, st, io);
    return hipGetLastError();
}

}  // namespace ac
