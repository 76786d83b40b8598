// EM statistics for the EKF's noise variances: k_ekf_em_nodes, k_ekf_em_reduce and their launcher (ac_em.hpp).
#include "ac_em.hpp"

namespace ac {
namespace {

// One lane of a 16-lane group: a phase, then the workgroup's barrier (it orders the LDS traffic of the phase).
struct EmGroupDev {
    EmLane L;
    int r;
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f(L, r);
        __syncthreads();
    }
};

}  // namespace

// Workgroup b works on chunk b / gb of the instances (b % gb) * 16 .. + 15 (gb: workgroups per chunk), so that neighbouring
// workgroups read neighbouring columns of the same nodes.  A group past the end of the batch works on the last instance again
// and stores nothing: every lane of the workgroup reaches every barrier (the chunk is the same for all).
__global__ __launch_bounds__(kEmGroups* kEkfLanes) void k_ekf_em_nodes(const EmIo io, const long gb) {
    __shared__ EmShared sh[kEmGroups];
    const int g = threadIdx.x / kEkfLanes;
    const long c = (long)blockIdx.x / gb;
    long i = ((long)blockIdx.x % gb) * kEmGroups + g;
    const bool store = i < io.n;
    if (!store) i = io.n - 1;
    EmGroupDev grp;
    grp.r = threadIdx.x % kEkfLanes;
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
