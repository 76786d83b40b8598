// RTS smoother over the EKF trace: k_ekf_smooth and its launcher (ac_rts.hpp).
#include "ac_rts.hpp"

namespace ac {
namespace {

// One lane of a 16-lane group: a phase, then the workgroup's barrier (it orders the LDS traffic of the phase).
struct RtsGroupDev {
    RtsLane L;
    int r;
    template <class F>
    __device__ __forceinline__ void each(F f) {
        f(L, r);
        __syncthreads();
    }
};

}  // namespace

// A group past the end of the batch smooths the last instance again and stores nothing: every lane of the workgroup
// reaches every barrier (T is the same for all).
__global__ __launch_bounds__(kRtsGroups* kEkfLanes) void k_ekf_smooth(const RtsIo io) {
    __shared__ RtsShared sh[kRtsGroups];
    const int g = threadIdx.x / kEkfLanes;
    long i = (long)blockIdx.x * kRtsGroups + g;
    const bool store = i < io.n;
    if (!store) i = io.n - 1;
    RtsGroupDev grp;
    grp.r = threadIdx.x % kEkfLanes;
    rts_sweep_group(grp, sh[g], io, i, store);
}

hipError_t rts_launch_smooth(const RtsIo& io, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((io.n + kRtsGroups - 1) / kRtsGroups);
    *lds = (int)(kRtsGroups * sizeof(RtsShared));
    hipLaunchKernelGGL(k_ekf_smooth, *grid, kRtsGroups * kEkfLanes, 0, st, io);
    return hipGetLastError();
}

}  // namespace ac
