// LQR about steady-flight trims: k_lqr_project, k_lqr_dare, k_lqr_gains, k_steady_error and their launchers (ac_lqr.hpp).
#include "ac_lqr.hpp"

namespace ac {
namespace {

int lane_grid(long n) { return (int)((n + kLqrBlock - 1) / kLqrBlock); }

}  // namespace

__global__ __launch_bounds__(kLqrBlock) void k_lqr_project(const float* __restrict__ X, const float* __restrict__ U,
                                                           const float* __restrict__ Xp, const float* __restrict__ A,
                                                           const float* __restrict__ B, long n, float* __restrict__ Axi,
                                                           float* __restrict__ Bxi) {
    const long i = (long)blockIdx.x * kLqrBlock + threadIdx.x;
    if (i >= n) return;
    lqr_project_unit(LqrCCol{X + i, n}, LqrCCol{U + i, n}, LqrCCol{Xp + i, n}, LqrCCol{A + i, n}, LqrCCol{B + i, n},
                     LqrCol{Axi + i, n}, LqrCol{Bxi + i, n});
}

// (a workgroup is one wave: the group's barrier orders its LDS traffic)
__global__ __launch_bounds__(kLqrGroups* kLqrLanes) void k_lqr_dare(const ac_lqr_opts o, int iters, const float* __restrict__ Axi,
                                                                     const float* __restrict__ Bxi, long n, float* __restrict__ P,
                                                                     float* __restrict__ K, float* __restrict__ resid,
                                                                     int* __restrict__ status, int* __restrict__ used_iters) {
    __shared__ LqrShared sh[kLqrGroups];
    AC_GROUP_SLOT(kLqrLanes, kLqrGroups, blockIdx.x, n);
    GroupDev<LqrLane> grp;
    grp.r = r;
    lqr_dare_group(grp, sh[g], o, iters, LqrCCol{Axi + i, n}, LqrCCol{Bxi + i, n}, LqrCol{P + i, n}, LqrCol{K + i, n}, resid + i,
                   status + i, used_iters + i, store);
}

__global__ __launch_bounds__(kLqrBlock) void k_lqr_gains(const float* __restrict__ Xnom, const float* __restrict__ K, long n, long H,
                                                         float* __restrict__ Kx) {
    const long i = (long)blockIdx.x * kLqrBlock + threadIdx.x;
    if (i >= n) return;
    for (long k = blockIdx.y; k < H; k += gridDim.y)
        lqr_gains_unit(LqrCCol{Xnom + k * 13 * n + i, n}, LqrCCol{K + i, n}, LqrCol{Kx + k * 91 * n + i, n});
}

__global__ __launch_bounds__(kLqrBlock) void k_steady_error(const float* __restrict__ X, const float* __restrict__ Xnom, long n,
                                                            float* __restrict__ xi) {
    const long i = (long)blockIdx.x * kLqrBlock + threadIdx.x;
    if (i >= n) return;
    lqr_error_unit(LqrCCol{X + i, n}, LqrCCol{Xnom + i, n}, LqrCol{xi + i, n});
}

hipError_t lqr_launch_project(const float* X, const float* U, const float* Xp, const float* A, const float* B, long n, float* Axi,
                              float* Bxi, hipStream_t st, int* grid) {
    *grid = lane_grid(n);
    hipLaunchKernelGGL(k_lqr_project, *grid, kLqrBlock, 0, st, X, U, Xp, A, B, n, Axi, Bxi);
    return hipGetLastError();
}

hipError_t lqr_launch_dare(const ac_lqr_opts& o, int iters, const float* Axi, const float* Bxi, long n, float* P, float* K,
                           float* resid, int* status, int* used_iters, hipStream_t st, int* grid, int* lds) {
    *grid = (int)((n + kLqrGroups - 1) / kLqrGroups);
    *lds = (int)(kLqrGroups * sizeof(LqrShared));
    hipLaunchKernelGGL(k_lqr_dare, *grid, kLqrGroups * kLqrLanes, 0, st, o, iters, Axi, Bxi, n, P, K, resid, status, used_iters);
    return hipGetLastError();
}

hipError_t lqr_launch_gains(const float* Xnom, const float* K, long n, long H, float* Kx, hipStream_t st, int* grid) {
    *grid = lane_grid(n);
    const dim3 g((unsigned)*grid, (unsigned)(H < 65535 ? H : 65535));
    hipLaunchKernelGGL(k_lqr_gains, g, kLqrBlock, 0, st, Xnom, K, n, H, Kx);
    return hipGetLastError();
}

hipError_t lqr_launch_error(const float* X, const float* Xnom, long n, float* xi, hipStream_t st, int* grid) {
    *grid = lane_grid(n);
    hipLaunchKernelGGL(k_steady_error, *grid, kLqrBlock, 0, st, X, Xnom, n, xi);
    return hipGetLastError();
}

}  // namespace ac
