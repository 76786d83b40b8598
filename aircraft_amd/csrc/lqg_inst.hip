// The loop closed through the estimator: k_lqg_sense, k_lqg_control, k_lqg_score and their launchers (ac_lqg.hpp).
#include "ac_lqg.hpp"

namespace ac {

// DISTURB false: Z, mask = sense(X); true: Xo = X (+) process noise.  A [rows][n] array of sigmas either way.
template <bool DISTURB>
__global__ __launch_bounds__(kLqgBlock) void k_lqg_sense(const LqgNoise o, float eps, int step, const int* __restrict__ step_dev,
                                                         const float* X, const float* __restrict__ sigma, long n, float* Xo_or_Z,
                                                         int* __restrict__ mask) {
    const long i = (long)blockIdx.x * kLqgBlock + threadIdx.x;
    if (i >= n) return;
    const int s = (int)((unsigned)step + (step_dev ? (unsigned)*step_dev : 0u));  // (wraps: no signed overflow)
    if (DISTURB) lqg_disturb_unit(o, s, X, sigma, n, i, Xo_or_Z);
    else lqg_sense_unit(o, eps, s, X, sigma, n, i, Xo_or_Z, mask);
}

__global__ __launch_bounds__(kLqgBlock) void k_lqg_control(const LqgLimits lim, const float* __restrict__ Fb,
                                                           const float* __restrict__ Xnom, const float* __restrict__ Unom,
                                                           const float* __restrict__ Kx, long n, float* __restrict__ U) {
    const long i = (long)blockIdx.x * kLqgBlock + threadIdx.x;
    if (i >= n) return;
    lqg_control_unit(lim, Fb, Xnom, Unom, Kx, n, i, U);
}

__global__ __launch_bounds__(kLqgBlock) void k_lqg_score(const float* __restrict__ X, const float* __restrict__ Xh,
                                                         const float* __restrict__ P, long n, float* __restrict__ E,
                                                         float* __restrict__ nees, int* __restrict__ status) {
    const long i = (long)blockIdx.x * kLqgBlock + threadIdx.x;
    if (i >= n) return;
    lqg_score_unit(X, Xh, P, n, i, E, nees, status);
}

static int lqg_grid(long n) { return (int)((n + kLqgBlock - 1) / kLqgBlock); }

hipError_t lqg_launch_sense(const LqgNoise& o, float eps, int step, const int* step_dev, const float* X, const float* sigma_r, long n,
                            float* Z, int* mask, hipStream_t st, int* grid) {
    *grid = lqg_grid(n);
    hipLaunchKernelGGL(k_lqg_sense<false>, *grid, kLqgBlock, 0, st, o, eps, step, step_dev, X, sigma_r, n, Z, mask);
    return hipGetLastError();
}

hipError_t lqg_launch_disturb(const LqgNoise& o, int step, const int* step_dev, const float* X, const float* sigma_q, long n, float* Xo,
                              hipStream_t st, int* grid) {
    *grid = lqg_grid(n);
    hipLaunchKernelGGL(k_lqg_sense<true>, *grid, kLqgBlock, 0, st, o, 0.f, step, step_dev, X, sigma_q, n, Xo, (int*)nullptr);
    return hipGetLastError();
}

hipError_t lqg_launch_control(const LqgLimits& lim, const float* Fb, const float* Xnom, const float* Unom, const float* Kx, long n,
                              float* U, hipStream_t st, int* grid) {
    *grid = lqg_grid(n);
    hipLaunchKernelGGL(k_lqg_control, *grid, kLqgBlock, 0, st, lim, Fb, Xnom, Unom, Kx, n, U);
    return hipGetLastError();
}

hipError_t lqg_launch_score(const float* X, const float* Xh, const float* P, long n, float* E, float* nees, int* status, hipStream_t st,
                            int* grid) {
    *grid = lqg_grid(n);
    hipLaunchKernelGGL(k_lqg_score, *grid, kLqgBlock, 0, st, X, Xh, P, n, E, nees, status);
    return hipGetLastError();
}

}  // namespace ac
