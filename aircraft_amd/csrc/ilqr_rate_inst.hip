// The quadratic control-rate cost and its model for the exact rate pass: k_ilqr_rate_model, k_ilqr_rate_cost and their launchers
// (see ac_ilqr_rate.hpp; the k_ilqr_backward_rate kernels are in ilqr_backward_inst.hip).
#include "ac_ilqr_rate.hpp"

namespace ac {

__global__ __launch_bounds__(kBlock) void k_ilqr_rate_model(const RateWeights W, const float* __restrict__ U,
                                                            const float* __restrict__ u_prev, long B, long H,
                                                            float* __restrict__ rate_g, float* __restrict__ rate_h) {
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= H * B) return;
    const long k = t / B, b = t % B;
    const bool on = k > 0 || u_prev != nullptr;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const long o = (k * 7 + i) * B + b;
        float g = 0.f, h = 0.f;
        if (on) {
            const float up = k > 0 ? U[o - 7 * B] : u_prev[i * B + b];
            g = W.w[i] * (U[o] - up);
            h = W.w[i];
        }
        rate_g[o] = g;
        rate_h[o] = h;
    }
}

__global__ __launch_bounds__(kBlock) void k_ilqr_rate_cost(const RateWeights W, const float* __restrict__ U,
                                                           const float* __restrict__ u_prev, long Bn, long B, long H,
                                                           float* __restrict__ cost) {
    const long o = (long)blockIdx.x * kBlock + threadIdx.x;
    if (o >= B) return;
    const long bn = o % Bn;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        float up = 0.f;
        for (long k = 0; k < H; ++k) {
            const float u = U[(k * 7 + i) * B + o];
            if (k == 0) up = u_prev ? u_prev[i * Bn + bn] : u;
            const float d = u - up;
            acc = fmaf(0.5f * W.w[i] * d, d, acc);
            up = u;
        }
    }
    cost[o] += acc;
}

hipError_t ilqr_rate_launch_model(const RateWeights& W, const float* U, const float* u_prev, long B, long H, float* rate_g,
                                  float* rate_h, hipStream_t st, int* grid) {
    *grid = (int)((H * B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_ilqr_rate_model, *grid, kBlock, 0, st, W, U, u_prev, B, H, rate_g, rate_h);
    return hipGetLastError();
}

hipError_t ilqr_rate_launch_cost(const RateWeights& W, const float* U, const float* u_prev, long Bn, long B, long H, float* cost,
                                 hipStream_t st, int* grid) {
    *grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_ilqr_rate_cost, *grid, kBlock, 0, st, W, U, u_prev, Bn, B, H, cost);
    return hipGetLastError();
}

}  // namespace ac
