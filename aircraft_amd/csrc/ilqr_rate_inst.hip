// The exact control-rate Riccati pass and the quadratic rate cost: k_ilqr_backward_rate<NODE, NEWTON> (all four),
// k_ilqr_rate_model, k_ilqr_rate_cost and their launchers (see ac_ilqr_rate.hpp).
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

hipError_t ilqr_rate_launch_backward(const IlqrCost& C, const NodeCost& N, const float* X, const float* U, const float* A,
                                     const float* Bm, const float* Hz, const float* rate_g, const float* rate_h, long B, long H,
                                     float* K, float* Kp, float* kff, float* dV, hipStream_t st) {
    const int grid = (int)B;  // one wave per instance
#define AC_BACKWARD_RATE(NODE_, NEWTON_)                                                                                      \
    hipLaunchKernelGGL((k_ilqr_backward_rate<NODE_, NEWTON_>), grid, 64, 0, st, C, N, X, U, A, Bm, Hz, rate_g, rate_h, B, H, K, \
                       Kp, kff, dV)
    const bool node = N.q != nullptr;
    if (node && Hz) AC_BACKWARD_RATE(true, true);
    else if (node) AC_BACKWARD_RATE(true, false);
    else if (Hz) AC_BACKWARD_RATE(false, true);
    else AC_BACKWARD_RATE(false, false);
#undef AC_BACKWARD_RATE
    return hipGetLastError();
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
