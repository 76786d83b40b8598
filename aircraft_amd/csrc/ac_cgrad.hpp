// ac_cgrad.hpp — gradients of step and rollout losses with respect to the COEFFICIENTS of the cubic-fit and the linear model
// (DESIGN.md §4.10).
//
// For L = lambda . F(x, u, dt; theta) the fused reverse sweep (step_vjp_unit, ac_vjp.hpp) visits every RK4 stage of every
// sub-step once and hands the coefficient provider the cotangent Cb[6] of that stage's raw coefficients (the stall factors
// already applied).  Both models are linear in their parameters, so
//   theta_bar = sum over units, sub-steps and stages of  Cb (x) features :
//   poly    theta = coef[6][34], intercept[6] (ac_set_poly's order, 210 floats).  phi(f) = the 34 monomials of sklearn's
//           PolynomialFeatures(3) over (alpha, beta, da, de) without the constant:
//             coef_bar[k][m] += Cb[k] phi_m(alpha, beta, da, de)     k = 0..3
//             coef_bar[4][m] += Cb[4] phi_m(alpha_e, beta, da, de),  coef_bar[5][m] += Cb[5] phi_m(alpha, beta_r, da, de)
//             intercept_bar[k] += Cb[k]
//             coef_bar[2][m] += (b/8) Cb[3] (alpha_r^j - alpha_l^j)  (m, j) = (0, 1), (4, 2), (14, 3): the wing-station term of C_l
//   linear  theta = W[6][6] (36 floats, the last column the bias):  W_bar[k][j] += Cb[k] in[j],  in = (qbar, alpha, beta, da, de, 1)
// A recording provider (RecCoeffs) derives from AdjAnalyticCoeffs<MODEL>: its vjp() runs the base adjoint, then adds the
// sample into a sink.  On the device the sink is this lane's column of an LDS array [P][64] (stride 1 across the lanes:
// conflict-free); after its last tile a workgroup adds the 64 columns of every row in a fixed order into one partial [P] in
// the caller's workspace, and k_wgrad_reduce adds the partials in workgroup order.  No floating-point atomics: the same
// inputs on the same grid give the same bits.
//
// The persistent sweeps (cgrad_step_sweep, cgrad_rollout_sweep) are templates over the accumulator count and the recording
// provider: the kernels here and those of the airframe gradient (ac_agrad.hpp) are one call each.  What a lane does per unit is
// step_vjp_lane / rollout_vjp_lane of ac_vjp.hpp, shared with the plain VJP kernels and the host twins.
#pragma once
#include "ac_vjp.hpp"

namespace ac {

template <int MODEL> struct CgradFloats {
    static constexpr int value = MODEL == AC_MODEL_POLY ? 6 * 34 + 6 : (MODEL == AC_MODEL_LINEAR ? 36 : 0);
};
// LDS words per lane: the accumulators, then the VjpColumn words (30 + 13 ns).  With the 210 accumulators of the cubic fits
// 240 + 13 ns <= 640 words (160 KB per 64 lanes): ns <= 30.  One limit for both models.
constexpr int kCgradMaxSubsteps = 30;
constexpr int cgrad_lane_words(int floats, int ns) { return floats + vjp_lane_words(ns); }

// This lane's column of accumulators, `stride` floats between entries (LDS: the lanes of the workgroup; host build: 1)
struct CgradColumn {
    float* base;
    int stride;
    AC_DI void add(int i, float v) const { base[(long)i * stride] += v; }
};

template <int MODEL, class Sink> struct RecCoeffs : AdjAnalyticCoeffs<MODEL> {
    static_assert(CgradFloats<MODEL>::value > 0, "coefficient gradients: the cubic-fit and the linear model");
    Sink sink;
    AC_DI explicit RecCoeffs(const Sink& s) : sink(s) {}
    // (hides the base's template: the sweep runs in plain floats)
    AC_DI void vjp(const DevParams& P, const AeroPre<float>& a, const float x[13], const float u[7], const float Cb[6],
                   AeroBar<float>& ab, float wb[3], float ub[7]) const {
        AdjAnalyticCoeffs<MODEL>::template vjp<float>(P, a, x, u, Cb, ab, wb, ub);
        if constexpr (MODEL == AC_MODEL_LINEAR) {
            const float in[5] = {a.qbar, a.alpha, a.beta, u[0], u[1]};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
#pragma unroll
                for (int j = 0; j < 5; ++j) sink.add(k * 6 + j, Cb[k] * in[j]);
                sink.add(k * 6 + 5, Cb[k]);
            }
        } else {
            // the effective angles exactly as poly_vjp forms them
            const float* w = &x[10];
            const float eps = P.p.epsilon, arm = P.p.rudder_moment_arm, b4 = P.p.b * 0.25f;
            const float ux = a.vr[0] + eps;
            const float ye = a.vr[2] + arm * w[1], yl = a.vr[2] - b4 * w[0], yr = a.vr[2] + b4 * w[0];
            const float alpha_e = m_atan2(ye, ux), alpha_l = m_atan2(yl, ux), alpha_r = m_atan2(yr, ux);
            const float vy = a.vr[1] - arm * w[2];
            const float nb = m_sqrt(a.vr[0] * a.vr[0] + vy * vy + a.vr[2] * a.vr[2] + eps);
            const float beta_r = m_asin(vy / nb);
            float m[34];
            {   // fits 0..3 at the main point; fit 2 also takes the wing stations of C_l (pure-alpha monomials 0, 4, 14)
                const float f[4] = {a.alpha, a.beta, u[0], u[1]};
                poly_monomials(f, m);
                const float wing = (b4 * 0.5f) * Cb[3];
                const float ar2 = alpha_r * alpha_r, al2 = alpha_l * alpha_l;
                const float d1 = alpha_r - alpha_l, d2 = ar2 - al2, d3 = ar2 * alpha_r - al2 * alpha_l;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
#pragma unroll
                    for (int q = 0; q < 34; ++q) {
                        float v = Cb[k] * m[q];
                        if (k == 2 && q == 0) v += wing * d1;
                        if (k == 2 && q == 4) v += wing * d2;
                        if (k == 2 && q == 14) v += wing * d3;
                        sink.add(k * 34 + q, v);
                    }
                }
            }
            {
                const float f[4] = {alpha_e, a.beta, u[0], u[1]};
                poly_monomials(f, m);
#pragma unroll
                for (int q = 0; q < 34; ++q) sink.add(4 * 34 + q, Cb[4] * m[q]);
            }
            {
                const float f[4] = {a.alpha, beta_r, u[0], u[1]};
                poly_monomials(f, m);
#pragma unroll
                for (int q = 0; q < 34; ++q) sink.add(5 * 34 + q, Cb[5] * m[q]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) sink.add(6 * 34 + k, Cb[k]);
        }
    }
};

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {

// The workgroup's partial: row r = the sum of its 64 columns, starting at column r mod 64 (the lanes of one read then hit 64
// different banks) and wrapping — an order fixed by the row alone.
template <int PF> AC_DI void cgrad_store_partial(const float* lds, float* __restrict__ out) {
    __syncthreads();
    const int l = threadIdx.x;
    for (int r = l; r < PF; r += kVjpBlock) {
        float s = 0.f;
#pragma unroll 8
        for (int c = 0; c < kVjpBlock; ++c) s += lds[r * kVjpBlock + ((c + l) & (kVjpBlock - 1))];
        out[r] = s;
    }
}

// The recording sweeps of one workgroup, persistent over tiles of 64 lanes (tile = blockIdx.x, + gridDim.x, ...): zero this
// lane's PF accumulators, run the lane body of ac_vjp.hpp with the recording provider Coeffs(CgradColumn) over every unit the
// lane owns, store the workgroup's partial [PF].  Dynamic LDS: [PF][kVjpBlock] accumulators, then
// [vjp_lane_words(ns)][kVjpBlock]: cgrad_lane_words(PF, ns) floats per lane.  Shared by the coefficient and the airframe
// gradient (ac_agrad.hpp); every per-unit output pointer is nullable.
//
// Step: X, U, Lam [13|7|13][n] -> partial [gridDim.x][PF], Xbar [13][n], Ubar [7][n], dtbar [n]
template <int PF, class Coeffs>
AC_DI void cgrad_step_sweep(const DevParams P, const float* __restrict__ X, const float* __restrict__ U, float dt,
                            const float* __restrict__ dt_per_unit, const float* __restrict__ Lam, long n,
                            float* __restrict__ Xbar, float* __restrict__ Ubar, float* __restrict__ dtbar,
                            float* __restrict__ partial) {
    extern __shared__ float cg_lds[];
    float* acc = &cg_lds[threadIdx.x];
    for (int r = 0; r < PF; ++r) acc[r * kVjpBlock] = 0.f;
    const VjpColumn col{&cg_lds[PF * kVjpBlock + threadIdx.x], kVjpBlock};
    Coeffs coeffs(CgradColumn{acc, kVjpBlock});
    const long ntiles = (n + kVjpBlock - 1) / kVjpBlock;
#pragma nounroll
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long i = tile * kVjpBlock + threadIdx.x;
        // (a mask, not a return: every lane takes part in the column sums below)
        if (i < n) step_vjp_lane(P, coeffs, col, X, U, dt, dt_per_unit, Lam, n, i, Xbar, Ubar, dtbar);
    }
    cgrad_store_partial<PF>(cg_lds, partial + (long)blockIdx.x * PF);
}

// Rollout: one lane per instance (rollout_vjp_lane's layouts and recurrence) -> partial [gridDim.x][PF], X0bar, Ubar, dtbar
template <int PF, class Coeffs>
AC_DI void cgrad_rollout_sweep(const DevParams P, const float* __restrict__ Xtraj, const float* __restrict__ U, float dt, long B,
                               long H, const float* __restrict__ G, float* __restrict__ X0bar, float* __restrict__ Ubar,
                               float* __restrict__ dtbar, float* __restrict__ partial) {
    extern __shared__ float cg_lds[];
    float* acc = &cg_lds[threadIdx.x];
    for (int r = 0; r < PF; ++r) acc[r * kVjpBlock] = 0.f;
    const VjpColumn col{&cg_lds[PF * kVjpBlock + threadIdx.x], kVjpBlock};
    Coeffs coeffs(CgradColumn{acc, kVjpBlock});
    const long ntiles = (B + kVjpBlock - 1) / kVjpBlock;
#pragma nounroll
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long i = tile * kVjpBlock + threadIdx.x;
        if (i < B) rollout_vjp_lane(P, coeffs, col, Xtraj, U, dt, B, H, G, i, X0bar, Ubar, dtbar);
    }
    cgrad_store_partial<PF>(cg_lds, partial + (long)blockIdx.x * PF);
}

template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_step_cgrad(const DevParams P, const float* __restrict__ X, const float* __restrict__ U,
                                                          float dt, const float* __restrict__ dt_per_unit,
                                                          const float* __restrict__ Lam, long n, float* __restrict__ Xbar,
                                                          float* __restrict__ Ubar, float* __restrict__ dtbar,
                                                          float* __restrict__ partial) {
    cgrad_step_sweep<CgradFloats<MODEL>::value, RecCoeffs<MODEL, CgradColumn>>(P, X, U, dt, dt_per_unit, Lam, n, Xbar, Ubar, dtbar,
                                                                               partial);
}
template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_rollout_cgrad(const DevParams P, const float* __restrict__ Xtraj,
                                                             const float* __restrict__ U, float dt, long B, long H,
                                                             const float* __restrict__ G, float* __restrict__ X0bar,
                                                             float* __restrict__ Ubar, float* __restrict__ dtbar,
                                                             float* __restrict__ partial) {
    cgrad_rollout_sweep<CgradFloats<MODEL>::value, RecCoeffs<MODEL, CgradColumn>>(P, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar,
                                                                                  partial);
}

// out[i] = partial[0][i] + partial[1][i] + ... in that order (defined with the weight gradient, ac_wgrad.hpp)
__global__ void k_wgrad_reduce(const float* __restrict__ partial, int parts, int floats, float* __restrict__ out);

// The kernels are compiled in a translation unit of their own (an_inst_cgrad.hip); every other unit only refers to them.
#define AC_CGRAD_STEP_ARGS \
    const DevParams, const float*, const float*, float, const float*, const float*, long, float*, float*, float*, float*
#define AC_CGRAD_ROLL_ARGS const DevParams, const float*, const float*, float, long, long, const float*, float*, float*, float*, float*
#define AC_CGRAD_MODEL(EXT, M)                                         \
    EXT template __global__ void k_step_cgrad<M>(AC_CGRAD_STEP_ARGS);  \
    EXT template __global__ void k_rollout_cgrad<M>(AC_CGRAD_ROLL_ARGS);
#ifdef AC_CGRAD_INSTANTIATE
AC_CGRAD_MODEL(, AC_MODEL_LINEAR) AC_CGRAD_MODEL(, AC_MODEL_POLY)
#else
AC_CGRAD_MODEL(extern, AC_MODEL_LINEAR) AC_CGRAD_MODEL(extern, AC_MODEL_POLY)
#endif
#undef AC_CGRAD_MODEL

}  // namespace ac
#endif  // AC_HOST_CHECK
