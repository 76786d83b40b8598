// ac_vjp.hpp — first-order REVERSE mode: vector-Jacobian products of the step, the rollout and f, for autograd callers.
//
// A torch loss over the outputs of state_update / rollout hands back one cotangent per unit (13 floats) where the forward
// sensitivity kernels push 21 tangents.  The reverse sweep of ac_adjoint.hpp (rk4_vjp, f_vjp in plain floats) turns it into
//   Xbar = A' lambda [13],  Ubar = B' lambda [7],  dtbar = c . lambda
// for about three evaluations of f per RK4 step.  Two routes:
//   fused     default / linear / cubic-fit models: one lane per unit (step) or per instance (rollout), everything recomputed
//             from the primal inputs; nothing but the inputs and the results touches memory
//   composed  MLP surrogate and quadrotor (and, on request, the analytic models): the existing sensitivity kernels write
//             A, B, c into a caller-provided workspace and a contraction kernel applies lambda (k_vjp_contract), or runs the
//             reverse recurrence of a rollout (k_vjp_recur)
//
// Sub-steps (physical_integration_substeps = ns > 1): state_update_carry runs ns RK4 steps of h = dt / ns on a float64 carry,
// each from the fp32 rounding of the carry, and normalises the quaternion ONCE after the last one.  The reverse sweep re-runs
// that forward pass, keeps the ns sub-step inputs (this lane's column of an LDS array, 13 ns floats) and pulls lambda back
// through them in reverse order; the normalisation adjoint enters the last sub-step only (rk4_vjp's norm_adj).
//
// What is shared, and where: step_vjp_unit is the sweep of one unit; step_vjp_lane / rollout_vjp_lane (below, host-compilable)
// are what one lane does around it (load x, u, lambda; sweep; store; the rollout's recurrence).  k_step_vjp / k_rollout_vjp,
// the coefficient gradient (ac_cgrad.hpp) and the airframe gradient (ac_agrad.hpp) all call the lane bodies with their own
// coefficient provider, and so do the host twins under tests/host_{vjp,cgrad,agrad}.
#pragma once
#include "ac_adjoint.hpp"

namespace ac {

constexpr int kVjpBlock = 64;          // lanes per workgroup of the fused kernels (one wave: the LDS column is per lane)
constexpr int kVjpMaxSubsteps = 40;    // (30 + 13 * 40) * 4 B * 64 lanes = 137.5 KB of LDS, under the 160 KB of a gfx950 workgroup

// This lane's column of a float array, `stride` floats between words (LDS on the device: stride = lanes of the workgroup;
// a plain array in the host build: stride 1):
//   words  0 .. 29            rk4_vjp's three stage states (rows 3..12).  In registers (StageRegs) hipcc turns them into a
//                             scratch array across the rolled stage loop (112 B/lane); in LDS they cost 7.5 KB per 64 lanes
//   words 30 + 13 s .. +12    the input of sub-step s = 1 .. ns-1 (sub-step 0 starts from x itself)
constexpr int kVjpStageWords = 30;
// (a constexpr function: host code sizes the dynamic LDS with it)
constexpr int vjp_lane_words(int ns) { return kVjpStageWords + 13 * (ns > 1 ? ns : 1); }
struct VjpColumn {
    float* base;
    int stride;
    // rk4_vjp's stage store
    AC_DI void put(int s, const float* row3) const {
        float* p = base + (long)s * 10 * stride;
#pragma unroll
        for (int i = 0; i < 10; ++i) p[i * stride] = row3[i];
    }
    AC_DI void get(int s, float* row3) const {
        const float* p = base + (long)s * 10 * stride;
#pragma unroll
        for (int i = 0; i < 10; ++i) row3[i] = p[i * stride];
    }
    // the sub-step inputs
    AC_DI void put_sub(int s, const float x[13]) const {
        float* p = base + (long)(kVjpStageWords + 13 * s) * stride;
#pragma unroll
        for (int i = 0; i < 13; ++i) p[i * stride] = x[i];
    }
    AC_DI void get_sub(int s, float x[13]) const {
        const float* p = base + (long)(kVjpStageWords + 13 * s) * stride;
#pragma unroll
        for (int i = 0; i < 13; ++i) x[i] = p[i * stride];
    }
};

// One full state_update (all sub-steps, the final normalisation) pulled back:  gx = A' lam, gu = B' lam, gdt = c . lam.
// `coeffs`: the coefficient provider of the sweep; its vjp() is called once per RK4 stage of every sub-step, in reverse order
// (a recording provider, ac_cgrad.hpp, sees the samples of all 4 ns stages there).
template <class Coeffs>
AC_DI void step_vjp_unit(const DevParams& P, Coeffs& coeffs, const float x[13], const float u[7], float dt, const float lam[13],
                         const VjpColumn& col, float gx[13], float gu[7], float& gdt) {
    const int ns = P.p.substeps < 1 ? 1 : P.p.substeps;
    const float h = (ns == 1) ? dt : dt / (float)ns;
    // forward: the inputs of sub-steps 1 .. ns-1 exactly as state_update_carry forms them
    if (ns > 1) {
        double xa[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) xa[i] = (double)x[i];
#pragma nounroll
        for (int s = 1; s < ns; ++s) {
            float xf[13], dx[13];
#pragma unroll
            for (int i = 0; i < 13; ++i) xf[i] = (float)xa[i];
            rk4_increment(P, coeffs, xf, u, h, dx);
#pragma unroll
            for (int i = 0; i < 13; ++i) { xa[i] += (double)dx[i]; xf[i] = (float)xa[i]; }
            col.put_sub(s, xf);
        }
    }
    // reverse: lambda through sub-steps ns-1 .. 0 (one instance of the sweep for every sub-step count)
#pragma unroll
    for (int i = 0; i < 13; ++i) gx[i] = lam[i];
#pragma unroll
    for (int i = 0; i < 7; ++i) gu[i] = 0.f;
    float gh = 0.f;
#pragma nounroll
    for (int s = ns - 1; s >= 0; --s) {
        float xs[13], xo[13], l[13], gxs[13], gus[7], ghs;
        if (s == 0) {
#pragma unroll
            for (int i = 0; i < 13; ++i) xs[i] = x[i];
        } else {
            col.get_sub(s, xs);
        }
#pragma unroll
        for (int i = 0; i < 13; ++i) l[i] = gx[i];
        VjpColumn stages = col;
        rk4_vjp<float>(P, coeffs, xs, u, h, l, xo, gxs, gus, ghs, stages, s == ns - 1);
#pragma unroll
        for (int i = 0; i < 13; ++i) gx[i] = gxs[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) gu[i] += gus[i];
        gh += ghs;
    }
    gdt = (ns == 1) ? gh : gh * (1.0f / (float)ns);  // h = dt / ns
}
// ... with the plain provider of an analytic model
template <int MODEL>
AC_DI void step_vjp_unit(const DevParams& P, const float x[13], const float u[7], float dt, const float lam[13],
                         const VjpColumn& col, float gx[13], float gu[7], float& gdt) {
    AdjAnalyticCoeffs<MODEL> coeffs;
    step_vjp_unit(P, coeffs, x, u, dt, lam, col, gx, gu, gdt);
}

// ---- lane bodies: what one lane of the fused kernels does, in plain pointers and an index ----------------------------------
// (no threadIdx: the kernels below, ac_cgrad.hpp and ac_agrad.hpp pass their lane's unit and LDS column, the host twins under
// tests/ pass n-strided arrays and a stride-1 column, so `pytest -m "not gpu"` runs this very code)
// Every output pointer is nullable: an output that is not asked for is not written; OUT_ALL: the caller guarantees Xbar / X0bar
// and Ubar (the plain VJP kernels: no null tests inside the horizon loop).  P by value: with a reference hipcc takes
// k_step_vjp from 239 to 256 VGPRs (linear) and to 256 + 5 AGPRs (default), 2 -> 1 waves per SIMD, for the same work.
//
// Step, unit i of X, U, Lam [13|7|13][n] -> Xbar [13][n], Ubar [7][n], dtbar [n]
template <bool OUT_ALL = false, class Coeffs>
AC_DI void step_vjp_lane(const DevParams P, Coeffs& coeffs, const VjpColumn& col, const float* __restrict__ X,
                         const float* __restrict__ U, float dt, const float* __restrict__ dt_per_unit,
                         const float* __restrict__ Lam, long n, long i, float* __restrict__ Xbar, float* __restrict__ Ubar,
                         float* __restrict__ dtbar) {
    float x[13], u[7], lam[13], gx[13], gu[7], gdt;
    load_rows<13>(X, n, i, x);
    load_rows<7>(U, n, i, u);
    load_rows<13>(Lam, n, i, lam);
    const float h = dt_per_unit ? dt_per_unit[i] : dt;
    step_vjp_unit(P, coeffs, x, u, h, lam, col, gx, gu, gdt);
    if (OUT_ALL || Xbar) store_rows<13>(Xbar, n, i, gx);
    if (OUT_ALL || Ubar) store_rows<7>(Ubar, n, i, gu);
    if (dtbar) dtbar[i] = gdt;
}

// Rollout, instance i, lambda in registers across the horizon:
//   lambda_H = G_H;  lambda_k = G_k + A_k' lambda_{k+1},  Ubar_k = B_k' lambda_{k+1},  dtbar = sum_k c_k . lambda_{k+1}
//   Xtraj [H+1][13][B] (the forward trajectory, ac_rollout_f32's layout), U [H][7][B], G [H+1][13][B] (dLoss/dX[k])
//   -> X0bar [13][B], Ubar [H][7][B], dtbar [B]
template <bool OUT_ALL = false, class Coeffs>
AC_DI void rollout_vjp_lane(const DevParams P, Coeffs& coeffs, const VjpColumn& col, const float* __restrict__ Xtraj,
                            const float* __restrict__ U, float dt, long B, long H, const float* __restrict__ G, long i,
                            float* __restrict__ X0bar, float* __restrict__ Ubar, float* __restrict__ dtbar) {
    float lam[13];
    load_rows<13>(G + H * 13 * B, B, i, lam);
    float gdt_sum = 0.f;
#pragma nounroll
    for (long k = H - 1; k >= 0; --k) {
        float x[13], u[7], g[13], gx[13], gu[7], gdt;
        load_rows<13>(Xtraj + k * 13 * B, B, i, x);
        load_rows<7>(U + k * 7 * B, B, i, u);
        load_rows<13>(G + k * 13 * B, B, i, g);
        step_vjp_unit(P, coeffs, x, u, dt, lam, col, gx, gu, gdt);
        if (OUT_ALL || Ubar) store_rows<7>(Ubar + k * 7 * B, B, i, gu);
        gdt_sum += gdt;
#pragma unroll
        for (int r = 0; r < 13; ++r) lam[r] = g[r] + gx[r];
    }
    if (OUT_ALL || X0bar) store_rows<13>(X0bar, B, i, lam);
    if (dtbar) dtbar[i] = gdt_sum;
}

// f itself pulled back:  gx = (df/dx)' w,  gu = (df/du)' w
template <int MODEL>
AC_DI void deriv_vjp_unit(const DevParams& P, const float x[13], const float u[7], const float w[13], float gx[13], float gu[7]) {
    AdjAnalyticCoeffs<MODEL> coeffs;
    float xd[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) gx[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 7; ++i) gu[i] = 0.f;
    f_vjp<float>(P, coeffs, x, u, w, xd, gx, gu);
}

}  // namespace ac

#ifndef AC_HOST_CHECK
#include "ac_kernels_analytic.hpp"

namespace ac {

// ---- fused, analytic models --------------------------------------------------------------------------------------------------
// Step: X, U, Lam [13|7|13][n] -> Xbar [13][n], Ubar [7][n], dtbar [n] (nullable).  Dynamic LDS: vjp_lane_words(ns) floats
// per lane.
template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_step_vjp(const DevParams P, const float* __restrict__ X, const float* __restrict__ U,
                                                        float dt, const float* __restrict__ dt_per_unit, const float* __restrict__ Lam,
                                                        long n, float* __restrict__ Xbar, float* __restrict__ Ubar,
                                                        float* __restrict__ dtbar) {
    extern __shared__ float vjp_lds[];  // [vjp_lane_words(ns)][kVjpBlock]
    const long i = (long)blockIdx.x * kVjpBlock + threadIdx.x;
    if (i >= n) return;  // (no barrier below: every lane owns its LDS column)
    AdjAnalyticCoeffs<MODEL> coeffs;
    step_vjp_lane<true>(P, coeffs, VjpColumn{&vjp_lds[threadIdx.x], kVjpBlock}, X, U, dt, dt_per_unit, Lam, n, i, Xbar, Ubar, dtbar);
}

// Rollout: one lane per instance (rollout_vjp_lane's layouts); dtbar nullable.
template <int MODEL>
__global__ __launch_bounds__(kVjpBlock) void k_rollout_vjp(const DevParams P, const float* __restrict__ Xtraj,
                                                           const float* __restrict__ U, float dt, long B, long H,
                                                           const float* __restrict__ G, float* __restrict__ X0bar,
                                                           float* __restrict__ Ubar, float* __restrict__ dtbar) {
    extern __shared__ float vjp_lds[];  // [vjp_lane_words(ns)][kVjpBlock]
    const long i = (long)blockIdx.x * kVjpBlock + threadIdx.x;
    if (i >= B) return;
    AdjAnalyticCoeffs<MODEL> coeffs;
    rollout_vjp_lane<true>(P, coeffs, VjpColumn{&vjp_lds[threadIdx.x], kVjpBlock}, Xtraj, U, dt, B, H, G, i, X0bar, Ubar, dtbar);
}

// f: X, U, W [13|7|13][n] -> Xbar [13][n], Ubar [7][n]
template <int MODEL>
__global__ __launch_bounds__(kBlock) void k_deriv_vjp(const DevParams P, const float* __restrict__ X, const float* __restrict__ U,
                                                      const float* __restrict__ W, long n, float* __restrict__ Xbar,
                                                      float* __restrict__ Ubar) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x[13], u[7], w[13], gx[13], gu[7];
    load_rows<13>(X, n, i, x);
    load_rows<7>(U, n, i, u);
    load_rows<13>(W, n, i, w);
    deriv_vjp_unit<MODEL>(P, x, u, w, gx, gu);
    store_rows<13>(Xbar, n, i, gx);
    store_rows<7>(Ubar, n, i, gu);
}

// ---- composed: Jacobians from the sensitivity kernels, then lambda applied --------------------------------------------------
// (defined in an_inst_vjp.hip only, below; declared for the other units)
__global__ void k_vjp_contract(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ c,
                               const float* __restrict__ Lam, long n, float* __restrict__ Xbar, float* __restrict__ Ubar,
                               float* __restrict__ dtbar);
__global__ void k_vjp_recur(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ c,
                            const float* __restrict__ G, long B, long H, float* __restrict__ X0bar, float* __restrict__ Ubar,
                            float* __restrict__ dtbar, float* __restrict__ LamTraj);
#ifdef AC_VJP_INSTANTIATE
// gx += A' lam, gu += B' lam, gdt += c . lam for unit i of A [13][13][n], Bm [13][7][n], c [13][n] (C_NULLABLE: may be NULL)
template <bool C_NULLABLE>
AC_DI void jac_transpose_apply(const float* __restrict__ A, const float* __restrict__ Bm, const float* __restrict__ c, long n,
                               long i, const float lam[13], float gx[13], float gu[7], float& gdt) {
#pragma unroll 1
    for (int r = 0; r < 13; ++r) {
#pragma unroll
        for (int j = 0; j < 13; ++j) gx[j] = fmaf(A[(long)(r * 13 + j) * n + i], lam[r], gx[j]);
#pragma unroll
        for (int j = 0; j < 7; ++j) gu[j] = fmaf(Bm[(long)(r * 7 + j) * n + i], lam[r], gu[j]);
        if (!C_NULLABLE || c) gdt = fmaf(c[(long)r * n + i], lam[r], gdt);
    }
}

// One unit per lane:  Xbar = A' lam, Ubar = B' lam, dtbar = c . lam  (c, dtbar nullable).  A [13][13][n], Bm [13][7][n],
// c [13][n] (ac_step_sens_f32's layout; Fx / Fu of ac_state_derivative_sens_f32 with c = NULL).
__global__ __launch_bounds__(kBlock) void k_vjp_contract(const float* __restrict__ A, const float* __restrict__ Bm,
                                                         const float* __restrict__ c, const float* __restrict__ Lam, long n,
                                                         float* __restrict__ Xbar, float* __restrict__ Ubar,
                                                         float* __restrict__ dtbar) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float lam[13];
    load_rows<13>(Lam, n, i, lam);
    float gx[13] = {}, gu[7] = {}, gdt = 0.f;
    jac_transpose_apply<true>(A, Bm, c, n, i, lam, gx, gu, gdt);
    store_rows<13>(Xbar, n, i, gx);
    store_rows<7>(Ubar, n, i, gu);
    if (dtbar) dtbar[i] = gdt;
}

// Reverse recurrence of a rollout over per-node Jacobians (ac_shoot_sens_f32's layout: A [H][13][13][B], Bm [H][13][7][B],
// c [H][13][B]), one instance per lane, with an arbitrary external cotangent G [H+1][13][B]:
//   lambda_H = G_H;  lambda_k = G_k + A_k' lambda_{k+1},  Ubar_k = B_k' lambda_{k+1},  dtbar += c_k . lambda_{k+1}
// LamTraj (nullable) [H][13][B]: node k receives lambda_{k+1}.
__global__ __launch_bounds__(kBlock) void k_vjp_recur(const float* __restrict__ A, const float* __restrict__ Bm,
                                                      const float* __restrict__ c, const float* __restrict__ G, long B, long H,
                                                      float* __restrict__ X0bar, float* __restrict__ Ubar,
                                                      float* __restrict__ dtbar, float* __restrict__ LamTraj) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    float lam[13];
    load_rows<13>(G + H * 13 * B, B, i, lam);
    float gdt = 0.f;
    for (long k = H - 1; k >= 0; --k) {
        // (the weight gradient's units are (X_k, U_k, lambda_{k+1}), ac_wgrad.hpp)
        if (LamTraj) store_rows<13>(LamTraj + k * 13 * B, B, i, lam);
        float gx[13], gu[7] = {};
        load_rows<13>(G + k * 13 * B, B, i, gx);
        jac_transpose_apply<false>(A + k * 169 * B, Bm + k * 91 * B, c + k * 13 * B, B, i, lam, gx, gu, gdt);
        store_rows<7>(Ubar + k * 7 * B, B, i, gu);
#pragma unroll
        for (int j = 0; j < 13; ++j) lam[j] = gx[j];
    }
    store_rows<13>(X0bar, B, i, lam);
    if (dtbar) dtbar[i] = gdt;
}

#endif  // AC_VJP_INSTANTIATE

// The fused kernels are compiled in a translation unit of their own (an_inst_vjp.hip); every other unit only refers to them.
#define AC_VJP_STEP_ARGS const DevParams, const float*, const float*, float, const float*, const float*, long, float*, float*, float*
#define AC_VJP_ROLL_ARGS const DevParams, const float*, const float*, float, long, long, const float*, float*, float*, float*
#define AC_VJP_DERIV_ARGS const DevParams, const float*, const float*, const float*, long, float*, float*
#define AC_VJP_MODEL(EXT, M)                                          \
    EXT template __global__ void k_step_vjp<M>(AC_VJP_STEP_ARGS);     \
    EXT template __global__ void k_rollout_vjp<M>(AC_VJP_ROLL_ARGS);  \
    EXT template __global__ void k_deriv_vjp<M>(AC_VJP_DERIV_ARGS);
#ifdef AC_VJP_INSTANTIATE
AC_VJP_MODEL(, AC_MODEL_DEFAULT) AC_VJP_MODEL(, AC_MODEL_LINEAR) AC_VJP_MODEL(, AC_MODEL_POLY)
#else
AC_VJP_MODEL(extern, AC_MODEL_DEFAULT) AC_VJP_MODEL(extern, AC_MODEL_LINEAR) AC_VJP_MODEL(extern, AC_MODEL_POLY)
#endif
#undef AC_VJP_MODEL

}  // namespace ac
#endif  // AC_HOST_CHECK
