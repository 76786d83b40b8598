// ac_lqg.hpp — the loop closed through the estimator: simulated sensors, process noise, the control law on an estimate and
// the scoring of the estimate against the truth (ac_sense_f32, ac_disturb_f32, ac_policy_f32, ac_estimate_score_f32,
// ac_lqg_rollout_f32).
//
// Noise.  Philox4x32-10 and Box-Muller as ac_mppi.hpp defines them,
//     key     = (seed_lo, seed_hi)
//     counter = (g low word, g high word, step, purpose)        g = instance_offset + i the GLOBAL instance
//     purpose 0-3   the four normals of measurement rows 4 p .. 4 p + 3 ((x0, x1) -> rows 4 p, 4 p + 1; (x2, x3) -> 4 p + 2, 4 p + 3;
//                   the sixteenth is dropped)
//     purpose 4     word j: the uniform (x[j] >> 8) 2^-24 of sensor group j = 0 .. 3
//     purpose 5     word 0: the uniform of group 4
//     purpose 6-8   the twelve process-noise normals, rows 4 (p - 6) .. 4 (p - 6) + 3
// A draw therefore depends on (seed, step, g, row) alone: not on n, on T, on how a batch is sharded or on whether the step was
// reached through the single-step call or the rollout.
// Sensor groups (three rows each, ac_ekf.hpp's rows): 0 GPS position, 1 GPS velocity, 2 gyro, 3 air data, 4 magnetometer.
// Group j reports at `step` when (step - phase[j]) % period[j] == 0 (taken in 64-bit) and its uniform is not below dropout[j];
// a group that does not report has a cleared mask bit and NaN in its rows (the EKF's own "did not report" rule).  A reporting
// row is
//     z = fmaf(sigma_r, normal, h(x))         h: k_ekf_measure's values (ekf_measure_unit), bit for bit when sigma_r = 0
// Process noise:  x (+) (sigma_q . normals) through ekf_inject.
// Control law:    u_r = clip(Unom_r + sum_c Kx[r][c] (fb_c - Xnom_c)), one fmaf per c in the order c = 0 .. 12, on whatever state
//                 it is handed (ac_rollout_policy_f32's law with kff = 0).
// Score:          e = x (-) x^ (rts_minus), nees = e' P^-1 e by a plain Cholesky P = L L' and one forward solve L y = e.
//
// Kernels (lqg_inst.hip), all one lane per instance, 256 lanes per workgroup, no LDS, no atomics, every sum in a fixed order:
// an instance's bits depend neither on n nor on where it sits in the batch.
//   k_lqg_sense<DISTURB>   false: Z, mask from X; true: Xo = X (+) noise
//   k_lqg_control          U from (fb, Xnom, Unom, Kx)
//   k_lqg_score            the 78 entries of L live in registers (every index is a compile-time constant after unrolling): the
//                          [rows][n] operands are read lane-contiguous, only the lower triangle of P is fetched, and neither LDS
//                          nor a barrier is needed.
// The per-lane code is shared with the host build (tests/host_lqg, -DAC_HOST_CHECK).
#pragma once
#include "ac_mppi.hpp"
#include "ac_rts.hpp"

namespace ac {

constexpr int kLqgBlock = 256;   // lanes per workgroup of every kernel here
constexpr int kLqgGroups = 5;    // sensor groups
constexpr int kLqgTri = 78;      // entries of the lower triangle of a 12 x 12 matrix
constexpr int AC_LQG_NOT_PD = 1; // score status: a pivot of the Cholesky of P was <= 0 or not finite

// purposes (counter word 3)
constexpr unsigned kLqgMeasNormals = 0u, kLqgDropA = 4u, kLqgDropB = 5u, kLqgProcNormals = 6u;

using LqgNoise = ac_sense_opts;  // passed to the noise kernels by value

struct LqgLimits {
    float u_min[7], u_max[7];
};

AC_HD float lqg_nan() { return __builtin_nanf(""); }

// the four normals of (g, step, purpose)
AC_HD void lqg_normals4(const LqgNoise& o, unsigned long long g, unsigned step, unsigned purpose, float nrm[4]) {
    const Philox4 p = philox4x32_10((unsigned)(g & 0xffffffffull), (unsigned)(g >> 32), step, purpose, o.seed_lo, o.seed_hi);
    mppi_box_muller(p.x[0], p.x[1], nrm[0], nrm[1]);
    mppi_box_muller(p.x[2], p.x[3], nrm[2], nrm[3]);
}

AC_HD float lqg_uniform(unsigned x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }  // 2^-24: exact

// is group j due at `step`?  (64-bit: step - phase cannot overflow for any int step and phase)
AC_HD bool lqg_due(const LqgNoise& o, int j, int step) { return ((long long)step - o.phase[j]) % o.period[j] == 0; }

// bits 0-14 of the rows that report at (g, step)
AC_HD int lqg_report_mask(const LqgNoise& o, unsigned long long g, int step) {
    bool any_drop = false;
#pragma unroll
    for (int j = 0; j < kLqgGroups; ++j) any_drop = any_drop || o.dropout[j] > 0.f;
    float u[kLqgGroups];
#pragma unroll
    for (int j = 0; j < kLqgGroups; ++j) u[j] = 1.0f;
    if (any_drop) {  // (a uniform is never below a dropout of 0: the two calls are skipped, no bit changes)
        const unsigned glo = (unsigned)(g & 0xffffffffull), ghi = (unsigned)(g >> 32);
        const Philox4 a = philox4x32_10(glo, ghi, (unsigned)step, kLqgDropA, o.seed_lo, o.seed_hi);
        const Philox4 b = philox4x32_10(glo, ghi, (unsigned)step, kLqgDropB, o.seed_lo, o.seed_hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = lqg_uniform(a.x[j]);
        u[4] = lqg_uniform(b.x[0]);
    }
    int mask = 0;
#pragma unroll
    for (int j = 0; j < kLqgGroups; ++j)
        if (lqg_due(o, j, step) && !(u[j] < o.dropout[j])) mask |= 7 << (3 * j);
    return mask;
}

// k_lqg_sense<false>'s unit: Z [15][n], mask [n] of instance i at `step`
AC_DI void lqg_sense_unit(const LqgNoise& o, float eps, int step, const float* X, const float* sigma_r, long n, long i, float* Z,
                          int* mask) {
    AC_EKF_FP
    const unsigned long long g = (unsigned long long)(o.instance_offset + i);
    const int m = lqg_report_mask(o, g, step);
    ac_ekf_opts eo;
    eo.mag_ned[0] = o.mag_ned[0]; eo.mag_ned[1] = o.mag_ned[1]; eo.mag_ned[2] = o.mag_ned[2];
    eo.predict = 1;
    float x[13], hx[16];
#pragma unroll
    for (int k = 0; k < 13; ++k) x[k] = X[k * n + i];
    ekf_measure_unit(eo, eps, x, 1, 0, hx);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float nrm[4] = {0.f, 0.f, 0.f, 0.f};
        if ((m >> (4 * p)) & 0xf) lqg_normals4(o, g, (unsigned)step, kLqgMeasNormals + (unsigned)p, nrm);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 4 * p + q;
            if (r < kEkfZ) Z[r * n + i] = ((m >> r) & 1) ? fmaf(sigma_r[r * n + i], nrm[q], hx[r]) : lqg_nan();
        }
    }
    mask[i] = m;
}

// k_lqg_sense<true>'s unit: Xo = X (+) (sigma_q . normals) of instance i at `step` (Xo may be X)
AC_DI void lqg_disturb_unit(const LqgNoise& o, int step, const float* X, const float* sigma_q, long n, long i, float* Xo) {
    AC_EKF_FP
    const unsigned long long g = (unsigned long long)(o.instance_offset + i);
    float x[13], d[12], xo[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) x[k] = X[k * n + i];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        float nrm[4];
        lqg_normals4(o, g, (unsigned)step, kLqgProcNormals + (unsigned)p, nrm);
#pragma unroll
        for (int q = 0; q < 4; ++q) d[4 * p + q] = sigma_q[(4 * p + q) * n + i] * nrm[q];
    }
    ekf_inject(x, d, xo);
#pragma unroll
    for (int k = 0; k < 13; ++k) Xo[k * n + i] = xo[k];
}

// k_lqg_control's unit: U [7][n] of instance i from the fed-back state Fb [13][n]
AC_DI void lqg_control_unit(const LqgLimits& lim, const float* Fb, const float* Xnom, const float* Unom, const float* Kx, long n,
                            long i, float* U) {
    AC_EKF_FP
    float dx[13];
#pragma unroll
    for (int c = 0; c < 13; ++c) dx[c] = Fb[c * n + i] - Xnom[c * n + i];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        float acc = Unom[r * n + i];
#pragma unroll
        for (int c = 0; c < 13; ++c) acc = fmaf(Kx[(r * 13 + c) * n + i], dx[c], acc);
        U[r * n + i] = mppi_clip(acc, lim.u_min[r], lim.u_max[r]);
    }
}

// k_lqg_score's unit: e [12][n], nees [n], status [n] of instance i (each output may be NULL)
AC_DI void lqg_score_unit(const float* X, const float* Xh, const float* P, long n, long i, float* E, float* nees, int* status) {
    AC_EKF_FP
    float x[13], xh[13], e[12];
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        x[k] = X[k * n + i];
        xh[k] = Xh[k * n + i];
    }
    rts_minus(x, xh, e);
    if (E) {
#pragma unroll
        for (int k = 0; k < 12; ++k) E[k * n + i] = e[k];
    }
    // P = L L' row by row (l[r (r + 1) / 2 + c], c <= r), y = L^-1 e alongside
    float l[kLqgTri], y[12];
    bool bad = false;
    float acc2 = 0.f;
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        float ys = e[r];
#pragma unroll
        for (int c = 0; c <= r; ++c) {
            float t = P[(r * 12 + c) * n + i];
#pragma unroll
            for (int k = 0; k < c; ++k) t = fmaf(-l[r * (r + 1) / 2 + k], l[c * (c + 1) / 2 + k], t);
            if (c < r) {
                const float v = t / l[c * (c + 1) / 2 + c];
                l[r * (r + 1) / 2 + c] = v;
                ys = fmaf(-v, y[c], ys);
            } else {
                bad = bad || !(t > 0.f) || !(t <= kEkfFltMax);
                const float dg = sqrtf(t);
                l[r * (r + 1) / 2 + r] = dg;
                y[r] = ys / dg;
                acc2 = fmaf(y[r], y[r], acc2);
            }
        }
    }
    if (nees) nees[i] = bad ? lqg_nan() : acc2;
    if (status) status[i] = bad ? AC_LQG_NOT_PD : 0;
}

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in lqg_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; none allocates or
// synchronises.  `grid` receives the launch dimension (ac_last_launch).  step_dev (or NULL) is read by the kernel and added to
// `step`, so that a captured launch can draw fresh noise on every replay.
hipError_t lqg_launch_sense(const LqgNoise& o, float eps, int step, const int* step_dev, const float* X, const float* sigma_r, long n,
                            float* Z, int* mask, hipStream_t st, int* grid);
hipError_t lqg_launch_disturb(const LqgNoise& o, int step, const int* step_dev, const float* X, const float* sigma_q, long n, float* Xo,
                              hipStream_t st, int* grid);
hipError_t lqg_launch_control(const LqgLimits& lim, const float* Fb, const float* Xnom, const float* Unom, const float* Kx, long n,
                              float* U, hipStream_t st, int* grid);
hipError_t lqg_launch_score(const float* X, const float* Xh, const float* P, long n, float* E, float* nees, int* status, hipStream_t st,
                            int* grid);
}  // namespace ac
#endif
