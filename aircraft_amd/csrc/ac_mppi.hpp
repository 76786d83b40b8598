// ac_mppi.hpp — sampling-based MPC (MPPI): the control-noise sampler and the softmin update (ac_mppi_sample_f32,
// ac_mppi_update_f32).
//
// Noise.  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85),
//     key     = (seed & 0xffffffff, seed >> 32)
//     counter = (k, g, t, 2 it + j)      k sample, g = instance_offset + b the GLOBAL instance, t node, it iteration, j in {0, 1}
// Each word pair (xa, xb) of a call gives two normals (Box-Muller):
//     u1 = ((xa >> 8) + 1) 2^-24 in (0, 1],  u2 = (xb >> 8) 2^-24,  r = sqrt(-2 ln u1),  na = r cos(2 pi u2),  nb = r sin(2 pi u2)
// Call j = 0 feeds control rows 0-3 ((x0, x1) -> rows 0, 1; (x2, x3) -> rows 2, 3), call j = 1 rows 4, 5, 6 (its fourth normal is
// dropped).  The draw of (seed, it, k, g, t, row) therefore does not depend on B, K, H or on how a batch is sharded.
//
// Kernels (mppi_inst.hip), candidate column o = k B + b as ac_rollout_policy_f32 writes it:
//   k_mppi_sample   Uc[t][r][o] = clip(Unom[t][r][b] + sigma[r] n), optional X0 -> X0c tiling; four columns per lane, one
//                   Philox call per four rows of a column, 16-byte stores along the instance axis
//   k_mppi_weights  per instance: Jmin over the finite costs, w_k = exp(-(J_k - Jmin) / lambda), eta, the normalised weights
//                   to the workspace, stats [4][B]
//   k_mppi_blend    Unew[t][r][b] = clip(sum_k w_k Uc[t][r][k B + b]): Uc is read exactly once
// Both update kernels lay a workgroup out as KL x BL lanes (BL along the instance axis, KL along the samples): B >= 256
// gives one lane per instance with k in a loop, B = 1 all 256 lanes over k, with an LDS tree over KL in a fixed order
// (no atomics: the same inputs give the same bits).
#pragma once
#include "ac_math.hpp"
#include "../../include/aircraft_hip.h"

#ifdef AC_HOST_CHECK
#define AC_HD inline
#else
#define AC_HD __host__ __device__ __forceinline__
#endif

namespace ac {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kMppiBlock = 256;      // lanes per workgroup of all three kernels
constexpr int kMppiCols = 4;         // candidate columns per lane of the sampler / instances per lane of the vector blend
constexpr float kMppiFltMax = 3.4028235e38f;

struct Philox4 {
    unsigned x[4];
};

AC_HD Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = (unsigned long long)kPhiloxM0 * c0;
        const unsigned long long p1 = (unsigned long long)kPhiloxM1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    Philox4 r;
    r.x[0] = c0; r.x[1] = c1; r.x[2] = c2; r.x[3] = c3;
    return r;
}

// two normals from one word pair
AC_HD void mppi_box_muller(unsigned xa, unsigned xb, float& na, float& nb) {
    const float u1 = (float)((xa >> 8) + 1u) * 5.9604644775390625e-8f;  // 2^-24: exact
    const float u2 = (float)(xb >> 8) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
#ifdef AC_HOST_CHECK
    s = sinf(6.283185307179586f * u2); c = cosf(6.283185307179586f * u2);
#else
    sincosf(6.283185307179586f * u2, &s, &c);
#endif
    na = r * c;
    nb = r * s;
}

// the four normals of call j of (k, g, t, it): rows 4 j .. 4 j + 3
AC_HD void mppi_normals4(unsigned seed_lo, unsigned seed_hi, unsigned k, unsigned g, unsigned t, unsigned it, unsigned j,
                         float n[4]) {
    const Philox4 p = philox4x32_10(k, g, t, 2u * it + j, seed_lo, seed_hi);
    mppi_box_muller(p.x[0], p.x[1], n[0], n[1]);
    mppi_box_muller(p.x[2], p.x[3], n[2], n[3]);
}

AC_HD float mppi_clip(float u, float lo, float hi) { return fminf(fmaxf(u, lo), hi); }
// one element of a candidate: clip(unom + sigma n)
AC_HD float mppi_sample_element(float unom, float sigma, float n, float lo, float hi) {
    return mppi_clip(fmaf(sigma, n, unom), lo, hi);
}
// The seven rows of one candidate column.  nominal: the column is the clipped nominal (keep_nominal, k = 0).  A call all
// of whose rows have sigma = 0 is skipped.
AC_HD void mppi_sample_column(const ac_mppi_opts& o, unsigned k, unsigned g, unsigned t, unsigned it, bool nominal,
                              const float unom[7], float out[7]) {
    float n[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) n[r] = 0.f;
    const unsigned lo = (unsigned)(o.seed & 0xffffffffull), hi = (unsigned)(o.seed >> 32);
    const bool call0 = o.sigma[0] != 0.f || o.sigma[1] != 0.f || o.sigma[2] != 0.f || o.sigma[3] != 0.f;
    const bool call1 = o.sigma[4] != 0.f || o.sigma[5] != 0.f || o.sigma[6] != 0.f;
    if (!nominal) {
        if (call0) mppi_normals4(lo, hi, k, g, t, it, 0u, n);
        if (call1) mppi_normals4(lo, hi, k, g, t, it, 1u, n + 4);
    }
#pragma unroll
    for (int r = 0; r < 7; ++r)
        out[r] = (nominal || o.sigma[r] == 0.f) ? mppi_clip(unom[r], o.u_min[r], o.u_max[r])
                                                : mppi_sample_element(unom[r], o.sigma[r], n[r], o.u_min[r], o.u_max[r]);
}

// a cost that may win: finite (false for NaN and +-inf)
AC_HD bool mppi_finite(float J) { return fabsf(J) <= kMppiFltMax; }
// unnormalised weight of one cost against the instance's cheapest finite one
AC_HD float mppi_weight(float J, float Jmin, float lambda) { return mppi_finite(J) ? expf(-(J - Jmin) / lambda) : 0.f; }
// (cost, index) order of the update: the lower cost wins, the lower index on ties
AC_HD bool mppi_better(float Ja, int ka, float Jb, int kb) { return Ja < Jb || (Ja == Jb && ka < kb); }

}  // namespace ac

#ifndef AC_HOST_CHECK
namespace ac {
// Launchers (defined in mppi_inst.hip, which holds the kernels).  Arguments are checked by the ABI unit; neither allocates nor
// synchronises.  `grid` receives the first launch dimension of the last kernel (ac_last_launch).
hipError_t mppi_launch_sample(const ac_mppi_opts& o, const unsigned* it_dev, const float* Unom, const float* X0, int K, long B,
                              long H, float* Uc, float* X0c, hipStream_t st, int* grid);
hipError_t mppi_launch_update(const ac_mppi_opts& o, unsigned* it_dev, const float* J, const float* Uc, const float* Unom, int K,
                              long B, long H, float* Unew, float* stats, float* w, hipStream_t st, int* grid);
}  // namespace ac
#endif
