// ac_wgrad.hpp — gradients of step and rollout losses with respect to the WEIGHTS of the MLP surrogate.
//
// For L = lambda . F(x, u, dt; theta) the RK4 reverse sweep (rk4_vjp, ac_adjoint.hpp) visits every stage once and hands the
// coefficient provider the cotangent Cbar[6] of that stage's coefficients.  With C = y os + mean that is a cotangent
// ybar = Cbar os on the raw network output at the stage's normalised input z, so
//   theta_bar = sum over units and stages of (dy/dtheta at z)' ybar :
// an ordinary MLP backward pass over 4 n samples (z[5], ybar[6]), reduced over the samples.  Three kernels:
//   k_nn_stage_jac<WT, MFMA>   walks the primal RK4 stages of 16 units per wave and stores y[6] and J[6][5] = dy/dz of every
//                              stage (the tangent-mode engine of the sensitivity kernels: value + five tangent slabs) —
//                              the first-order sibling of k_nn_stage_tensors: 36 floats per stage instead of 126
//   k_wgrad_seeds              one lane per unit: rk4_vjp<float> with a provider over that table which RECORDS, per stage,
//                              z and ybar:  Z [4][5][n], Ybar [4][6][n]
//   k_mlp_wgrad<WT, MFMA>      the weight gradient of the folded net over those samples on fp32 MFMA, one partial per
//                              persistent workgroup; k_wgrad_reduce adds the partials in a fixed order (no atomics: the same
//                              inputs give the same bits)
// One RK4 sub-step only: ac_step_wgrad_* refuse physical_integration_substeps > 1 (AC_ERR_UNSUPPORTED).
#pragma once
#include "ac_wgrad_plan.hpp"  // the host side: WgradPlan and build_wgrad_image, what ac_set_mlp prepares

#if defined(__HIPCC__) && !defined(AC_HOST_CHECK)
#include <utility>

#include "ac_hess_nn.hpp"
#include "ac_vjp.hpp"

namespace ac {

constexpr int kJacRows = 36;                 // y[6], J[6][5]
constexpr int kJacFloats = 4 * kJacRows;     // per unit

// ---- first-order stage table -----------------------------------------------------------------------------------------------
// out: [n / blk][4 stages][36][blk] (UnitAddr).  The engine takes the plan of the sensitivity kernels (engine_plan).
template <int WT, bool USE_MFMA>
__global__ __launch_bounds__(kBlock, 1) void k_nn_stage_jac(const DevParams P, const MlpPlan plan, const float* __restrict__ blob,
                                                            const float* __restrict__ X, const float* __restrict__ U, float dt,
                                                            const float* __restrict__ dt_per_unit, long n, long blk,
                                                            float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    MlpEngine<6, WT, USE_MFMA> eng(plan, blob, smem);
    eng.load_weights();
    const WaveUnit w(n, blk);
    float x0[13], u[7], xs[13];
    load_rows<13>(X, w.ua, x0);
    load_rows<7>(U, w.ua, u);
    const float h = dt_per_unit ? dt_per_unit[w.unit] : dt;
#pragma unroll
    for (int i = 0; i < 13; ++i) xs[i] = x0[i];
#pragma nounroll
    for (int s = 0; s < 4; ++s) {
        AeroPre<float> a;
        aero_pre(P, xs, a);
        const float in[5] = {a.qbar, a.alpha, a.beta, u[0], u[1]};
        float z[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) z[j] = (in[j] - P.mlp_in_mean[j]) / P.mlp_in_std[j];
        GivenY prov;
        float J[6][5];
        eng.forward(z, prov.y, J);
        if (w.live && w.g == 0) {  // (the four lane groups of a unit hold the same results)
            float* o = out + w.ua.off(kJacFloats) + (long)s * kJacRows * blk;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                o[(long)k * blk] = prov.y[k];
#pragma unroll
                for (int j = 0; j < 5; ++j) o[(long)(6 + k * 5 + j) * blk] = J[k][j];
            }
        }
        if (s < 3) {  // next primal stage point
            float k1[13];
            state_derivative<float>(P, prov, xs, u, k1);
            const float hs = h * ((s == 2) ? 1.0f : 0.5f);
#pragma unroll
            for (int i = 0; i < 13; ++i) xs[i] = fmaf(hs, k1[i], x0[i]);
        }
    }
    eng.drain();
}

// ---- recording reverse sweep -------------------------------------------------------------------------------------------------
// The MLP through the first-order stage table, for rk4_vjp<float> (the first-order use of AdjTensorCoeffsT's pattern); its
// adjoint records the stage's normalised input z and the cotangent ybar = Cbar os of the raw network output (the stall
// factors are already in Cbar: f_vjp applies them before it calls the provider).
struct StageJacCoeffs {
    static constexpr int kModel = AC_MODEL_NN;
    const float* __restrict__ base;
    const float* tp;
    long blk;
    int stage;
    float* zrec;   // this unit's column of Z [4][5][n]
    float* yrec;   // ... of Ybar [4][6][n]
    long n;
    AC_DI StageJacCoeffs(const float* table, const UnitAddr& ua, float* Z, float* Ybar, long unit, long n_)
        : base(table + ua.off(kJacFloats)), tp(base), blk(ua.blk), stage(0), zrec(Z + unit), yrec(Ybar + unit), n(n_) {}
    AC_DI void set_stage(int s) { stage = s; tp = base + (long)s * kJacRows * blk; }
    AC_DI float row(int r) const { return tp[(long)r * blk]; }
    AC_DI void operator()(const DevParams& P, const AeroPre<float>&, const float*, const float u[7], float C[6]) const {
#pragma unroll
        for (int k = 0; k < 6; ++k) C[k] = fmaf(row(k), P.mlp_out_std[k], P.mlp_out_mean[k]);
        C[5] += (-0.1f * 6.0f * kDeg) * u[2];
    }
    AC_DI void vjp(const DevParams& P, const AeroPre<float>& a, const float*, const float* u, const float Cb[6], AeroBar<float>& ab,
                   float wb[3], float ub[7]) const {
        (void)wb;
        float yb[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            yb[k] = Cb[k] * P.mlp_out_std[k];
            yrec[(long)(stage * 6 + k) * n] = yb[k];
        }
        const float in[5] = {a.qbar, a.alpha, a.beta, u[0], u[1]};
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            zrec[(long)(stage * 5 + j) * n] = (in[j] - P.mlp_in_mean[j]) / P.mlp_in_std[j];
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 6; ++k) s = fmaf(row(6 + k * 5 + j), yb[k], s);
            const float ib = s / P.mlp_in_std[j];
            if (j == 0) ab.qbar += ib; else if (j == 1) ab.alpha += ib; else if (j == 2) ab.beta += ib; else ub[j - 3] += ib;
        }
        ub[2] += (-0.1f * 6.0f * kDeg) * Cb[5];
    }
};

// X, U, Lam: units addressed through UnitAddr(unit, blk) ([13|7|13][n] with blk = n; rollout-shaped buffers with blk = B);
// Z [4][5][n], Ybar [4][6][n] flat over the n units.
__global__ void k_wgrad_seeds(const DevParams P, const float* __restrict__ X, const float* __restrict__ U, float dt,
                              const float* __restrict__ dt_per_unit, const float* __restrict__ Lam,
                              const float* __restrict__ table, long n, long blk, float* __restrict__ Z, float* __restrict__ Ybar);
__global__ void k_wgrad_reduce(const float* __restrict__ partial, int parts, int floats, float* __restrict__ out);
#ifdef AC_WGRAD_INSTANTIATE
__global__ __launch_bounds__(kVjpBlock) void k_wgrad_seeds(const DevParams P, const float* __restrict__ X, const float* __restrict__ U,
                                                           float dt, const float* __restrict__ dt_per_unit,
                                                           const float* __restrict__ Lam, const float* __restrict__ table, long n,
                                                           long blk, float* __restrict__ Z, float* __restrict__ Ybar) {
    __shared__ float stage_lds[kVjpStageWords * kVjpBlock];
    const long i = (long)blockIdx.x * kVjpBlock + threadIdx.x;
    if (i >= n) return;  // (no barrier below: every lane owns its LDS column)
    const UnitAddr ua(i, blk);
    float x[13], u[7], lam[13], xo[13], gx[13], gu[7], gh;
    load_rows<13>(X, ua, x);
    load_rows<7>(U, ua, u);
    load_rows<13>(Lam, ua, lam);
    const float h = dt_per_unit ? dt_per_unit[i] : dt;
    StageJacCoeffs coeffs(table, ua, Z, Ybar, i, n);
    VjpColumn col{&stage_lds[threadIdx.x], kVjpBlock};
    rk4_vjp<float>(P, coeffs, x, u, h, lam, xo, gx, gu, gh, col, true);
}

// out[i] = partial[0][i] + partial[1][i] + ... in that order
__global__ __launch_bounds__(kBlock) void k_wgrad_reduce(const float* __restrict__ partial, int parts, int floats,
                                                         float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= floats) return;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += partial[(long)p * floats + i];
    out[i] = s;
}
#endif

// ---- the weight gradient -----------------------------------------------------------------------------------------------------
template <class F, int... Is> AC_DI void wg_static_for(F&& f, std::integer_sequence<int, Is...>) {
    (f(std::integral_constant<int, Is>{}), ...);
}

// Samples: Z [G][5][n], Ybar [G][6][n], sample m = (group m / n, unit m % n), N = G n of them.  A workgroup (four waves) takes
// tiles of 32 samples (two MFMA column tiles), persistent over tiles blockIdx.x, + gridDim.x, ...:
//   forward       h_l = tanh(W_l h_{l-1} + b_l) for every layer but the last (its output is not needed: no activation there),
//                 neurons as rows, samples as columns; the A operands are the packed fragments read from global memory (L2),
//                 the B operands activation rows in LDS; the 2 wt output tiles of a layer are split over the waves
//   backward data delta_{l-1} = (W_l' delta_l) (1 - h_{l-1}^2) the same way over the transposed fragments; delta_{L-1} = ybar
//   weights       dW_l += delta_l h_{l-1}': the contraction runs over the SAMPLES, so both operands are read from LDS across
//                 their rows (row stride 36 floats: conflict-free for both this and the forward reads — the 16 x 16
//                 transpositions cost nothing beyond the LDS round trip the activations make anyway); the NT x KT
//                 accumulator tiles of a layer are split over the four waves and stay in registers over all tiles
//   bias          db_l += sum over the samples of delta_l: thread r adds row r
// At the end every workgroup stores its accumulators as one partial gradient vector (logical sizes, WgradPlan::g_off).
template <int WT, bool USE_MFMA>
__global__ __launch_bounds__(kWgBlock, 1) void k_mlp_wgrad(const WgradPlan pl, const float* __restrict__ img,
                                                           const float* __restrict__ Z, const float* __restrict__ Ybar, long n,
                                                           long N, float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float act_lds[];
    constexpr int P = 16 * WT, LS = kWgRowStride, S = kWgSamples;
    static_assert(S == 32, "two MFMA column tiles per sample tile");
    constexpr int TH = WT * WT / 4;      // hidden-product accumulator tiles per wave
    constexpr int TE = (WT + 3) / 4;     // first / last layer accumulator tiles per wave
    constexpr int MAXHH = wgrad_max_hidden_products(WT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, g = lane >> 4;
    const int L = pl.n_layers;
    // rows: [z 16][ybar 16][h_0 .. h_{L-2}: P each][delta ping, pong: P each]
    auto hrow = [&](int l) { return l < 0 ? 0 : 32 + l * P; };                                  // h_l, h_{-1} = z
    auto drow = [&](int l) { return l == L - 1 ? 16 : 32 + (L - 1) * P + (l & 1) * P; };        // delta_l
    f32x4 accH[MAXHH][TH], accF[TE], accL[TE];
    float accB[AC_MAX_LAYERS];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < MAXHH; ++l)
#pragma unroll
        for (int t = 0; t < TH; ++t) accH[l][t] = zero4;
#pragma unroll
    for (int t = 0; t < TE; ++t) { accF[t] = zero4; accL[t] = zero4; }
#pragma unroll
    for (int l = 0; l < AC_MAX_LAYERS; ++l) accB[l] = 0.f;
    // the padding rows of z (5..15) and ybar (6..15) stay zero; the loader below writes rows 0..4 and 0..5 only
    for (int e = tid; e < 32 * LS; e += kWgBlock) act_lds[e] = 0.f;

    // one layer's product for the two sample tiles:  out[rt][sc] = A-fragments(frag, RT x KTl) . in, then `epi` per element
    // (widths <= 32 have two row tiles only: there the four waves take one (row tile, sample tile) pair each)
    auto product = [&](const float* frag, int RT, int KTl, int in_row, auto&& init, auto&& epi) __attribute__((always_inline)) {
        if constexpr (WT >= 4) {
            // a wave takes whole row tiles: one fragment load serves both sample tiles (two independent accumulators), and the
            // next k-tile's fragment is requested before the products of the current one
            for (int rt = wave; rt < RT; rt += 4) {
                f32x4 acc0, acc1;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc0[r] = acc1[r] = init(16 * rt + 4 * g + r);
                const f32x4* fp = reinterpret_cast<const f32x4*>(frag) + (long)rt * KTl * 64 + lane;
                f32x4 w = fp[0];
                for (int kt = 0; kt < KTl; ++kt) {
                    const f32x4 wn = fp[(kt + 1 < KTl ? kt + 1 : kt) * 64];
                    const float* in = act_lds + (in_row + 16 * kt + 4 * g) * LS + col;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        acc0 = mma_16x16x4<USE_MFMA>(w[r], in[r * LS], acc0);
                        acc1 = mma_16x16x4<USE_MFMA>(w[r], in[r * LS + 16], acc1);
                    }
                    w = wn;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    epi(16 * rt + 4 * g + r, col, acc0[r]);
                    epi(16 * rt + 4 * g + r, 16 + col, acc1[r]);
                }
            }
        } else {
            for (int j = wave; j < 2 * RT; j += 4) {
                const int rt = j >> 1, sc = j & 1;
                f32x4 acc;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = init(16 * rt + 4 * g + r);
                for (int kt = 0; kt < KTl; ++kt) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(frag + ((long)(rt * KTl + kt) * 64 + lane) * 4);
                    const float* in = act_lds + (in_row + 16 * kt + 4 * g) * LS + 16 * sc + col;
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc = mma_16x16x4<USE_MFMA>(w[r], in[r * LS], acc);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) epi(16 * rt + 4 * g + r, 16 * sc + col, acc[r]);
            }
        }
    };
    // dW tiles t = wave, wave + 4, ... of an RT x CT tile grid:  acc[i] += delta rows of tile row . h rows of tile column
    auto outer = [&](auto& acc, auto NTILES, int tiles, int CT, int d_row, int h_row) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < S / 4; ++ks) {
#pragma unroll
            for (int i = 0; i < NTILES(); ++i) {
                const int t = wave + 4 * i;
                if (t < tiles) {  // (wave-uniform)
                    const int rt = t / CT, ct = t % CT;
                    const float a = act_lds[(d_row + 16 * rt + col) * LS + 4 * ks + g];
                    const float b = act_lds[(h_row + 16 * ct + col) * LS + 4 * ks + g];
                    acc[i] = mma_16x16x4<USE_MFMA>(a, b, acc[i]);
                }
            }
        }
    };
    auto store_tiles = [&](const auto& acc, auto NTILES, int tiles, int CT, int l, float* dst) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NTILES(); ++i) {
            const int t = wave + 4 * i;
            if (t < tiles) {
                const int rt = t / CT, ct = t % CT, c = 16 * ct + col;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * rt + 4 * g + r;
                    if (row < pl.nout[l] && c < pl.nin[l]) dst[pl.g_off[l] + row * pl.nin[l] + c] = acc[i][r];
                }
            }
        }
    };
    using TEc = std::integral_constant<int, TE>;
    using THc = std::integral_constant<int, TH>;

    const long ntiles = (N + S - 1) / S;
#pragma nounroll
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads();  // every wave is done with the previous tile's rows (and, the first time, the zero fill is complete)
        for (int e = tid; e < 11 * S; e += kWgBlock) {
            const int row = e / S, s = e % S;
            const long m = tile * S + s;
            float v = 0.f;
            if (m < N) {
                const long grp = m / n, unit = m % n;
                v = row < 5 ? Z[(grp * 5 + row) * n + unit] : Ybar[(grp * 6 + (row - 5)) * n + unit];
            }
            act_lds[(row < 5 ? row : 16 + row - 5) * LS + s] = v;
        }
        __syncthreads();
        // forward: every layer but the last
#pragma nounroll
        for (int l = 0; l < L - 1; ++l) {
            const float* bias = img + pl.b_off[l];
            float* out = act_lds + hrow(l) * LS;
            product(img + pl.wf_off[l], WT, l == 0 ? 1 : WT, hrow(l - 1), [&](int row) { return bias[row]; },
                    [&](int row, int s, float v) { out[row * LS + s] = act_tanh(v); });
            __syncthreads();
        }
        // backward: layers L-1 .. 0 (unrolled: the accumulators of a layer are registers)
        wg_static_for([&](auto lc) __attribute__((always_inline)) {
            constexpr int l = AC_MAX_LAYERS - 1 - decltype(lc)::value;
            if (l < L) {
                const bool first = l == 0, last = l == L - 1;
                const int RT = last ? 1 : WT, CT = first ? 1 : WT;
                if (first) {  // (a single-layer net: its one tile lives here too)
                    outer(accF, TEc{}, RT * CT, CT, drow(l), hrow(l - 1));
                } else if (last) {
                    outer(accL, TEc{}, RT * CT, CT, drow(l), hrow(l - 1));
                } else if constexpr (l >= 1 && l <= MAXHH) {
                    outer(accH[l - 1], THc{}, RT * CT, CT, drow(l), hrow(l - 1));
                }
                if (tid < 16 * RT) {
                    const float* d = act_lds + (drow(l) + tid) * LS;
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < S; ++k) s += d[k];
                    accB[l] += s;
                }
                if (l >= 1) {
                    const float* hp = act_lds + hrow(l - 1) * LS;
                    float* out = act_lds + drow(l - 1) * LS;
                    product(img + pl.wt_off[l], WT, RT, drow(l), [](int) { return 0.f; },
                            [&](int row, int s, float v) { const float h = hp[row * LS + s]; out[row * LS + s] = v * fmaf(-h, h, 1.0f); });
                    __syncthreads();
                }
            }
        }, std::make_integer_sequence<int, AC_MAX_LAYERS>{});
    }
    // this workgroup's partial gradient
    float* dst = partial + (long)blockIdx.x * pl.grad_floats;
    wg_static_for([&](auto lc) __attribute__((always_inline)) {
        constexpr int l = decltype(lc)::value;
        if (l < L) {
            const bool first = l == 0, last = l == L - 1;
            const int RT = last ? 1 : WT, CT = first ? 1 : WT;
            if (first) store_tiles(accF, TEc{}, RT * CT, CT, l, dst);
            else if (last) store_tiles(accL, TEc{}, RT * CT, CT, l, dst);
            else if constexpr (l >= 1 && l <= MAXHH) store_tiles(accH[l - 1], THc{}, RT * CT, CT, l, dst);
            if (tid < pl.nout[l]) dst[pl.g_off[l] + pl.nout[l] * pl.nin[l] + tid] = accB[l];
        }
    }, std::make_integer_sequence<int, AC_MAX_LAYERS>{});
}

}  // namespace ac
#endif  // __HIPCC__
