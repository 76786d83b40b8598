// ac_f16_pack.hpp — host-side image of a hidden (width x width) layer for the two-plane f16 matrix-core path of the
// sensitivity engines (MlpEngine::layer_bf with HID == kHiddenF16), and the range gate that decides whether
// a net may take that path.  Plain C++: build_mlp_model (ac_mlp_model.hpp) packs and gates with it, and the CPU tests (tests/test_mlp_f16_planes.py)
// compile it with g++.
//
// Two-plane split: hi = f16(w) (round to nearest even), lo' = f16((w - hi) * S) with S = 2^11.  w - hi is exact in fp32 and
// fits 13 bits, so hi + lo' / S reproduces w to 2^-22 relative (at most two fp32 ulps); the scale keeps lo' at the magnitude
// of w instead of 2^-11 below it, i.e. out of f16's subnormal range wherever hi is out of it.  Subnormal f16 values are KEPT
// (gradual underflow, as IEEE conversion gives them): the device split assumes that the matrix core, v_cvt_pk_f16_f32 and
// v_fma_mix_f32 of gfx950 all keep them under a kernel's default MODE (tools/experiments/f16_subnormals.hip is the probe
// that reads it off the hardware; DESIGN.md §4.3 says what to change if it reports a flush), so host and device split alike.
//
// Image of one layer: bf16_pack_layer's geometry (ac_bf16_pack.hpp: halves, 1-KiB pieces, bf16_chunk_row) with two planes
// per (tile, chunk) instead of three — the A operand of v_mfma_f32_16x16x32_f16 has the bf16 form's layout.
//   front: [nt 0 .. WT/2-1][c][plane 0..1] fragments, then the fp32 bias piece (16 WT floats, padded to 1 KiB)
//   back:  [nt WT/2 .. WT-1][c][plane 0..1] fragments
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ac_bf16_pack.hpp"

namespace ac {

constexpr float kF16LoScale = 2048.0f;  // S = 2^11

// fp32 -> f16 bits, round to nearest even, gradual underflow, overflow to infinity (what v_cvt_f16_f32 gives)
inline uint16_t f16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);   // NaN
    if (a >= 0x47800000u) return (uint16_t)(sign | 0x7c00u);  // >= 2^16 (and infinity); 65520 .. 65536 round up below
    if (a < 0x33000000u) return sign;                         // < 2^-25: rounds to zero (2^-25 itself ties to even = 0)
    const int e = (int)(a >> 23) - 127;                       // unbiased exponent, -25 .. 15
    uint32_t m = (a & 0x7fffffu) | 0x800000u;                 // 24-bit significand
    const int shift = e >= -14 ? 13 : 13 + (-14 - e);         // bits dropped: 13 for normals, more for subnormals
    const uint32_t kept = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t r = kept + ((rem > half || (rem == half && (kept & 1u))) ? 1u : 0u);
    // normals: r carries the implicit bit (0x400 .. 0x800); a carry to 0x800 bumps the exponent by itself in the sum below
    const uint32_t bits = e >= -14 ? ((uint32_t)(e + 14) << 10) + r : r;  // (e + 15 - 1): the implicit bit adds the last 1
    return (uint16_t)(sign | (bits >= 0x7c00u ? 0x7c00u : bits));
}
inline float f16_to_f32(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    float v;
    if (e == 0) v = std::ldexp((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp((float)(m | 0x400), e - 25);
    return (h & 0x8000u) ? -v : v;
}
inline void f16_split2(float w, uint16_t p[2]) {
    p[0] = f16_rne(w);
    p[1] = f16_rne((w - f16_to_f32(p[0])) * kF16LoScale);
}
inline int f16_front_bytes(int wt) { return plane_front_bytes(wt, 2); }
inline int f16_back_bytes(int wt) { return plane_back_bytes(wt, 2); }
inline int f16_layer_bytes(int wt) { return plane_layer_bytes(wt, 2); }
// W: [nout][nin] row-major fp32, b: [nout]; nin, nout <= 16 wt (zero padded).  dst: f16_layer_bytes(wt) bytes.
inline void f16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) {
    pack_plane_layer<2>(W, b, nin, nout, wt, dst, f16_split2);
}

// ---- range gate -----------------------------------------------------------------------------------------------------
// The f16 route is taken only when the weights PROVE every MFMA operand of the hidden layers inside f16's range with a
// factor 2 to spare (limit 2^15 against the format's 2^16), and when the tangents are not uniformly tiny:
//   weights of the hidden layers: |w| < 2^15 (then |lo'| <= 2^-11 |w| S < 2^15 as well);
//   value activations: |h| <= 1 (tanh);
//   tangents entering hidden layer l: |T_1| <= max |W_0| (act' <= 1), |T_{l+1}| <= ||W_l||_inf |T_l|, each < 2^15, the
//   last hidden layer's output bound included (their scaled lo planes have the magnitude of the element, so the same
//   bound covers them);
//   the largest tangent entering every hidden layer, at the fixed sample of normalised inputs below, >= 2^-14: under it
//   an element's hi plane is subnormal and carries fewer than 11 bits, and a net whose tangents are ALL that small would
//   lose relative accuracy (one small element among large ones does not: the error is relative to the largest).
// W[l]: [widths[l + 1]][widths[l]] row-major, b[l]: [widths[l + 1]]; tanh on every layer but the last (ac_set_mlp's fold
// guarantees it); hidden layers are l = 1 .. n_layers - 2.  Returns 0 if the net passes, else a reason code:
enum F16Gate { F16_GATE_OK = 0, F16_GATE_WEIGHT = 1, F16_GATE_TANGENT_BOUND = 2, F16_GATE_TANGENT_TINY = 3, F16_GATE_NONFINITE = 4 };
constexpr double kF16GateLimit = 32768.0;             // 2^15
constexpr double kF16GateMinTangent = 1.0 / 16384.0;  // 2^-14
constexpr int kF16GateSamples = 32;

// normalised input j of gate sample i: a fixed low-discrepancy set in [-2, 2]^5 (additive recurrence on irrational steps)
inline double f16_gate_sample(int i, int j) {
    static const double step[5] = {0.8191725133961645, 0.6710436067037893, 0.5497004779019703, 0.4503017857385955, 0.3688759116332580};
    const double t = (i + 1) * step[j];
    return 4.0 * (t - std::floor(t)) - 2.0;
}

inline int f16_gate(int n_layers, const int* widths, const float* const* W, const float* const* b, double* worst = nullptr) {
    if (worst) *worst = 0.0;
    if (n_layers < 3) return F16_GATE_OK;  // no hidden layer: nothing runs on the matrix core's f16 form
    for (int l = 1; l < n_layers - 1; ++l)
        for (long i = 0; i < (long)widths[l] * widths[l + 1]; ++i) {
            const double a = std::fabs((double)W[l][i]);
            if (!(a == a) || std::isinf(a)) return F16_GATE_NONFINITE;
            if (a >= kF16GateLimit) { if (worst) *worst = a; return F16_GATE_WEIGHT; }
        }
    double tb = 0.0;  // bound of the tangents entering hidden layer 1
    for (long i = 0; i < (long)widths[0] * widths[1]; ++i) tb = std::fmax(tb, std::fabs((double)W[0][i]));
    for (int l = 1; l < n_layers - 1; ++l) {
        if (!(tb < kF16GateLimit)) { if (worst) *worst = tb; return F16_GATE_TANGENT_BOUND; }
        double norm = 0.0;
        for (int r = 0; r < widths[l + 1]; ++r) {
            double s = 0.0;
            for (int k = 0; k < widths[l]; ++k) s += std::fabs((double)W[l][(long)r * widths[l] + k]);
            norm = std::fmax(norm, s);
        }
        tb *= norm;  // the bound entering layer l + 1
    }
    // (the last one bounds what the last hidden layer hands to the vector ALUs in fp32: not an f16 operand, held to the same
    // limit as a margin — a net that can reach 2^15 there is within one layer's gain of overflowing its operands)
    if (!(tb < kF16GateLimit)) { if (worst) *worst = tb; return F16_GATE_TANGENT_BOUND; }
    // largest tangent entering every hidden layer over the sample, in float64
    int wmax = 0;
    for (int l = 0; l <= n_layers; ++l) wmax = widths[l] > wmax ? widths[l] : wmax;
    double* buf = new double[(size_t)wmax * 6 * 2];
    double tmax[32];
    for (int l = 0; l < 32; ++l) tmax[l] = 0.0;
    for (int smp = 0; smp < kF16GateSamples; ++smp) {
        double *cur = buf, *nxt = buf + (size_t)wmax * 6;  // [6][width]: value, five tangents
        for (int j = 0; j < 5; ++j) {
            cur[j] = f16_gate_sample(smp, j);
            for (int t = 0; t < 5; ++t) cur[(size_t)(1 + t) * wmax + j] = t == j ? 1.0 : 0.0;
        }
        for (int l = 0; l < n_layers - 1; ++l) {
            const int nin = widths[l], nout = widths[l + 1];
            if (l >= 1 && l < 32)
                for (int t = 0; t < 5; ++t)
                    for (int k = 0; k < nin; ++k) tmax[l] = std::fmax(tmax[l], std::fabs(cur[(size_t)(1 + t) * wmax + k]));
            for (int r = 0; r < nout; ++r) {
                double s[6] = {(double)b[l][r], 0, 0, 0, 0, 0};
                for (int k = 0; k < nin; ++k) {
                    const double w = (double)W[l][(long)r * nin + k];
                    for (int t = 0; t < 6; ++t) s[t] += w * cur[(size_t)t * wmax + k];
                }
                const double h = std::tanh(s[0]), sp = 1.0 - h * h;
                nxt[r] = h;
                for (int t = 1; t < 6; ++t) nxt[(size_t)t * wmax + r] = sp * s[t];
            }
            double* sw = cur; cur = nxt; nxt = sw;
        }
    }
    delete[] buf;
    for (int l = 1; l < n_layers - 1 && l < 32; ++l) {
        if (!(tmax[l] == tmax[l])) return F16_GATE_NONFINITE;
        if (tmax[l] < kF16GateMinTangent) { if (worst) *worst = tmax[l]; return F16_GATE_TANGENT_TINY; }
    }
    return F16_GATE_OK;
}

}  // namespace ac
