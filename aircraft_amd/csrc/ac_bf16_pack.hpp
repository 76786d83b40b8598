// ac_bf16_pack.hpp — host-side image of a hidden (width x width) layer for the bf16 matrix-core path of the
// sensitivity engines (MlpEngine::layer_bf).  Plain C++: build_mlp_model (ac_mlp_model.hpp) packs with it, and the CPU test
// (tests/test_mlp_bf16_planes.py) compiles it with g++ to check the split and the packing.
//
// Three-plane split: w1 = bf16(w), w2 = bf16(w - w1), w3 = bf16(w - w1 - w2), each rounded to nearest even.  Every
// residual is exact in fp32 and the last one fits 8 bits, so w1 + w2 + w3 == w bit for bit: the network the kernel
// multiplies by IS the fp32 network.
//
// Image of one layer (WT tiles of 16 per side, KC = WT / 2 k-chunks of 32), in 1-KiB pieces:
//   front: [nt 0 .. WT/2-1][c][plane 0..2] fragments, then the fp32 bias piece (16 WT floats, padded to 1 KiB)
//   back:  [nt WT/2 .. WT-1][c][plane 0..2] fragments
// A fragment piece holds lane l = i + 16 g (i = l & 15, g = l >> 4) at byte 16 l: eight bf16, the A operand of
// v_mfma_f32_16x16x32_bf16 for output row 16 nt + i and chunk-local k = 8 g + q, q = 0..7.  The B operand of that k is
// built in registers from two fp32 D tiles of the previous layer without shuffles (rows 4 g + r of tiles 2c and 2c+1),
// so chunk-local k = 8 g + q is input row 32 c + 4 g + q (q < 4) or 32 c + 16 + 4 g + (q - 4) (q >= 4): bf16_chunk_row().
#pragma once
#include <cstdint>
#include <cstring>

namespace ac {

inline uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline void bf16_split3(float w, uint16_t p[3]) {
    p[0] = bf16_rne(w);
    float r = w - bf16_to_f32(p[0]);
    p[1] = bf16_rne(r);
    r = r - bf16_to_f32(p[1]);
    p[2] = bf16_rne(r);
}
// input row of chunk-local k index kk (0..31) of k-chunk c
inline int bf16_chunk_row(int c, int kk) {
    const int g = kk >> 3, q = kk & 7;
    return 32 * c + ((q & 4) ? 16 : 0) + 4 * g + (q & 3);
}
// Geometry and packing of a plane image, shared by the bf16 form (three planes) and the f16 form (two, ac_f16_pack.hpp).
inline int plane_front_bytes(int wt, int planes) { return (wt / 2) * (wt / 2) * planes * 1024 + 1024; }
inline int plane_back_bytes(int wt, int planes) { return (wt / 2) * (wt / 2) * planes * 1024; }
inline int plane_layer_bytes(int wt, int planes) { return plane_front_bytes(wt, planes) + plane_back_bytes(wt, planes); }

// W: [nout][nin] row-major fp32, b: [nout]; nin, nout <= 16 wt (zero padded).  dst: plane_layer_bytes(wt, PLANES) bytes.
// split(w, p) writes the PLANES 16-bit planes of one weight.
template <int PLANES, class Split>
inline void pack_plane_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst, Split split) {
    unsigned char* img = static_cast<unsigned char*>(dst);
    memset(img, 0, (size_t)plane_layer_bytes(wt, PLANES));
    const int half = wt / 2, kc = wt / 2;
    for (int nt = 0; nt < wt; ++nt) {
        const size_t base = nt < half ? 0 : (size_t)plane_front_bytes(wt, PLANES);
        for (int c = 0; c < kc; ++c)
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 8; ++q) {
                    const int row = 16 * nt + (lane & 15), k = bf16_chunk_row(c, 8 * (lane >> 4) + q);
                    const float w = (row < nout && k < nin) ? W[(size_t)row * nin + k] : 0.f;
                    uint16_t p[PLANES];
                    split(w, p);
                    for (int pl = 0; pl < PLANES; ++pl) {
                        const size_t piece = (size_t)((nt % half) * kc + c) * PLANES + pl;
                        memcpy(img + base + piece * 1024 + (size_t)lane * 16 + 2 * q, &p[pl], 2);
                    }
                }
    }
    float* bias = reinterpret_cast<float*>(img + (size_t)half * kc * PLANES * 1024);
    for (int i = 0; i < 16 * wt; ++i) bias[i] = i < nout ? b[i] : 0.f;
}

inline int bf16_front_bytes(int wt) { return plane_front_bytes(wt, 3); }
inline int bf16_back_bytes(int wt) { return plane_back_bytes(wt, 3); }
inline int bf16_layer_bytes(int wt) { return plane_layer_bytes(wt, 3); }
inline void bf16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) {
    pack_plane_layer<3>(W, b, nin, nout, wt, dst, bf16_split3);
}

}  // namespace ac
