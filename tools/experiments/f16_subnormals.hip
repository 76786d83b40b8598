// f16_subnormals.hip — what gfx950 does with subnormal f16 values in the three instructions of the two-plane f16 hidden
// layers (MlpEngine::layer_bf), under the default MODE of a HIP kernel.  One wave, run once:
//
//   hipcc --offload-arch=gfx950 -O2 tools/experiments/f16_subnormals.hip -o f16_subnormals && ./f16_subnormals
//
//   1. v_mfma_f32_16x16x32_f16: A = 2^-20 (subnormal f16) in every element, B = 1.0: D = 32 * 2^-20 if honoured, 0 if flushed;
//      and the other way round (A = 1.0, B = 2^-20).
//   2. v_cvt_pk_f16_f32 of 2^-20: bits 0x0010 if honoured, 0 if flushed.
//   3. v_fma_mix_f32 reading the subnormal half 0x0010 (low and high half): x - h = 1 - 2^-20 if honoured, 1 if flushed.
// It also checks the split's identities on a normal value: x - hi exact through v_fma_mix_f32 for both halves.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__global__ void k_probe(float* out, unsigned* bits) {
    const _Float16 tiny = (_Float16)9.5367431640625e-07f;  // 2^-20, exact as an f16 subnormal (0x0010)
    f16x8 a, b;
    for (int i = 0; i < 8; ++i) { a[i] = tiny; b[i] = (_Float16)1.0f; }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    const f32x4 d0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    const f32x4 d1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0);
    float tf = 9.5367431640625e-07f, big = 0.333251953125f + 1.0e-5f;
    asm volatile("" : "+v"(tf), "+v"(big));
    const unsigned pk = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{tf, tf}, f16x2));
    float one = 1.0f, mlo, mhi;
    asm volatile("" : "+v"(one));
    asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(mlo) : "v"(pk), "v"(one));
    asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(mhi) : "v"(pk), "v"(one));
    // a normal pair: the residuals x - f16(x), y - f16(y) through the same instruction
    float x = big, y = -3.0f * big;
    const unsigned pn = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x, y}, f16x2));
    float rx, ry;
    asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(rx) : "v"(pn), "v"(x));
    asm volatile("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(ry) : "v"(pn), "v"(y));
    if (threadIdx.x == 0) {
        out[0] = d0[0]; out[1] = d1[0]; out[2] = mlo; out[3] = mhi; out[4] = x; out[5] = y; out[6] = rx; out[7] = ry;
        bits[0] = pk; bits[1] = pn;
    }
}

static float half_bits_to_float(unsigned h) {
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    const float v = e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(m | 0x400), e - 25);
    return (h & 0x8000u) ? -v : v;
}

int main() {
    float* d_out; unsigned* d_bits;
    if (hipMalloc(&d_out, 64) != hipSuccess || hipMalloc(&d_bits, 64) != hipSuccess) { printf("hipMalloc failed\n"); return 2; }
    hipLaunchKernelGGL(k_probe, 1, 64, 0, 0, d_out, d_bits);
    float o[8]; unsigned bb[2];
    if (hipMemcpy(o, d_out, sizeof(o), hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 2; }
    (void)hipMemcpy(bb, d_bits, sizeof(bb), hipMemcpyDeviceToHost);
    const float want = 32.0f * 9.5367431640625e-07f;
    printf("mfma A subnormal: D = %.9g (honoured: %.9g) -> %s\n", o[0], want, o[0] == want ? "HONOURED" : (o[0] == 0.f ? "FLUSHED" : "OTHER"));
    printf("mfma B subnormal: D = %.9g (honoured: %.9g) -> %s\n", o[1], want, o[1] == want ? "HONOURED" : (o[1] == 0.f ? "FLUSHED" : "OTHER"));
    printf("v_cvt_pk_f16_f32(2^-20): 0x%08x -> %s\n", bb[0], bb[0] == 0x00100010u ? "HONOURED" : (bb[0] == 0 ? "FLUSHED" : "OTHER"));
    const float wm = 1.0f - 9.5367431640625e-07f;
    printf("v_fma_mix_f32 low half:  1 - h = %.9g -> %s\n", o[2], o[2] == wm ? "HONOURED" : (o[2] == 1.f ? "FLUSHED" : "OTHER (or cvt flushed)"));
    printf("v_fma_mix_f32 high half: 1 - h = %.9g -> %s\n", o[3], o[3] == wm ? "HONOURED" : (o[3] == 1.f ? "FLUSHED" : "OTHER (or cvt flushed)"));
    const float ex = o[4] - half_bits_to_float(bb[1] & 0xffffu), ey = o[5] - half_bits_to_float(bb[1] >> 16);
    printf("residuals of a normal pair: %.9g %.9g (expected %.9g %.9g) -> %s\n", o[6], o[7], ex, ey, (o[6] == ex && o[7] == ey) ? "EXACT" : "MISMATCH");
    return 0;
}
