// A test aid, not a product kernel: the two forms of the f16 activation split (MlpEngine::split_pair, f16 branch) side by
// side over every finite fp32 bit pattern with |x| < 2^15 — subnormals and both zeros included — once in the low and once in
// the high position of the pair, and the number of patterns on which the packed residual planes differ.
//   multiply form (before): lo' = v_cvt_pk_f16_f32((x - hi_x) S, (y - hi_y) S)
//   fused form (now):       lo' = v_fma_mixlo_f16(x - hi_x, S, 0) | v_fma_mixhi_f16(y - hi_y, S, 0)
// The hi plane and the residuals are the same instructions in both.  tests/test_gpu_f16_split_bits.py runs it.
#include <hip/hip_runtime.h>

#include "../../include/aircraft_hip.h"
#define AC_CH 2  // the output-tile chunk of the f16 units (build.py UNIT_FLAGS): the engine type below is theirs
#include "ac_mlp.hpp"

namespace ac {

typedef MlpEngine<6, 8, true, true, false, 0, 0, kHiddenF16> SplitEngine;
constexpr unsigned kSplitLimit = 0x47000000u;  // the bits of 2^15: magnitudes [0, kSplitLimit) are the finite |x| < 2^15

struct SplitPlanes { unsigned hi, lo_mul, lo_fused; };

AC_DI SplitPlanes split_both(float x, float y) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    SplitPlanes o;
    o.hi = SplitEngine::cvt_pk_f16(f32x2{x, y});
    const float rx = SplitEngine::sub_f16_lo(x, o.hi), ry = SplitEngine::sub_f16_hi(y, o.hi);
    o.lo_mul = SplitEngine::cvt_pk_f16(f32x2{rx * SplitEngine::kLoScale, ry * SplitEngine::kLoScale});
    o.lo_fused = SplitEngine::scale_f16_hi(SplitEngine::scale_f16_lo(rx), ry);
    return o;
}

// out[0]: patterns that differ in the low position, out[1]: in the high position, out[2]: patterns visited,
// out[3]: one differing pattern + 1 (0: none)
__global__ __launch_bounds__(256) void k_f16_split_check(unsigned long long* __restrict__ out) {
    const unsigned long long total = 2ull * kSplitLimit;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned bad_lo = 0, bad_hi = 0, seen = 0, first = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned mag = (unsigned)(i >> 1), bits = mag | ((unsigned)(i & 1) << 31);
        // the partner in the other half of the pair: another pattern of the same range, spread over magnitudes and signs
        const unsigned pm = (unsigned)((mag * 2654435761ull + 0x9e3779b9ull) % kSplitLimit), pbits = pm | ((mag & 2u) << 30);
        const float x = __uint_as_float(bits), p = __uint_as_float(pbits);
        const SplitPlanes a = split_both(x, p), b = split_both(p, x);
        const bool dl = a.lo_mul != a.lo_fused, dh = b.lo_mul != b.lo_fused;
        bad_lo += dl;
        bad_hi += dh;
        if ((dl || dh) && !first) first = bits + 1u;
        ++seen;
    }
    if (bad_lo) atomicAdd(&out[0], (unsigned long long)bad_lo);
    if (bad_hi) atomicAdd(&out[1], (unsigned long long)bad_hi);
    atomicAdd(&out[2], (unsigned long long)seen);
    if (first) atomicMax(&out[3], (unsigned long long)first);
}

}  // namespace ac

extern "C" int ac_f16_split_check(unsigned long long out[4]) {
    if (!out) return AC_ERR_BAD_ARG;
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, 4 * sizeof(unsigned long long)) != hipSuccess) return AC_ERR_HIP;
    int rc = AC_OK;
    if (hipMemset(d, 0, 4 * sizeof(unsigned long long)) != hipSuccess) rc = AC_ERR_HIP;
    if (rc == AC_OK) {
        hipLaunchKernelGGL(ac::k_f16_split_check, 4096, 256, 0, 0, d);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = AC_ERR_HIP;
    }
    if (rc == AC_OK && hipMemcpy(out, d, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) rc = AC_ERR_HIP;
    (void)hipFree(d);
    return rc;
}
