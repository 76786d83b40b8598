// Host build of the bf16 three-plane split and layer packing (aircraft_amd/csrc/ac_bf16_pack.hpp) for
// tests/test_mlp_bf16_planes.py.
#include "../../aircraft_amd/csrc/ac_bf16_pack.hpp"

extern "C" {
int host_bf16_layer_bytes(int wt) { return ac::bf16_layer_bytes(wt); }
int host_bf16_front_bytes(int wt) { return ac::bf16_front_bytes(wt); }
void host_bf16_split3(const float* w, long n, unsigned short* planes) {  // planes: [n][3]
    for (long i = 0; i < n; ++i) ac::bf16_split3(w[i], planes + 3 * i);
}
void host_bf16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) {
    ac::bf16_pack_layer(W, b, nin, nout, wt, dst);
}
}
