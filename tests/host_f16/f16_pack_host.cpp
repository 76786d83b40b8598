// Host build of the f16 two-plane split, the layer packing and the range gate (aircraft_amd/csrc/ac_f16_pack.hpp) for
// tests/test_mlp_f16_planes.py.
#include "../../aircraft_amd/csrc/ac_f16_pack.hpp"

extern "C" {
int host_f16_layer_bytes(int wt) { return ac::f16_layer_bytes(wt); }
int host_f16_front_bytes(int wt) { return ac::f16_front_bytes(wt); }
void host_f16_split2(const float* w, long n, unsigned short* planes) {  // planes: [n][2]
    for (long i = 0; i < n; ++i) ac::f16_split2(w[i], planes + 2 * i);
}
void host_f16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) {
    ac::f16_pack_layer(W, b, nin, nout, wt, dst);
}
// widths: [n_layers + 1]; W, b: one pointer per layer
int host_f16_gate(int n_layers, const int* widths, const float* const* W, const float* const* b, double* worst) {
    return ac::f16_gate(n_layers, widths, W, b, worst);
}
}
