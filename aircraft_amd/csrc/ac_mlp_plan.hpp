// ac_mlp_plan.hpp — the weight plans the host hands to the MLP kernels by value.  Plain C++ (no HIP): the device engines
// (ac_mlp.hpp, ac_mlp_valu.hpp) and the host-side builder (ac_mlp_model.hpp) share these two structs.
#pragma once
#include "../../include/aircraft_hip.h"

namespace ac {

struct MlpPlan {
    int n_layers;
    int KT[AC_MAX_LAYERS];       // ceil(n_in / 16)
    int NT[AC_MAX_LAYERS];       // ceil(n_out / 16)
    int act[AC_MAX_LAYERS];      // 0 identity, 1 tanh; ac_set_mlp guarantees 1 on every layer but the last
    int g_off[AC_MAX_LAYERS];    // float offset of the packed layer block in the global blob
    int bytes[AC_MAX_LAYERS];    // block size: NT*KT*1024 (weights) + 1024 (bias piece)
    int lds_off[AC_MAX_LAYERS];  // byte offset if resident, -1 if streamed through the ring
    int ring_off[2];             // byte offsets of the two ring slots
    int n_streamed;              // number of streamed layers per forward pass
    int first_streamed;          // index of the first streamed layer (-1 if none)
    int streamed[AC_MAX_LAYERS]; // layer index of the i-th streamed layer, i < n_streamed
    int lds_total;               // dynamic LDS bytes to request
    int bf_region[3];            // plan_bf / plan_bf_pair: byte offsets of the half-layer regions of the bf16 hidden layers
};

constexpr int kLdsBudget = 160 * 1024;  // gfx950 LDS per workgroup

// Four-region ring of the one-wave f16 sensitivity kernel (MlpEngine::kRing4): a fourth half-layer region behind the three of
// plan_f16, at offset plan.lds_total, so that two slots of (front, back) hold two whole hidden layers.  Returns the dynamic
// LDS bytes of that launch, or 0 when the plan has no such ring: no hidden layer, regions that are not adjacent and 1 KiB
// aligned (a slot takes a layer as one run of pieces: region bytes = the front half's), or a total beyond the LDS.  A net
// that gets 0 keeps the three-region kernel.
constexpr int f16_ring4_lds(const MlpPlan& p, int front_bytes) {
    if (p.n_streamed < 1 || p.bf_region[0] < 0 || p.bf_region[2] < 0) return 0;
    const int region = p.bf_region[1] - p.bf_region[0];
    if (region != front_bytes || p.bf_region[2] - p.bf_region[1] != region || p.lds_total != p.bf_region[2] + region) return 0;
    if (region % 1024 != 0 || p.bf_region[0] % 1024 != 0) return 0;
    const int total = p.lds_total + region;
    return total <= kLdsBudget ? total : 0;
}
// Byte offset of slot k (0 or 1) of that ring: its front region, the back region behind it.
constexpr int f16_ring4_slot(const MlpPlan& p, int k) { return k ? p.bf_region[2] : p.bf_region[0]; }
// The ring's schedule.  ring_pos: streamed layers acquired so far; snext: position in streamed[] of the next layer to request
// (starts at 1, or 0 for a single streamed layer: the prologue loads streamed[0] into slot 0).  The layer acquired now is read
// from slot ring_pos & 1; behind the barrier at its head the layer streamed[snext] is requested into the other slot.
struct Ring4Step { int read_slot, next_layer, next_slot, snext; };
constexpr Ring4Step f16_ring4_step(const MlpPlan& p, int ring_pos, int snext) {
    return Ring4Step{ring_pos & 1, p.streamed[snext], (ring_pos & 1) ^ 1, snext + 1 == p.n_streamed ? 0 : snext + 1};
}

struct ValuPlan {
    int n_layers;                 // >= 2 (after the fold); layer 0: 8 (5 padded) -> W, hidden: W -> W, last: W -> 8 (6 padded)
    int act_last;                 // tanh on the last layer?
    int w_off[AC_MAX_LAYERS];     // float offset of the layer's weights in the image: [K][N] row-major (k-major) for all
                                  // layers but the last, which is stored transposed [8][K + 4] (padded rows)
    int b_off[AC_MAX_LAYERS];     // float offset of the bias (N floats, zero padded)
    int image_floats;             // padded to a multiple of 256 (whole 1-KiB LDS-DMA pieces)
};

}  // namespace ac
