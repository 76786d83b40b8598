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

struct ValuPlan {
    int n_layers;                 // >= 2 (after the fold); layer 0: 8 (5 padded) -> W, hidden: W -> W, last: W -> 8 (6 padded)
    int act_last;                 // tanh on the last layer?
    int w_off[AC_MAX_LAYERS];     // float offset of the layer's weights in the image: [K][N] row-major (k-major) for all
                                  // layers but the last, which is stored transposed [8][K + 4] (padded rows)
    int b_off[AC_MAX_LAYERS];     // float offset of the bias (N floats, zero padded)
    int image_floats;             // padded to a multiple of 256 (whole 1-KiB LDS-DMA pieces)
};

}  // namespace ac
