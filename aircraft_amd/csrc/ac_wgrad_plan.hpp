// ac_wgrad_plan.hpp — the host half of the weight gradient (ac_wgrad.hpp): the plan and the fragment image ac_set_mlp prepares.
// Plain C++ on its own, so that the handle (ac_abi.hpp) holds a WgradPlan without the kernels of ac_wgrad.hpp behind it.
#pragma once
#include "ac_mlp_model.hpp"

namespace ac {

// ---- host side: what ac_set_mlp prepares (plain C++) ---------------------------------------------------------------------------
// The folded net as k_mlp_wgrad reads it: per layer the forward fragments W [NT][KT][64 lanes][4] (pack_fragments), the bias
// (NT * 16 floats, zero padded) and — for every layer but the first — the fragments of W' [KT][NT][64][4], the A operand of
// the backward-data product.  Hidden widths are padded to 16 wt as everywhere else; padding is zero.
struct WgradPlan {
    int n_layers;
    int nin[AC_MAX_LAYERS], nout[AC_MAX_LAYERS];   // logical sizes of the folded layers
    int wf_off[AC_MAX_LAYERS], b_off[AC_MAX_LAYERS], wt_off[AC_MAX_LAYERS];  // float offsets into the image
    int g_off[AC_MAX_LAYERS];                      // float offset of W[l] in the gradient vector; b[l] follows its W[l]
    int grad_floats;                               // sum of nout (nin + 1)
    int image_floats;
    int act_last;                                  // tanh on the last layer (not supported by the weight gradient)
};

constexpr int kWgSamples = 32;      // samples per tile of k_mlp_wgrad
constexpr int kWgRowStride = 36;    // floats between activation rows in LDS (32 samples + 4: conflict-free operand reads)
constexpr int kWgBlock = 256;
// hidden-to-hidden layers whose accumulators one workgroup holds in registers (64 per wave and layer at width 128)
constexpr int wgrad_max_hidden_products(int wt) { return wt == 8 ? 3 : 6; }
// activation rows in LDS: z and ybar (16 each), one block of 16 wt rows per hidden layer, two for the deltas
inline int wgrad_lds_bytes(int n_layers, int wt) {
    const int rows = 32 + (n_layers > 1 ? (n_layers - 1 + 2) * 16 * wt : 0);
    return rows * kWgRowStride * (int)sizeof(float);
}

inline void build_wgrad_image(const MlpModel& m, WgradPlan& p, std::vector<float>& img) {
    const int L = (int)m.W.size(), wt = m.wt;
    p = WgradPlan{};
    p.n_layers = L;
    p.act_last = m.act[(size_t)L - 1];
    size_t off = 0;
    int g = 0;
    for (int l = 0; l < L; ++l) {
        const int NT = l == L - 1 ? 1 : wt, KT = l == 0 ? 1 : wt;
        p.nin[l] = m.widths[(size_t)l]; p.nout[l] = m.widths[(size_t)l + 1];
        p.wf_off[l] = (int)off; off += (size_t)NT * KT * 256;
        p.b_off[l] = (int)off; off += (size_t)NT * 16;
        p.wt_off[l] = (int)off; if (l > 0) off += (size_t)NT * KT * 256;
        p.g_off[l] = g; g += p.nout[l] * (p.nin[l] + 1);
    }
    p.grad_floats = g;
    p.image_floats = (int)off;
    img.assign(off, 0.f);
    for (int l = 0; l < L; ++l) {
        const int NT = l == L - 1 ? 1 : wt, KT = l == 0 ? 1 : wt;
        const float* W = m.W[(size_t)l].data();
        pack_fragments(W, p.nin[l], p.nout[l], false, NT, KT, img.data() + p.wf_off[l]);
        for (int i = 0; i < p.nout[l]; ++i) img[(size_t)p.b_off[l] + i] = m.b[(size_t)l][(size_t)i];
        if (l > 0) pack_fragments(W, p.nin[l], p.nout[l], true, KT, NT, img.data() + p.wt_off[l]);
    }
}

}  // namespace ac
