// ac_mlp_model.hpp — everything ac_set_mlp computes on the host before it touches the device: the folded net, the packed
// weight blob, the LDS plans of every kernel family, and the weight image of the tiled vector-ALU engine.  Plain C++ (no
// HIP): abi_core.hip uploads what build_mlp_model returns, and tests/test_mlp_model_host.py checks it with g++ alone.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ac_bf16_pack.hpp"
#include "ac_f16_pack.hpp"
#include "ac_mlp_plan.hpp"

namespace ac {

// What the handle keeps of a model once blob and image are on the device.
struct MlpModelInfo {
    MlpPlan plan;
    MlpPlan plan_sens;      // the MFMA sensitivity engines' plan: last layer = [bias][wlt] for MlpEngine::last_valu
    MlpPlan plan_rev;       // width 128, <= 3 hidden products: plan_sens + the TRANSPOSED hidden blocks of the reverse sweep
    MlpPlan plan_bf;        // width 128 (wt 8): plan_sens with the hidden layers as three-plane bf16 images streamed in
    MlpPlan plan_bf_pair;   // half-layer regions — three rotating (k_nn_step_sens), two (k_nn_step_sens_pair)
    MlpPlan plan_f16;       // the same two plans over the two-plane f16 images (ac_f16_pack.hpp): the route of a net that
    MlpPlan plan_f16_pair;  // passes the range gate (f16_gate); plan_bf / plan_bf_pair stay its fall-back
    bool has_bf;
    int f16_gate;           // F16Gate code of the net (0: passes); meaningful when has_bf
    int f16_ring4_lds;      // LDS bytes of the one-wave f16 kernel on its four-region ring (f16_ring4_lds); 0: three regions
    bool has_rev;           // reverse sweep of k_nn_stage_tensors_rev (ac_hess_rev.hpp); rev_layers = layers of the net itself
    int rev_layers;
    int wt;                 // register tiles per slab the plan needs (2, 4 or 8)
    int use_mfma;
    // "MFMA off" flavour on the tiled v_pk_fma_f32 engine (ac_mlp_valu.hpp): hidden widths <= 64, >= 2 layers
    bool has_vplan;
    ValuPlan vplan;
    int vwidth;             // 32 or 64
};

struct MlpModel : MlpModelInfo {
    std::vector<float> blob;    // packed weights + biases; every plan's g_off is a float offset into it
    std::vector<float> vimage;  // weight image [layer][K][N] (+ biases) of the vector-ALU engine; empty unless has_vplan
    // the folded net, rounded once to fp32: W[l] is [widths[l + 1]][widths[l]] row-major
    std::vector<int> widths, act;
    std::vector<std::vector<float>> W, b;
};

// Fold every activation-free layer that is not the last into its successor (in float64):
//   W2 (W1 x + b1) + b2 = (W2 W1) x + (W2 b1 + b2).
// The device engines then see tanh on every layer but the last (a compile-time fact in the hidden-layer epilogues,
// which are exposed VALU time) and the reference checkpoint's Linear-Linear-Tanh-Linear net (surrogates/models.py:
// 114-123) runs as 5-32-6 instead of 5-16-32-6.
inline void fold_linear_layers(int n_layers, const int* widths, const int* act, const float* const* W, const float* const* b,
                               MlpModel& m) {
    struct HostLayer { int nin, nout, act; std::vector<double> W, b; };
    std::vector<HostLayer> net((size_t)n_layers);
    for (int l = 0; l < n_layers; ++l) {
        HostLayer& L = net[(size_t)l];
        L.nin = widths[l]; L.nout = widths[l + 1]; L.act = act[l] ? 1 : 0;
        L.W.assign(W[l], W[l] + (size_t)L.nin * L.nout);
        L.b.assign(b[l], b[l] + L.nout);
    }
    for (size_t l = 0; l + 1 < net.size();) {
        if (net[l].act) { ++l; continue; }
        const HostLayer &A = net[l], &B = net[l + 1];
        HostLayer M;
        M.nin = A.nin; M.nout = B.nout; M.act = B.act;
        M.W.assign((size_t)M.nin * M.nout, 0.0);
        M.b = B.b;
        for (int i = 0; i < B.nout; ++i)
            for (int k = 0; k < B.nin; ++k) {
                const double w = B.W[(size_t)i * B.nin + k];
                M.b[(size_t)i] += w * A.b[(size_t)k];
                for (int j = 0; j < A.nin; ++j) M.W[(size_t)i * M.nin + j] += w * A.W[(size_t)k * A.nin + j];
            }
        net[l] = std::move(M);
        net.erase(net.begin() + (long)l + 1);
    }
    m.widths.assign(1, net[0].nin);
    m.act.clear(); m.W.clear(); m.b.clear();
    for (const HostLayer& L : net) {
        m.widths.push_back(L.nout);
        m.act.push_back(L.act);  // 1 for every layer but the last after the fold
        m.W.emplace_back(L.W.begin(), L.W.end());
        m.b.emplace_back(L.b.begin(), L.b.end());
    }
}

// MFMA fragment order [nt][kt][lane][4]: lane = col + 16 g holds M[16 nt + col][16 kt + 4 g + j], j = 0..3, zero outside
// the matrix.  M is W ([nout][nin] row-major) or, for the blocks of the reverse sweep, its transpose.
inline void pack_fragments(const float* W, int nin, int nout, bool transposed, int NT, int KT, float* dst) {
    const int rows = transposed ? nin : nout, cols = transposed ? nout : nin;
    for (int nt = 0; nt < NT; ++nt)
        for (int kt = 0; kt < KT; ++kt)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int row = 16 * nt + (lane & 15), k = 16 * kt + 4 * (lane >> 4) + j;
                    const size_t src = transposed ? (size_t)k * nin + row : (size_t)row * nin + k;
                    dst[((size_t)(nt * KT + kt) * 64 + lane) * 4 + j] = (row < rows && k < cols) ? W[src] : 0.f;
                }
}

// wlt, the per-lane weight pairs of MlpEngine::last_valu: [wt tiles][4 lane groups][6 float4] =
// {W(2kp, n), W(2kp+1, n), W(2kp, n+1), W(2kp+1, n+1)} at n = 16 t + 4 g + 2 rp, float4 index 2 kp + rp.
inline void pack_wlt(const float* W, int nin, int nout, int wt, float* wl) {
    auto wv = [&](int k, int n) { return (k < nout && n < nin) ? W[(size_t)k * nin + n] : 0.f; };
    for (int t = 0; t < wt; ++t)
        for (int g = 0; g < 4; ++g)
            for (int kp = 0; kp < 3; ++kp)
                for (int rp = 0; rp < 2; ++rp) {
                    float* q = wl + (size_t)(((t * 4 + g) * 6) + 2 * kp + rp) * 4;
                    const int n0 = 16 * t + 4 * g + 2 * rp;
                    q[0] = wv(2 * kp, n0); q[1] = wv(2 * kp + 1, n0); q[2] = wv(2 * kp, n0 + 1); q[3] = wv(2 * kp + 1, n0 + 1);
                }
}

// LDS plan: everything resident if it fits; otherwise the largest layers stream through a 2-slot ring.
// force_stream: the largest size class goes through the ring even when everything would fit (plan_rev of a net with ONE
// hidden product: the reverse-sweep kernel sequences its hidden and transposed blocks through the ring by hand)
inline int plan_lds(MlpPlan& pl, bool force_stream, char* err, size_t errlen) {
    const int n_layers = pl.n_layers;  // (plan_rev carries more blocks than the net has layers)
    pl.n_streamed = 0; pl.first_streamed = -1;
    int total = 0;
    for (int l = 0; l < n_layers; ++l) total += pl.bytes[l];
    for (int l = 0; l < n_layers; ++l) pl.lds_off[l] = 0;
    if (total <= kLdsBudget && !force_stream) {
        int off = 0;
        for (int l = 0; l < n_layers; ++l) { pl.lds_off[l] = off; off += pl.bytes[l]; }
        pl.lds_total = off;
    } else {
        int big = 0;
        for (int l = 0; l < n_layers; ++l) big = std::max(big, pl.bytes[l]);
        // stream every layer of the maximal size class; keep the rest resident
        int off = 0, resident = 0;
        for (int l = 0; l < n_layers; ++l) if (pl.bytes[l] < big) resident += pl.bytes[l];
        if (resident + 2 * big > kLdsBudget) {
            snprintf(err, errlen, "MLP does not fit the LDS plan (%d resident + 2 x %d ring)", resident, big);
            return (int)AC_ERR_UNSUPPORTED;
        }
        for (int l = 0; l < n_layers; ++l) {
            if (pl.bytes[l] < big) { pl.lds_off[l] = off; off += pl.bytes[l]; }
            else { pl.lds_off[l] = -1; pl.n_streamed++; if (pl.first_streamed < 0) pl.first_streamed = l; }
        }
        pl.ring_off[0] = off; pl.ring_off[1] = off + big;
        pl.lds_total = off + 2 * big;
    }
    for (int l = 0, i = 0; l < n_layers; ++l)
        if (pl.lds_off[l] < 0) pl.streamed[i++] = l;
    return AC_OK;
}

// plan_bf / plan_f16: the edge blocks of plan_sens resident where they are, every hidden layer (its plane image of
// layer_bytes at g_off[l]) streamed through three rotating half-layer regions behind them (MlpEngine::acquire, BF engines)
inline MlpPlan hidden_ring_plan(const MlpPlan& ps, int layer_bytes, int region_bytes, const size_t* g_off) {
    MlpPlan p = ps;
    const int last = ps.n_layers - 1;
    p.lds_off[0] = 0; p.lds_off[last] = ps.bytes[0];
    const int edge = ps.bytes[0] + ps.bytes[last];
    p.n_streamed = 0; p.first_streamed = 1;
    for (int l = 1; l < last; ++l) {
        p.lds_off[l] = -1; p.g_off[l] = (int)g_off[l]; p.bytes[l] = layer_bytes;
        p.streamed[p.n_streamed++] = l;
    }
    for (int i = 0; i < 3; ++i) p.bf_region[i] = edge + i * region_bytes;
    p.ring_off[0] = p.ring_off[1] = -1;
    p.lds_total = edge + 3 * region_bytes;
    return p;
}
// ... and the pair kernel's form of such a plan: two regions
inline MlpPlan drop_third_region(MlpPlan p) {
    p.lds_total = p.bf_region[2];
    p.bf_region[2] = -1;
    return p;
}

// "MFMA off": weight image of the tiled vector-ALU engine, k-major [K][N] per layer (the last layer transposed [8][K + 4]),
// hidden widths zero-padded to vw = 32 or 64.  False when image + activation buffers do not fit the LDS.
inline bool build_valu_image(const MlpModel& m, int vw, ValuPlan& vp, std::vector<float>& img) {
    const int n_layers = (int)m.W.size();
    vp.n_layers = n_layers;
    vp.act_last = m.act[(size_t)n_layers - 1];
    size_t off = 0;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        const int K = l == 0 ? 8 : vw, N = last ? 8 : vw;
        vp.w_off[l] = (int)off; off += last ? (size_t)N * (K + 4) : (size_t)K * N;  // last layer: transposed, rows padded
        vp.b_off[l] = (int)off; off += (size_t)N;
    }
    vp.image_floats = (int)((off + 255) / 256 * 256);
    if (vp.image_floats * 4 + 4 * 96 * (vw + 4) * 4 > kLdsBudget) return false;
    img.assign((size_t)vp.image_floats, 0.f);
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        const int nin = m.widths[(size_t)l], nout = m.widths[(size_t)l + 1], K = l == 0 ? 8 : vw, N = last ? 8 : vw;
        float* wd = img.data() + vp.w_off[l];
        for (int k = 0; k < nin; ++k)
            for (int nn = 0; nn < nout; ++nn) {
                const float wv = m.W[(size_t)l][(size_t)nn * nin + k];
                if (last) wd[(size_t)nn * (K + 4) + k] = wv;   // Wt[j][k], row stride K + 4
                else wd[(size_t)k * N + nn] = wv;        // W[k][n]
            }
        for (int nn = 0; nn < nout; ++nn) img[(size_t)vp.b_off[l] + nn] = m.b[(size_t)l][(size_t)nn];
    }
    return true;
}

// widths: [n_layers + 1] (5 ... 6); act[l] != 0: tanh on layer l; W[l]: [widths[l + 1]][widths[l]] row-major.
// Returns AC_OK, or an error code with its text in err (AC_ERR_UNSUPPORTED) and `out` unspecified.
inline int build_mlp_model(int n_layers, const int* widths, const int* act, const float* const* W, const float* const* b,
                           int use_mfma, MlpModel& out, char* err, size_t errlen) {
    if (!widths || !act || !W || !b) return AC_ERR_BAD_ARG;
    if (n_layers < 1 || n_layers > AC_MAX_LAYERS) return AC_ERR_BAD_ARG;
    if (widths[0] != 5 || widths[n_layers] != 6) return AC_ERR_BAD_ARG;
    for (int l = 0; l <= n_layers; ++l) {
        if (widths[l] < 1) return AC_ERR_BAD_ARG;
        if (widths[l] > AC_MAX_WIDTH) {
            snprintf(err, errlen, "MLP width %d > AC_MAX_WIDTH %d", widths[l], AC_MAX_WIDTH);
            return AC_ERR_UNSUPPORTED;
        }
    }
    for (int l = 0; l < n_layers; ++l)
        if (!W[l] || !b[l]) return AC_ERR_BAD_ARG;
    MlpModel m;
    static_cast<MlpModelInfo&>(m) = MlpModelInfo{};
    fold_linear_layers(n_layers, widths, act, W, b, m);
    n_layers = (int)m.W.size();
    widths = m.widths.data();
    // Hidden widths are zero-padded to one common multiple of 16 (wt tiles): padded neurons get zero weights
    // and zero bias, so they output act(0) = 0 and feed nothing forward.  Input (5) pads to one tile, output (6)
    // to one tile.  The engine then only meets the static shapes <1,wt>, <wt,wt>, <wt,1>, <1,1>.
    int maxh = 0;
    for (int l = 1; l < n_layers; ++l) maxh = std::max(maxh, widths[l]);
    const int maxt = (maxh + 15) / 16;
    const int wt = maxt <= 2 ? 2 : (maxt <= 4 ? 4 : 8);
    const int last = n_layers - 1, n_hid = n_layers - 2;

    // ---- blob layout: the net's own blocks, then the reverse sweep's, then the bf16 and the f16 images of the hidden layers
    MlpPlan& pl = m.plan;
    pl.n_layers = n_layers;
    size_t total_floats = 0;
    const int wlt_bytes = ((wt * 384 + 1023) / 1024) * 1024;  // [wt tiles][4 lane groups][6 float4], whole LDS-DMA pieces
    for (int l = 0; l < n_layers; ++l) {
        pl.KT[l] = (l == 0) ? 1 : wt;
        pl.NT[l] = (l == last) ? 1 : wt;
        pl.act[l] = m.act[(size_t)l];
        pl.bytes[l] = pl.NT[l] * pl.KT[l] * 1024 + 1024;  // weights + one 1-KiB bias piece (whole LDS-DMA pieces only)
        // first layer of a multi-layer net: + W0 transposed [5][16*wt] for the MFMA-free tangent slabs
        if (l == 0 && n_layers > 1) pl.bytes[l] += ((5 * wt * 64 + 1023) / 1024) * 1024;
        pl.g_off[l] = (int)total_floats;
        total_floats += (size_t)pl.bytes[l] / 4;
        // last layer of a multi-layer net: + wlt — in the global blob only; plan_sens (below) copies [bias][wlt] to LDS,
        // `pl` the fragments and the bias
        if (l == last && n_layers > 1) total_floats += (size_t)wlt_bytes / 4;
    }
    // Width 128 with one to three hidden products: the transposed hidden blocks of the reverse sweep
    // (k_nn_stage_tensors_rev, both flavours of the matrix product), top hidden layer first.
    const bool want_rev = wt == 8 && n_hid >= 1 && n_layers + n_hid <= AC_MAX_LAYERS;
    const size_t rev_block_floats = (size_t)wt * wt * 256 + 256;  // fragments + a (zero) bias piece: the hidden blocks' size class
    // Width 128 with hidden layers: their three-plane bf16 images for the sensitivity kernels' layer_bf, and their two-plane
    // f16 images behind those; which of the two the kernels read is decided per net by the range gate (and ac_set_hidden_route)
    const bool want_bf = wt == 8 && n_hid >= 1;
    size_t rev_off[AC_MAX_LAYERS] = {0}, bf_off[AC_MAX_LAYERS] = {0}, f16_off[AC_MAX_LAYERS] = {0};
    if (want_rev)
        for (int i = 0; i < n_hid; ++i) { rev_off[i] = total_floats; total_floats += rev_block_floats; }
    if (want_bf) {
        for (int l = 1; l < last; ++l) { bf_off[l] = total_floats; total_floats += (size_t)bf16_layer_bytes(wt) / 4; }
        for (int l = 1; l < last; ++l) { f16_off[l] = total_floats; total_floats += (size_t)f16_layer_bytes(wt) / 4; }
    }

    // ---- fill
    m.blob.assign(total_floats, 0.f);
    float* blob = m.blob.data();
    for (int l = 0; l < n_layers; ++l) {
        const float* Wl = m.W[(size_t)l].data();
        const int nin = widths[l], nout = widths[l + 1], NT = pl.NT[l], KT = pl.KT[l];
        float* dst = blob + pl.g_off[l];
        pack_fragments(Wl, nin, nout, false, NT, KT, dst);
        float* bd = dst + (size_t)NT * KT * 256;
        for (int i = 0; i < NT * 16; ++i) bd[i] = i < nout ? m.b[(size_t)l][(size_t)i] : 0.f;
        float* tail = bd + 256;  // after the 1-KiB bias piece
        if (l == 0 && n_layers > 1)
            for (int j = 0; j < 5; ++j)
                for (int n = 0; n < wt * 16; ++n) tail[j * wt * 16 + n] = n < nout ? Wl[(size_t)n * nin + j] : 0.f;
        if (l == last && n_layers > 1) pack_wlt(Wl, nin, nout, wt, tail);
    }
    if (want_rev)
        for (int i = 0; i < n_hid; ++i) {
            const int l = n_hid - i;  // forward layer l: h_l (nin) -> h_{l+1} (nout); the block multiplies by its transpose
            pack_fragments(m.W[(size_t)l].data(), widths[l], widths[l + 1], true, wt, wt, blob + rev_off[i]);
        }
    m.f16_gate = F16_GATE_OK;
    if (want_bf) {
        std::vector<const float*> gw, gb;
        for (int l = 0; l < n_layers; ++l) { gw.push_back(m.W[(size_t)l].data()); gb.push_back(m.b[(size_t)l].data()); }
        for (int l = 1; l < last; ++l) {
            bf16_pack_layer(gw[(size_t)l], gb[(size_t)l], widths[l], widths[l + 1], wt, blob + bf_off[l]);
            f16_pack_layer(gw[(size_t)l], gb[(size_t)l], widths[l], widths[l + 1], wt, blob + f16_off[l]);
        }
        m.f16_gate = f16_gate(n_layers, widths, gw.data(), gb.data());
    }

    // ---- plans
    { const int rc = plan_lds(pl, false, err, errlen); if (rc != AC_OK) return rc; }
    // plan_sens: the first and last layers run on the vector ALUs there (MlpEngine::first_valu / last_valu), so their LDS
    // copies leave the MFMA fragments out: [bias 1 KiB][W0 transposed] and [bias 1 KiB][wlt] (the blob keeps the fragments
    // in front of them for the other kernels)
    MlpPlan& ps = m.plan_sens = pl;
    if (n_layers > 1) {
        ps.g_off[0] = pl.g_off[0] + pl.NT[0] * pl.KT[0] * 256;
        ps.bytes[0] = pl.bytes[0] - pl.NT[0] * pl.KT[0] * 1024;
        ps.g_off[last] = pl.g_off[last] + pl.NT[last] * pl.KT[last] * 256;
        ps.bytes[last] = 1024 + wlt_bytes;
        const int rc = plan_lds(ps, false, err, errlen);
        if (rc != AC_OK) return rc;
    }
    // the f16 regions are 33 KiB where the bf16 ones are 49
    m.plan_bf = m.plan_f16 = ps;
    if (want_bf) {
        m.plan_bf = hidden_ring_plan(ps, bf16_layer_bytes(wt), bf16_front_bytes(wt), bf_off);
        m.plan_f16 = hidden_ring_plan(ps, f16_layer_bytes(wt), f16_front_bytes(wt), f16_off);
        if (m.plan_bf.lds_total > kLdsBudget) {
            snprintf(err, errlen, "%s", "bf16 hidden-layer ring does not fit the LDS");
            return AC_ERR_UNSUPPORTED;
        }
    }
    m.plan_bf_pair = want_bf ? drop_third_region(m.plan_bf) : ps;
    m.plan_f16_pair = want_bf ? drop_third_region(m.plan_f16) : ps;
    m.f16_ring4_lds = want_bf ? f16_ring4_lds(m.plan_f16, f16_front_bytes(wt)) : 0;
    MlpPlan& pr = m.plan_rev = ps;
    if (want_rev) {
        for (int i = 0; i < n_hid; ++i) {
            const int e = n_layers + i;
            pr.KT[e] = wt; pr.NT[e] = wt; pr.act[e] = 0;
            pr.g_off[e] = (int)rev_off[i];
            pr.bytes[e] = (int)(rev_block_floats * 4);
        }
        pr.n_layers = n_layers + n_hid;
        // the kernel expects the hidden and the transposed blocks to stream (one size class) and the edge blocks to stay
        m.has_rev = plan_lds(pr, /*force_stream=*/true, err, errlen) == AC_OK && pr.n_streamed == 2 * n_hid &&
                    pr.lds_off[0] >= 0 && pr.lds_off[last] >= 0;
    }
    m.has_bf = want_bf;
    m.rev_layers = n_layers;
    m.wt = wt;
    m.use_mfma = use_mfma ? 1 : 0;
    // Nets the vector-ALU engine does not cover (wider than 64, or a single layer after the fold) keep the cross-lane
    // validation path.
    m.vwidth = maxh <= 32 ? 32 : 64;
    m.has_vplan = !use_mfma && n_layers >= 2 && maxh <= 64 && build_valu_image(m, m.vwidth, m.vplan, m.vimage);
    out = std::move(m);
    return AC_OK;
}

}  // namespace ac
