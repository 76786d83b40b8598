// Host build of the MLP model builder (aircraft_amd/csrc/ac_mlp_model.hpp) for tests/test_mlp_model_host.py: the blob, the
// plans and the vector-ALU image of a net, as ac_set_mlp would upload them.
#include "../../aircraft_amd/csrc/ac_mlp_model.hpp"

namespace {
struct Built {
    ac::MlpModel m;
    int rc;
    char err[512];
};
}  // namespace

extern "C" {
// widths: [n_layers + 1]; act: [n_layers]; W, b: one pointer per layer.  Never NULL: the status is in host_mlp_rc.
void* host_mlp_build(int n_layers, const int* widths, const int* act, const float* const* W, const float* const* b, int use_mfma) {
    Built* p = new Built();
    p->err[0] = 0;
    p->rc = ac::build_mlp_model(n_layers, widths, act, W, b, use_mfma, p->m, p->err, sizeof(p->err));
    return p;
}
void host_mlp_free(void* h) { delete static_cast<Built*>(h); }
int host_mlp_rc(const void* h) { return static_cast<const Built*>(h)->rc; }
const char* host_mlp_err(const void* h) { return static_cast<const Built*>(h)->err; }

int host_mlp_plan_ints(void) { return (int)(sizeof(ac::MlpPlan) / sizeof(int)); }
int host_mlp_vplan_ints(void) { return (int)(sizeof(ac::ValuPlan) / sizeof(int)); }
// which: 0 plan, 1 plan_sens, 2 plan_rev, 3 plan_bf, 4 plan_bf_pair, 5 plan_f16, 6 plan_f16_pair
void host_mlp_plan(const void* h, int which, int* dst) {
    const ac::MlpModel& m = static_cast<const Built*>(h)->m;
    const ac::MlpPlan* plans[7] = {&m.plan, &m.plan_sens, &m.plan_rev, &m.plan_bf, &m.plan_bf_pair, &m.plan_f16, &m.plan_f16_pair};
    memcpy(dst, plans[which], sizeof(ac::MlpPlan));
}
void host_mlp_vplan(const void* h, int* dst) { memcpy(dst, &static_cast<const Built*>(h)->m.vplan, sizeof(ac::ValuPlan)); }
// dst: wt, use_mfma, has_bf, f16_gate, has_rev, rev_layers, has_vplan, vwidth, folded layer count
void host_mlp_scalars(const void* h, int* dst) {
    const ac::MlpModel& m = static_cast<const Built*>(h)->m;
    const int v[9] = {m.wt, m.use_mfma, m.has_bf, m.f16_gate, m.has_rev, m.rev_layers, m.has_vplan, m.vwidth, (int)m.W.size()};
    memcpy(dst, v, sizeof(v));
}
long host_mlp_blob(const void* h, const float** p) {
    const ac::MlpModel& m = static_cast<const Built*>(h)->m;
    *p = m.blob.data();
    return (long)m.blob.size();
}
long host_mlp_vimage(const void* h, const float** p) {
    const ac::MlpModel& m = static_cast<const Built*>(h)->m;
    *p = m.vimage.data();
    return (long)m.vimage.size();
}
// the folded net: widths [layers + 1], act [layers]; W, b of layer l
void host_mlp_folded_shape(const void* h, int* widths, int* act) {
    const ac::MlpModel& m = static_cast<const Built*>(h)->m;
    memcpy(widths, m.widths.data(), m.widths.size() * sizeof(int));
    memcpy(act, m.act.data(), m.act.size() * sizeof(int));
}
const float* host_mlp_folded_W(const void* h, int l) { return static_cast<const Built*>(h)->m.W[(size_t)l].data(); }
const float* host_mlp_folded_b(const void* h, int l) { return static_cast<const Built*>(h)->m.b[(size_t)l].data(); }

// plan_lds on a caller's plan (an array of host_mlp_plan_ints() ints, planned in place)
int host_mlp_plan_lds(int* plan, int force_stream, char* err, int errlen) {
    return ac::plan_lds(*reinterpret_cast<ac::MlpPlan*>(plan), force_stream != 0, err, (size_t)errlen);
}

// the stand-alone packers and gate, for comparison with the regions of the blob
int host_mlp_bf16_layer_bytes(int wt) { return ac::bf16_layer_bytes(wt); }
int host_mlp_f16_layer_bytes(int wt) { return ac::f16_layer_bytes(wt); }
void host_mlp_bf16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) { ac::bf16_pack_layer(W, b, nin, nout, wt, dst); }
void host_mlp_f16_pack_layer(const float* W, const float* b, int nin, int nout, int wt, void* dst) { ac::f16_pack_layer(W, b, nin, nout, wt, dst); }
int host_mlp_f16_gate(int n_layers, const int* widths, const float* const* W, const float* const* b) {
    return ac::f16_gate(n_layers, widths, W, b);
}
}
