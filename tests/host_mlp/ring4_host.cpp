// Host view of the four-region weight ring of the one-wave f16 sensitivity kernel (aircraft_amd/csrc/ac_mlp_plan.hpp) for
// tests/test_f16_ring4_host.py.  Built into one library with mlp_model_host.cpp, whose host_mlp_plan() hands out the plans.
#include "../../aircraft_amd/csrc/ac_mlp_model.hpp"

extern "C" {
int host_ring4_front_bytes(int wt) { return ac::f16_front_bytes(wt); }
int host_ring4_layer_bytes(int wt) { return ac::f16_layer_bytes(wt); }
// plan: host_mlp_plan_ints() ints (plan_f16)
int host_ring4_lds(const int* plan, int front_bytes) { return ac::f16_ring4_lds(*reinterpret_cast<const ac::MlpPlan*>(plan), front_bytes); }
int host_ring4_slot(const int* plan, int k) { return ac::f16_ring4_slot(*reinterpret_cast<const ac::MlpPlan*>(plan), k); }
// what the dispatcher reads: MlpModelInfo::f16_ring4_lds of a net (arguments as host_mlp_build); < 0: the build's error code
int host_ring4_of_net(int n_layers, const int* widths, const int* act, const float* const* W, const float* const* b) {
    ac::MlpModel m;
    char err[256];
    const int rc = ac::build_mlp_model(n_layers, widths, act, W, b, 1, m, err, sizeof(err));
    return rc == AC_OK ? m.f16_ring4_lds : rc;
}
// out: read_slot, next_layer, next_slot, snext
void host_ring4_step(const int* plan, int ring_pos, int snext, int* out) {
    const ac::Ring4Step s = ac::f16_ring4_step(*reinterpret_cast<const ac::MlpPlan*>(plan), ring_pos, snext);
    out[0] = s.read_slot; out[1] = s.next_layer; out[2] = s.next_slot; out[3] = s.snext;
}
}
