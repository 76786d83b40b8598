// group_host.cpp — the column of the group Cholesky (aircraft_amd/csrc/ac_group.hpp) compiled for the HOST (g++,
// -DAC_HOST_CHECK -ffp-contract=off) behind a small C API, so that `pytest -m "not gpu"` measures its float32 arithmetic
// against float64 without a GPU.  The 16 lanes of a group run one after the other, phase by phase (GroupHost), as in the
// kernels that rest on them.  AC_GROUP_HEADER names the header (the tests also build mutated copies of it).
// TEST INFRASTRUCTURE: nothing in aircraft_amd loads this.
#define AC_HOST_CHECK 1
#ifndef AC_GROUP_HEADER
#define AC_GROUP_HEADER "../../aircraft_amd/csrc/ac_group.hpp"
#endif
#include AC_GROUP_HEADER

using namespace ac;

namespace {

struct GroupLane {
    float l[12], inv[12];
    bool bad[12];
};

}  // namespace

extern "C" {

// M [12][12] row-major -> L [12][12] (zero above the diagonal), inv [12] = 1 / L_jj and ok [12] (the pivot of column j was
// good).  -> 1 when the lanes of the group disagree on a pivot (they must not).
int host_group_chol(const float* M, float* L, float* inv, int* ok) {
    GroupHost<GroupLane, kGrpLanes> grp{};
    float m[kGrpLanes][kGrpLd] = {};
    grp.each([&](GroupLane&, int r) {
        for (int j = 0; j < 12; ++j) m[r][j] = M[(r < 12 ? r : 0) * 12 + j];  // the idle lanes repeat row 0, as in the kernels
    });
    for (int j = 0; j < 12; ++j) grp.each([&](GroupLane& G, int r) { grp_chol_column(m, G.l, r, j, G.inv[j], G.bad[j]); });
    int split = 0;
    for (int j = 0; j < 12; ++j) {
        inv[j] = grp.L[0].inv[j];
        ok[j] = grp.L[0].bad[j] ? 0 : 1;
        for (int r = 1; r < kGrpLanes; ++r)
            if (grp.L[r].bad[j] != grp.L[0].bad[j] || !(grp.L[r].inv[j] == grp.L[0].inv[j])) split = 1;
        for (int r = 0; r < 12; ++r) L[r * 12 + j] = j <= r ? grp.L[r].l[j] : 0.f;
    }
    return split;
}

}  // extern "C"
