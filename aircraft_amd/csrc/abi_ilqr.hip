// abi_ilqr.hip — the solver side: trajectory costs and selection, the Riccati backward pass in all its forms, costate, goal loss,
// control-rate terms, multiple shooting, track and progress terms, and the closed-loop rollout.
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include <cmath>
#include <cstring>
#include <vector>

#include "ac_abi.hpp"
#include "ac_goal.hpp"
#include "ac_ilqr.hpp"
#include "ac_ilqr_rate.hpp"
#include "ac_nn_decl.hpp"
#include "ac_select.hpp"
#include "ac_shoot.hpp"
#include "ac_track.hpp"

using namespace ac;

namespace ac {
// Trajectory cost for the random-restart driver: X [H+1][13][B] -> cost [B]
__global__ __launch_bounds__(kBlock) void k_traj_cost(const float* __restrict__ X, long B, long H, float gx, float gy,
                                                      float gz, float w_track, float w_goal,
                                                      float* __restrict__ cost) {
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B) return;
    float acc = 0.f, last = 0.f;
    for (long k = 0; k <= H; ++k) {
        const float* xk = X + k * 13 * B;
        const float dx = xk[i] - gx, dy = xk[B + i] - gy, dz = xk[2 * B + i] - gz;
        last = dx * dx + dy * dy + dz * dz;
        acc += last;
    }
    cost[i] = w_track * acc + w_goal * last;
}

}  // namespace ac

extern "C" {

int ac_traj_cost_f32(ac_handle* h, const float* X, long B, long H, const float* goal3, float w_track, float w_goal,
                     float* cost, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !X || !goal3 || !cost || B < 0 || H < 0) return AC_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_traj_cost, grid, kBlock, 0, st, X, B, H, goal3[0], goal3[1], goal3[2], w_track, w_goal, cost);
    note_launch(h, "k_traj_cost", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_best_records_f32(ac_handle* h, const float* cost, const float* X, const float* U, long B, long H, int K,
                        float* rec, void* stream) {
    AC_ENTER(h);
    if (!h || K < 0 || B < 0 || H < 0) return AC_ERR_BAD_ARG;
    if (K == 0) return AC_OK;
    if (!cost || !X || !rec || (H > 0 && !U)) return AC_ERR_BAD_ARG;
    if (K > kMaxBestK) return fail(AC_ERR_BAD_ARG, "ac_best_records_f32: K > 8");
    if (K > B) return fail(AC_ERR_BAD_ARG, "ac_best_records_f32: K exceeds the number of instances");
    hipLaunchKernelGGL(k_best_records, K, kSelBlock, 0, (hipStream_t)stream, cost, X, U, B, H, K, rec);
    note_launch(h, "k_best_records", K, kSelBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_merge_records_f32(ac_handle* h, const float* rec_in, long n, long R, float* rec_out, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || R < 1) return AC_ERR_BAD_ARG;
    if (n == 0) return AC_OK;
    if (!rec_in || !rec_out || rec_in == rec_out) return AC_ERR_BAD_ARG;
    if (n > 1024) return fail(AC_ERR_BAD_ARG, "ac_merge_records_f32: more than 1024 rows");
    hipLaunchKernelGGL(k_merge_records, (int)n, 256, 0, (hipStream_t)stream, rec_in, n, R, rec_out);
    note_launch(h, "k_merge_records", (int)n, 256, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_ilqr_accept_f32(ac_handle* h, const float* Jc, const float* J0, const float* Xc, const float* Uc, int n_alpha,
                       long B, long H, float* X, float* U, float* Jout, unsigned char* improved, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !Jc || !J0 || !Xc || !X || !Jout || (H > 0 && (!Uc || !U)) || n_alpha < 1 || n_alpha > 8 || B < 0 || H < 0)
        return AC_ERR_BAD_ARG;
    // Jout is written by the row-0 workgroups while the others still read J0 and Jc to decide whether to copy: an aliased
    // Jout tears the iterate
    if (Jout == J0 || (Jout >= Jc && Jout < Jc + (long)n_alpha * B) || (Jc >= Jout && Jc < Jout + B))
        return fail(AC_ERR_BAD_ARG, "ac_ilqr_accept_f32: Jout must not alias J0 or Jc");
    const long nrows = (H + 1) * 13 + H * 7;
    dim3 grid((unsigned)((B + 255) / 256), (unsigned)((nrows + kAcceptRows - 1) / kAcceptRows));
    hipLaunchKernelGGL(k_ilqr_accept, grid, 256, 0, (hipStream_t)stream, Jc, J0, Xc, Uc, n_alpha, B, H, X, U, Jout, improved);
    note_launch(h, "k_ilqr_accept", (int)grid.x, 256, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

static IlqrCost to_dev_cost(const ac_ilqr_cost* c) {
    IlqrCost d;
    static_assert(sizeof(IlqrCost) == sizeof(ac_ilqr_cost), "ac_ilqr_cost layout");
    memcpy(&d, c, sizeof(d));
    return d;
}

static bool box_ok(const ac_ilqr_cost* c) {
    for (int i = 0; i < 7; ++i) {
        const float lo = c->u_min[i], hi = c->u_max[i];
        if (!(fabsf(lo) <= 3.4028235e38f) || !(fabsf(hi) <= 3.4028235e38f) || lo > hi) return false;
    }
    return true;
}

// ---- the Riccati backward pass (ac_ilqr.hpp, ac_ilqr_rate.hpp, ac_boxqp.hpp): every entry point fills IlqrBackwardArgs, then ONE
// validation and ONE launcher (ilqr_backward_inst.hip: all 24 kernels) ----------------------------------------------------------
static IlqrBackwardArgs backward_args(const float* node_q, const float* node_xref, const float* node_glin, const float* node_uglin,
                                      const float* Hz, const float* X, const float* U, const float* A, const float* Bm, long B,
                                      long H, float* K, float* kff, float* dV) {
    IlqrBackwardArgs a{};  // (C is filled in by backward_run, once the cost is known to be there)
    a.N = NodeCost{node_q, node_xref, node_glin, B, node_uglin};
    a.X = X, a.U = U, a.A = A, a.Bm = Bm, a.Hz = Hz;
    a.B = B, a.H = H;
    a.K = K, a.kff = kff, a.dV = dV;
    return a;
}

// `extra`: the arrays this entry point cannot do without beyond X, U, A, Bm, K, kff, dV are all there; `name`: what the launch
// is noted under.  The rules of every entry point: the node arrays go together, node_uglin needs them and Hz, Vx and Vxx go
// together, a box has finite bounds with u_min <= u_max.
static int backward_run(ac_handle* h, const ac_ilqr_cost* cost, IlqrBackwardArgs& a, bool extra, const char* name, void* stream) {
    AC_ENTER(h);
    if (h && a.B == 0) return AC_OK;
    if (!h || !cost || !extra || !a.X || !a.U || !a.A || !a.Bm || !a.K || !a.kff || !a.dV || a.B < 0 || a.H < 1) return AC_ERR_BAD_ARG;
    const NodeCost& n = a.N;
    if ((n.q || n.xref || n.glin) && !(n.q && n.xref && n.glin)) return AC_ERR_BAD_ARG;
    if (n.uglin && !(n.q && a.Hz)) return AC_ERR_BAD_ARG;
    if ((a.Vx != nullptr) != (a.Vxx != nullptr)) return fail(AC_ERR_BAD_ARG, "ac_ilqr_backward_shoot_f32: Vx and Vxx go together");
    if (a.box && !box_ok(cost)) return AC_ERR_BAD_ARG;
    a.C = to_dev_cost(cost);
    AC_HIP(ilqr_launch_backward(a, (hipStream_t)stream));
    note_launch(h, name, (int)a.B, 64, 0);  // one wave per instance
    return AC_OK;
}

int ac_ilqr_backward_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* X, const float* U, const float* A,
                         const float* Bm, long B, long H, float* K, float* kff, float* dV, void* stream) {
    return ac_ilqr_backward_node_f32(h, cost, nullptr, nullptr, nullptr, X, U, A, Bm, B, H, K, kff, dV, stream);
}

int ac_ilqr_backward_node_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* X, const float* U, const float* A, const float* Bm,
                              long B, long H, float* K, float* kff, float* dV, void* stream) {
    return ac_ilqr_backward_newton_f32(h, cost, node_q, node_xref, node_glin, nullptr, X, U, A, Bm, B, H, K, kff, dV,
                                       stream);
}

int ac_ilqr_costate_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                        const float* node_glin, const float* X, const float* A, long B, long H, float* Lam,
                        void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !cost || !X || !A || !Lam || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if ((node_q || node_xref || node_glin) && !(node_q && node_xref && node_glin)) return AC_ERR_BAD_ARG;
    const NodeCost nc{node_q, node_xref, node_glin, B};
    const int grid = (int)((B + kBlock - 1) / kBlock);
    if (node_q) hipLaunchKernelGGL(k_ilqr_costate<true>, grid, kBlock, 0, (hipStream_t)stream, to_dev_cost(cost), nc, X, A, B, H, Lam);
    else hipLaunchKernelGGL(k_ilqr_costate<false>, grid, kBlock, 0, (hipStream_t)stream, to_dev_cost(cost), nc, X, A, B, H, Lam);
    note_launch(h, "k_ilqr_costate", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_ilqr_backward_newton_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                                const float* node_glin, const float* Hz, const float* X, const float* U, const float* A,
                                const float* Bm, long B, long H, float* K, float* kff, float* dV, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, nullptr, Hz, X, U, A, Bm, B, H, K, kff, dV);
    return backward_run(h, cost, a, true, "k_ilqr_backward", stream);
}

// ---- the goal-acquisition loss of the reference's MPC driver (main/control/control.py:44-68; ac_goal.hpp) ----------------
static GoalLoss to_dev_goal(const ac_goal_loss* g) {
    GoalLoss d;
    static_assert(sizeof(GoalLoss) == sizeof(ac_goal_loss), "ac_goal_loss layout");
    memcpy(&d, g, sizeof(d));
    return d;
}

int ac_goal_cost_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, long Bn, const float* X,
                     const float* U, long B, long H, float* cost_inout, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !loss || !goal || !X || !U || !cost_inout || B < 0 || H < 1 || Bn < 1 || B % Bn != 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_goal_cost<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_goal(loss), goal, lam, Bn, X, U, B, H,
                       cost_inout);
    note_launch(h, "k_goal_cost", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_goal_model_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, const float* X,
                      const float* U, long B, long H, float* node_q, float* node_xref, float* node_glin, float* node_uglin,
                      float* Hz, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !loss || !goal || !X || !U || !node_q || !node_xref || !node_glin || !node_uglin || B < 0 || H < 1)
        return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const long n = (H + 1) * B;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_goal_model<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_goal(loss), goal, lam, X, U, B, H,
                       node_q, node_xref, node_glin, node_uglin, Hz);
    note_launch(h, "k_goal_model", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_goal_multiplier_f32(ac_handle* h, const ac_goal_loss* loss, const float* X, long B, long H, float* lam, float* viol,
                           void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !loss || !X || !lam || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_goal_multiplier<0>, grid, kBlock, 0, (hipStream_t)stream, to_dev_goal(loss), X, B, H, lam, viol);
    note_launch(h, "k_goal_multiplier", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_ilqr_backward_goal_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* node_uglin, const float* Hz, const float* X,
                              const float* U, const float* A, const float* Bm, long B, long H, float* K, float* kff,
                              float* dV, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, node_uglin, Hz, X, U, A, Bm, B, H, K, kff, dV);
    return backward_run(h, cost, a, node_q && node_xref && node_glin && Hz, "k_ilqr_backward", stream);  // always <true, true>
}

// ---- the control-rate term modelled exactly: u_{k-1} carried through the Riccati pass (ac_ilqr_rate.hpp) -------------------
int ac_ilqr_backward_rate_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* Hz, const float* rate_g, const float* rate_h, const float* X,
                              const float* U, const float* A, const float* Bm, long B, long H, float* K, float* Kp, float* kff,
                              float* dV, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, nullptr, Hz, X, U, A, Bm, B, H, K, kff, dV);
    a.rate_g = rate_g, a.rate_h = rate_h, a.Kp = Kp;
    return backward_run(h, cost, a, rate_g && rate_h && Kp, "k_ilqr_backward_rate", stream);
}

// ---- the control box in the backward pass: a 7-variable QP per node (ac_boxqp.hpp; the BOX kernels) ------------------------------
int ac_ilqr_backward_box_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                             const float* node_glin, const float* node_uglin, const float* Hz, const float* X, const float* U,
                             const float* A, const float* Bm, long B, long H, float* K, float* kff, float* dV, signed char* act,
                             int* stat, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, node_uglin, Hz, X, U, A, Bm, B, H, K, kff, dV);
    a.box = true, a.act = act, a.stat = stat;
    return backward_run(h, cost, a, true, "k_ilqr_backward_box", stream);
}

int ac_ilqr_backward_rate_box_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                                  const float* node_glin, const float* Hz, const float* rate_g, const float* rate_h,
                                  const float* X, const float* U, const float* A, const float* Bm, long B, long H, float* K,
                                  float* Kp, float* kff, float* dV, signed char* act, int* stat, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, nullptr, Hz, X, U, A, Bm, B, H, K, kff, dV);
    a.rate_g = rate_g, a.rate_h = rate_h, a.Kp = Kp;
    a.box = true, a.act = act, a.stat = stat;
    return backward_run(h, cost, a, rate_g && rate_h && Kp, "k_ilqr_backward_rate_box", stream);
}

// ---- Gauss-Newton multiple shooting: the defects in the Riccati pass, direction, candidates, merit (ac_shoot.hpp) -------------
int ac_ilqr_backward_shoot_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                               const float* node_glin, const float* node_uglin, const float* Hz, const float* X, const float* U,
                               const float* A, const float* Bm, const float* F, long B, long H, float* K, float* kff, float* dV,
                               float* Vx, float* Vxx, int box, signed char* act, int* stat, void* stream) {
    IlqrBackwardArgs a = backward_args(node_q, node_xref, node_glin, node_uglin, Hz, X, U, A, Bm, B, H, K, kff, dV);
    a.F = F, a.Vx = Vx, a.Vxx = Vxx;
    a.box = box != 0, a.act = act, a.stat = stat;
    return backward_run(h, cost, a, F != nullptr, box ? "k_ilqr_backward_shoot_box" : "k_ilqr_backward_shoot", stream);
}

int ac_shoot_direction_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X, const float* U, const float* F, const float* A,
                           const float* Bm, const float* K, const float* kff, const float* Vx, const float* Vxx, long B, long H,
                           float* dX, float* dU, float* Lam, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !X || !F || !A || !Bm || !K || !kff || !dX || !dU || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if ((Vx != nullptr) != (Vxx != nullptr)) return fail(AC_ERR_BAD_ARG, "ac_shoot_direction_f32: Vx and Vxx go together");
    if (Lam && !Vx) return fail(AC_ERR_BAD_ARG, "ac_shoot_direction_f32: Lam needs Vx and Vxx");
    if (limits && (!U || !box_ok(limits))) return fail(AC_ERR_BAD_ARG, "ac_shoot_direction_f32: limits need U and finite bounds, u_min <= u_max");
    IlqrCost lim;
    memset(&lim, 0, sizeof(lim));
    if (limits) lim = to_dev_cost(limits);
    int grid = 0;
    AC_HIP(shoot_launch_direction(lim, limits != nullptr, X, U, F, A, Bm, K, kff, Vx, Vxx, B, H, dX, dU, Vx ? Lam : nullptr,
                                  (hipStream_t)stream, &grid));
    note_launch(h, "k_shoot_direction", grid, 64, 0);
    return AC_OK;
}

int ac_shoot_merit_weight_f32(ac_handle* h, const float* Lam, float factor, long B, long H, float* mu, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !Lam || !mu || B < 0 || H < 1 || !(factor >= 0.f) || !(factor <= 3.4028235e38f)) return AC_ERR_BAD_ARG;
    int grid = 0;
    AC_HIP(shoot_launch_merit_weight(Lam, factor, B, H, mu, (hipStream_t)stream, &grid));
    note_launch(h, "k_shoot_merit_weight", grid, kBlock, 0);
    return AC_OK;
}

int ac_shoot_candidates_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X, const float* U, const float* dX,
                            const float* dU, const float* alphas, int n_alpha, long B, long H, float* Xc, float* Uc, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !limits || !X || !U || !dX || !dU || !alphas || !Xc || !Uc || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if (n_alpha < 1 || n_alpha > 8) return AC_ERR_BAD_ARG;
    AlphaSet al;
    al.n = n_alpha;
    for (int i = 0; i < 8; ++i) al.a[i] = i < n_alpha ? alphas[i] : 0.f;
    int grid = 0;
    AC_HIP(shoot_launch_candidates(to_dev_cost(limits), X, U, dX, dU, al, B, H, Xc, Uc, (hipStream_t)stream, &grid));
    note_launch(h, "k_shoot_candidates", grid, kBlock, 0);
    return AC_OK;
}

int ac_shoot_merit_f32(ac_handle* h, const float* J, const float* mu, long Bn, const float* R, const float* F, const float* X,
                       long B, long H, float* phi, float* defect_inf, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !J || !mu || !phi || !defect_inf || B < 0 || H < 1 || Bn < 1 || B % Bn != 0) return AC_ERR_BAD_ARG;
    if (!R && !(F && X)) return fail(AC_ERR_BAD_ARG, "ac_shoot_merit_f32: R, or F and X");
    if (!R && Bn != B) return fail(AC_ERR_BAD_ARG, "ac_shoot_merit_f32: the (F, X) form is the iterate's: Bn == B");
    int grid = 0;
    AC_HIP(shoot_launch_merit(J, mu, Bn, R, F, X, B, H, phi, defect_inf, (hipStream_t)stream, &grid));
    note_launch(h, "k_shoot_merit", grid, kBlock, 0);
    return AC_OK;
}

int ac_goal_model_rate_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, const float* X,
                           const float* U, long B, long H, float* node_q, float* node_xref, float* node_glin, float* rate_g,
                           float* rate_h, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !loss || !goal || !X || !U || !node_q || !node_xref || !node_glin || !rate_g || !rate_h || B < 0 || H < 1)
        return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const long n = (H + 1) * B;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_goal_model<0, true>), grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_goal(loss), goal, lam, X, U, B,
                       H, node_q, node_xref, node_glin, rate_g, rate_h);
    note_launch(h, "k_goal_model_rate", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

static bool rate_weights(const float* w, RateWeights* out) {
    for (int i = 0; i < 7; ++i) {
        if (!(w[i] >= 0.f) || !(w[i] <= 3.4028235e38f)) return false;
        out->w[i] = w[i];
    }
    return true;
}

int ac_ilqr_rate_model_f32(ac_handle* h, const float* rate_weight, const float* U, const float* u_prev, long B, long H,
                           float* rate_g, float* rate_h, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !rate_weight || !U || !rate_g || !rate_h || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    RateWeights W;
    if (!rate_weights(rate_weight, &W)) return fail(AC_ERR_BAD_ARG, "ac_ilqr_rate_model_f32: rate weights must be finite and >= 0");
    int grid = 0;
    AC_HIP(ilqr_rate_launch_model(W, U, u_prev, B, H, rate_g, rate_h, (hipStream_t)stream, &grid));
    note_launch(h, "k_ilqr_rate_model", grid, kBlock, 0);
    return AC_OK;
}

int ac_ilqr_rate_cost_f32(ac_handle* h, const float* rate_weight, const float* u_prev, long Bn, const float* U, long B, long H,
                          float* cost_inout, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !rate_weight || !U || !cost_inout || B < 0 || H < 1 || Bn < 1 || B % Bn != 0) return AC_ERR_BAD_ARG;
    RateWeights W;
    if (!rate_weights(rate_weight, &W)) return fail(AC_ERR_BAD_ARG, "ac_ilqr_rate_cost_f32: rate weights must be finite and >= 0");
    int grid = 0;
    AC_HIP(ilqr_rate_launch_cost(W, U, u_prev, Bn, B, H, cost_inout, (hipStream_t)stream, &grid));
    note_launch(h, "k_ilqr_rate_cost", grid, kBlock, 0);
    return AC_OK;
}

int ac_ilqr_cost_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* X, const float* U, long B, long H,
                     float* out, void* stream) {
    return ac_ilqr_cost_node_f32(h, cost, nullptr, nullptr, nullptr, B, X, U, B, H, out, stream);
}

int ac_ilqr_cost_node_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                          const float* node_glin, long Bn, const float* X, const float* U, long B, long H, float* out,
                          void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !cost || !X || !U || !out || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if ((node_q || node_xref || node_glin) && !(node_q && node_xref && node_glin && Bn > 0)) return AC_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    const NodeCost nc{node_q, node_xref, node_glin, Bn > 0 ? Bn : 1};
    if (node_q) hipLaunchKernelGGL(k_ilqr_cost<true>, grid, kBlock, 0, st, to_dev_cost(cost), nc, X, U, B, H, out);
    else hipLaunchKernelGGL(k_ilqr_cost<false>, grid, kBlock, 0, st, to_dev_cost(cost), nc, X, U, B, H, out);
    note_launch(h, "k_ilqr_cost", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// ---- track + progress terms -------------------------------------------------------------------------
int ac_set_track(ac_handle* h, int n_segments, const float* coef, float length) {
    if (!h || !coef || n_segments < 1 || !(length > 0.f)) return AC_ERR_BAD_ARG;
    AC_ENTER(h);
    if (h->d_track) { (void)hipFree(h->d_track); h->d_track = nullptr; }
    memset(&h->track, 0, sizeof(h->track));  // no dangling device pointer if anything below fails
    // [nseg][3][4] cubics, then one flag per knot: is the knot's float64 value (numpy linspace(0, 1, nseg + 1): i * step, the
    // last one exactly 1) representable in fp32?  Only such a knot can be hit EXACTLY by an fp32 progress value — where the
    // reference's closed segment intervals count the point twice (track_eval, ac_track.hpp).
    std::vector<float> img((size_t)n_segments * 12 + (size_t)n_segments + 1);
    memcpy(img.data(), coef, (size_t)n_segments * 12 * sizeof(float));
    const double step = 1.0 / (double)n_segments;
    for (int i = 0; i <= n_segments; ++i) {
        const double si = (i == n_segments) ? 1.0 : (double)i * step;
        img[(size_t)n_segments * 12 + (size_t)i] = ((double)(float)si == si) ? 1.f : 0.f;
    }
    const size_t bytes = img.size() * sizeof(float);
    {
        hipError_t e = hipMalloc((void**)&h->d_track, bytes);
        if (e != hipSuccess) { h->d_track = nullptr; return hip_fail(e, "hipMalloc(track)"); }
        e = hipMemcpy(h->d_track, img.data(), bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(h->d_track); h->d_track = nullptr; return hip_fail(e, "hipMemcpy(track)"); }
    }
    h->track.coef = h->d_track;
    h->track.knot_exact = h->d_track + (size_t)n_segments * 12;
    h->track.nseg = n_segments;
    h->track.inv_length = 1.f / length;
    const float* last = coef + (size_t)(n_segments - 1) * 12;
    for (int a = 0; a < 3; ++a) h->track.end_pos[a] = last[a * 4] + last[a * 4 + 1] + last[a * 4 + 2] + last[a * 4 + 3];
    return AC_OK;
}

int ac_track_eval_f32(ac_handle* h, const float* s, long n, float* pos, float* tangent, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !s || !pos || !tangent || n < 0) return AC_ERR_BAD_ARG;
    if (!h->d_track) return AC_ERR_NO_MODEL;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_track_eval, grid, kBlock, 0, (hipStream_t)stream, h->track, s, n, pos, tangent);
    note_launch(h, "k_track_eval", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

static MhttWeights to_dev_weights(const ac_mhtt_weights* w) {
    MhttWeights d{};
    static_assert(sizeof(MhttWeights) == sizeof(ac_mhtt_weights), "ac_mhtt_weights layout");
    if (w) memcpy(&d, w, sizeof(d));
    return d;
}

int ac_track_progress_f32(ac_handle* h, const ac_mhtt_weights* weights, const float* X, const float* s0, float dt,
                          long B, long H, int mode, float* S, float* s_dot, float* track_err, float* node_q,
                          float* node_xref, float* node_glin, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !X || !s0 || !S || B < 0 || H < 1 || (mode != 0 && mode != 1)) return AC_ERR_BAD_ARG;
    const bool any = node_q || node_xref || node_glin;
    if (any && !(node_q && node_xref && node_glin && weights)) return AC_ERR_BAD_ARG;
    if (!h->d_track) return AC_ERR_NO_MODEL;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_track_progress, grid, kBlock, 0, (hipStream_t)stream, h->track, to_dev_weights(weights), X, s0,
                       dt, B, H, mode, S, s_dot, track_err, node_q, node_xref, node_glin);
    note_launch(h, "k_track_progress", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_mhtt_loss_f32(ac_handle* h, const ac_mhtt_weights* weights, const float* X, const float* U, const float* S,
                     long B, long H, float* J, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !weights || !X || !U || !S || !J || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if (!h->d_track) return AC_ERR_NO_MODEL;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_mhtt_loss, grid, kBlock, 0, (hipStream_t)stream, h->track, to_dev_weights(weights), X, U, S, B,
                       H, J);
    note_launch(h, "k_mhtt_loss", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// the two closed-loop entries; Kp == nullptr: the law without the previous-control term (ac_rollout_policy_f32)
static int rollout_policy(ac_handle* h, const ac_ilqr_cost* limits, const float* X0, const float* Xnom, const float* U,
                          const float* K, const float* Kp, const float* kff, const float* alphas, int n_alpha, float dt, long B,
                          long H, float* Xout, float* Uout, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !limits || !X0 || !Xnom || !U || !K || !kff || !alphas || !Xout || !Uout || B < 0 || H < 1) return AC_ERR_BAD_ARG;
    if (n_alpha < 1 || n_alpha > 8) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    Policy pol;
    pol.Xnom = Xnom; pol.U = U; pol.K = K; pol.kff = kff; pol.B = B; pol.Kp = Kp;
    pol.alphas.n = n_alpha;
    for (int i = 0; i < 8; ++i) pol.alphas.a[i] = i < n_alpha ? alphas[i] : 0.f;
    memcpy(pol.u_min, limits->u_min, sizeof(pol.u_min));
    memcpy(pol.u_max, limits->u_max, sizeof(pol.u_max));
    pol.dt_row = limits->dt_row;
    if (pol.dt_row >= 7) return AC_ERR_BAD_ARG;
    if (pol.dt_row > 0) {
        // the time row must be one the force model ignores, and its box must keep dt positive
        const bool quad = h->dp.p.model_kind == AC_MODEL_QUAD;
        if (quad ? pol.dt_row < 4 : (pol.dt_row < 3 || pol.dt_row > 5)) return fail(AC_ERR_BAD_ARG, "dt_row must be a control row without effect (aircraft: 3-5, quadrotor: 4-6)");
        if (!(limits->u_min[pol.dt_row] > 0.f)) return fail(AC_ERR_BAD_ARG, "the time row's lower bound (dt_bounds[0]) must be > 0");
    }
    const long Bout = B * n_alpha;
    if (h->dp.p.model_kind == AC_MODEL_NN) {
        if (!h->use_mfma) {
            if (!h->has_vplan) return fail(AC_ERR_UNSUPPORTED, "policy rollout through the MLP with the MFMA path off needs hidden width 32 or 64");
            const long roll_units = h->vwidth == 64 ? kRolloutUnits<64> : kRolloutUnits<32>;
            const int grid = (int)((Bout + 4 * roll_units - 1) / (4 * roll_units));
            const int lds = h->vplan.image_floats * 4 + 4 * (int)roll_units * (h->vwidth + 4) * 4;
            return instance(pick<32, 64>(h->vwidth, [&](auto W) {
                return launch_kernel(h, st, "k_nn_rollout_policy_tiled8", k_nn_rollout_policy_tiled8<W()>, grid, kBlock, lds, h->dp,
                                 h->vplan, h->d_vblob, pol, X0, dt, Bout, H, Xout, Uout);
            }), kNoTiledInstance);
        }
        const int grid = (int)((Bout + 15) / 16);
        const int nh = h->plan.n_layers - 2;
        if (nh >= 1 && nh <= 3) {
            const int ldsr = 2 * h->wt * 1024;
            return instance(pick<2, 4, 8>(h->wt, [&](auto wt) {
                constexpr int WT = wt;
                return pick<1, 2, 3>(nh, [&](auto NH) {
                    return launch_kernel(h, st, "k_nn_rollout_policy_reg", k_nn_rollout_policy_reg<WT, NH()>, grid, kBlock, ldsr, h->dp,
                                     h->plan, h->d_blob, pol, X0, dt, Bout, H, Xout, Uout);
                });
            }), kNoNnInstance);
        }
        const int lds = h->plan.lds_total + h->wt * 1024;
        return instance(pick<2, 4, 8>(h->wt, [&](auto WT) {
            return launch_kernel(h, st, "k_nn_rollout_policy_coop", k_nn_rollout_policy_coop<WT(), true>, grid, kBlock, lds, h->dp,
                             h->plan, h->d_blob, pol, X0, dt, Bout, H, Xout, Uout);
        }), kNoNnInstance);
    }
    const int grid = (int)((Bout + 63) / 64);
    with_analytic_model(h, [&](auto M) { hipLaunchKernelGGL(k_rollout_policy<M()>, grid, 64, 0, st, h->dp, pol, X0, dt, Bout, H, Xout, Uout); });
    note_launch(h, "k_rollout_policy", grid, 64, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_rollout_policy_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X0, const float* Xnom, const float* U,
                          const float* K, const float* kff, const float* alphas, int n_alpha, float dt, long B, long H,
                          float* Xout, float* Uout, void* stream) {
    return rollout_policy(h, limits, X0, Xnom, U, K, nullptr, kff, alphas, n_alpha, dt, B, H, Xout, Uout, stream);
}

int ac_rollout_policy_rate_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X0, const float* Xnom, const float* U,
                               const float* K, const float* Kp, const float* kff, const float* alphas, int n_alpha, float dt,
                               long B, long H, float* Xout, float* Uout, void* stream) {
    if (h && B != 0 && !Kp) { AC_ENTER(h); return AC_ERR_BAD_ARG; }
    return rollout_policy(h, limits, X0, Xnom, U, K, Kp, kff, alphas, n_alpha, dt, B, H, Xout, Uout, stream);
}

}  // extern "C"
