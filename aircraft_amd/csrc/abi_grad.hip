// abi_grad.hip — reverse mode: vector-Jacobian products, and gradients to the surrogate's weights, to the coefficients of the
// cubic-fit and linear models, and to the airframe.
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include <algorithm>

#include "ac_abi.hpp"
#include "ac_agrad.hpp"
#include "ac_cgrad.hpp"
#include "ac_nn_decl.hpp"
#include "ac_vjp.hpp"
#include "ac_wgrad.hpp"

using namespace ac;

namespace {

// ---- reverse mode to parameters (ac_cgrad.hpp, ac_agrad.hpp): one recording sweep and one set of entry points; a descriptor
// says what is recorded ----------------------------------------------------------------------------------------------------------
int cgrad_floats_of(const ac_handle* h) {
    const int mk = h->dp.p.model_kind;
    return mk == AC_MODEL_POLY ? CgradFloats<AC_MODEL_POLY>::value : (mk == AC_MODEL_LINEAR ? CgradFloats<AC_MODEL_LINEAR>::value : 0);
}
// why the coefficient gradient cannot run on this handle (nullptr: it can); sets *code
const char* cgrad_refusal(const ac_handle* h, int* code) {
    *code = AC_ERR_UNSUPPORTED;
    if (!cgrad_floats_of(h)) return "coefficient gradients exist for the cubic-fit (poly) and the linear model only";
    if (model_ready(h) != AC_OK) { *code = AC_ERR_NO_MODEL; return "no coefficients installed: call ac_set_poly / ac_set_linear first"; }
    if (h->dp.p.substeps > kCgradMaxSubsteps)
        return "coefficient gradients: at most 30 RK4 sub-steps (240 + 13 sub-steps <= 640 words of LDS per lane)";
    return nullptr;
}
// why the airframe gradient cannot run on this handle (nullptr: it can); sets *code
const char* agrad_refusal(const ac_handle* h, int* code) {
    *code = AC_ERR_UNSUPPORTED;
    const int mk = h->dp.p.model_kind;
    if (mk == AC_MODEL_NN) return "airframe gradients: the MLP surrogate has no fused reverse sweep (default, linear and cubic-fit models only)";
    if (mk == AC_MODEL_QUAD) return "airframe gradients: the quadrotor's sweep is not recorded (default, linear and cubic-fit models only)";
    if (model_ready(h) != AC_OK) { *code = AC_ERR_NO_MODEL; return "no coefficients installed: call ac_set_poly / ac_set_linear first"; }
    if (h->dp.p.substeps > kAgradMaxSubsteps) return "airframe gradients: at most 40 RK4 sub-steps (the limit of the fused reverse sweep)";
    return nullptr;
}

// What a parameter gradient records: its refusal, the gradient length on this handle, the workspace message, and its kernels
// by model (with_model: pick over the models it is instantiated for).
struct CoefGrad {
    static constexpr auto refusal = cgrad_refusal;
    static int floats(const ac_handle* h) { return cgrad_floats_of(h); }
    static constexpr const char* kWorkspace = "coefficient-gradient workspace too small: see ac_cgrad_workspace_floats";
    static constexpr const char* kStep = "k_step_cgrad";
    static constexpr const char* kRollout = "k_rollout_cgrad";
    template <class F> static int with_model(const ac_handle* h, F&& f) {
        return instance(pick<AC_MODEL_LINEAR, AC_MODEL_POLY>(h->dp.p.model_kind, f), "no coefficient-gradient kernel for this model");
    }
    template <int M> static auto step_kernel() { return k_step_cgrad<M>; }
    template <int M> static auto rollout_kernel() { return k_rollout_cgrad<M>; }
};
struct AirframeGrad {
    static constexpr auto refusal = agrad_refusal;
    static int floats(const ac_handle*) { return kAgradFloats; }
    static constexpr const char* kWorkspace = "airframe-gradient workspace too small: see ac_agrad_workspace_floats";
    static constexpr const char* kStep = "k_step_agrad";
    static constexpr const char* kRollout = "k_rollout_agrad";
    template <class F> static int with_model(const ac_handle* h, F&& f) { return pick_fused_model(h, f); }
    template <int M> static auto step_kernel() { return k_step_agrad<M>; }
    template <int M> static auto rollout_kernel() { return k_rollout_agrad<M>; }
};

template <class D> int pgrad_lds_bytes(const ac_handle* h) {
    return cgrad_lane_words(D::floats(h), h->dp.p.substeps) * kVjpBlock * (int)sizeof(float);
}
// Workgroups of a launch over `units` lanes: one per tile of 64 up to the handle's cap — the CU count read at creation times
// the workgroups whose LDS fits one CU (at most 8), or ac_set_cgrad_grid's value.  Never the runtime's occupancy: the same
// inputs on the same handle give the same partials.
template <class D> int pgrad_grid_of(const ac_handle* h, long units) {
    const long tiles = (units + kVjpBlock - 1) / kVjpBlock;
    long cap = h->cgrad_grid;
    if (cap <= 0) {
        const long per_cu = std::max(1, std::min(8, 160 * 1024 / pgrad_lds_bytes<D>(h)));
        cap = (h->num_cus > 0 ? h->num_cus : 256) * per_cu;
    }
    return (int)std::max<long>(1, std::min(tiles, cap));
}

template <class D> int pgrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats) {
    if (!h || !floats || n_or_B < 0 || H < 0 || which < AC_CGRAD_STEP || which > AC_CGRAD_ROLLOUT) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    int code;
    if (const char* why = D::refusal(h, &code)) return fail(code, why);
    *floats = (size_t)pgrad_grid_of<D>(h, n_or_B) * (size_t)D::floats(h);
    return AC_OK;
}

// The sweep `kern` over `units` lanes with its partials in ws, then the F floats of the partials added in workgroup order
template <class D, class K, class... Args>
int pgrad_sweep(ac_handle* h, hipStream_t st, const char* name, K kern, long units, float* out, float* ws, size_t ws_floats,
                const Args&... args) {
    const int grid = pgrad_grid_of<D>(h, units), lds = pgrad_lds_bytes<D>(h), F = D::floats(h);
    if (!ws || ws_floats < (size_t)grid * (size_t)F) return fail(AC_ERR_WORKSPACE, D::kWorkspace);
    const int rc = D::with_model(h, [&](auto M) { return launch_kernel(h, st, name, kern(M), grid, kVjpBlock, lds, h->dp, args..., ws); });
    if (rc != AC_OK) return rc;
    hipLaunchKernelGGL(k_wgrad_reduce, (F + kBlock - 1) / kBlock, kBlock, 0, st, (const float*)ws, grid, F, out);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

template <class D>
int pgrad_step(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
               float* Xbar, float* Ubar, float* dtbar, float* out, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !out || n < 0 || (n > 0 && (!X || !U || !Lam))) return AC_ERR_BAD_ARG;
    int code;
    if (const char* why = D::refusal(h, &code)) return fail(code, why);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        AC_HIP(hipMemsetAsync(out, 0, (size_t)D::floats(h) * sizeof(float), st));
        return AC_OK;
    }
    return pgrad_sweep<D>(h, st, D::kStep, [](auto M) { return D::template step_kernel<M()>(); }, n, out, ws, ws_floats, X, U, dt,
                          dt_per_unit, Lam, n, Xbar, Ubar, dtbar);
}

template <class D>
int pgrad_rollout(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                  float* Ubar, float* dtbar, float* out, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !out || B < 0 || H < 0 || (B > 0 && (!Xtraj || !G || (H > 0 && !U)))) return AC_ERR_BAD_ARG;
    int code;
    if (const char* why = D::refusal(h, &code)) return fail(code, why);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || H == 0) {  // no step, no parameter enters; X[0] = x0: the cotangent passes through
        AC_HIP(hipMemsetAsync(out, 0, (size_t)D::floats(h) * sizeof(float), st));
        if (B > 0 && X0bar) AC_HIP(hipMemcpyAsync(X0bar, G, (size_t)B * 13 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (B > 0 && dtbar) AC_HIP(hipMemsetAsync(dtbar, 0, (size_t)B * sizeof(float), st));
        return AC_OK;
    }
    return pgrad_sweep<D>(h, st, D::kRollout, [](auto M) { return D::template rollout_kernel<M()>(); }, B, out, ws, ws_floats, Xtraj,
                          U, dt, B, H, G, X0bar, Ubar, dtbar);
}

}  // namespace

extern "C" {

// ---- reverse mode: vector-Jacobian products (ac_vjp.hpp) ----------------------------------------------------------------------
namespace {
// The route a VJP call of this handle takes: AC_VJP_FUSED, AC_VJP_COMPOSED, or AC_ERR_UNSUPPORTED (fused forced on a model
// that has no fused kernel, or more sub-steps than its LDS column holds).
int vjp_route_of(const ac_handle* h) {
    const int mk = h->dp.p.model_kind;
    const bool fusable = (mk == AC_MODEL_DEFAULT || mk == AC_MODEL_LINEAR || mk == AC_MODEL_POLY) &&
                         h->dp.p.substeps <= kVjpMaxSubsteps;
    if (h->vjp_route == AC_VJP_COMPOSED) return AC_VJP_COMPOSED;
    if (h->vjp_route == AC_VJP_FUSED) return fusable ? AC_VJP_FUSED : AC_ERR_UNSUPPORTED;
    return fusable ? AC_VJP_FUSED : AC_VJP_COMPOSED;
}
// floats per unit of the composed route's workspace: x+ (or x_dot), A (Fx), B (Fu) and, for the step, c
constexpr size_t kVjpStepWs = 13 + 169 + 91 + 13;
constexpr size_t kVjpDerivWs = 13 + 169 + 91;
size_t vjp_ws_floats(const ac_handle* h, int which, long n, long H) {
    if (vjp_route_of(h) != AC_VJP_COMPOSED) return 0;
    if (which == AC_VJP_ROLLOUT) return (size_t)n * (size_t)H * kVjpStepWs;
    return (size_t)n * (which == AC_VJP_DERIVATIVE ? kVjpDerivWs : kVjpStepWs);
}
int vjp_lds_bytes(const ac_handle* h) { return vjp_lane_words(h->dp.p.substeps) * kVjpBlock * (int)sizeof(float); }
// The composed route's contraction of n units:  Xbar = A' lam, Ubar = B' lam, dtbar = c . lam  (c, dtbar nullable)
int vjp_contract(ac_handle* h, hipStream_t st, const float* A, const float* Bm, const float* c, const float* Lam, long n,
                 float* Xbar, float* Ubar, float* dtbar) {
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_vjp_contract, grid, kBlock, 0, st, A, Bm, c, Lam, n, Xbar, Ubar, dtbar);
    note_launch(h, "k_vjp_contract", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}
// The composed route over a saved rollout: every (node, instance) pair is one unit of the multiple-shooting sensitivity kernels
// (x+, A, B, c into ws, kVjpStepWs floats per pair), then the reverse recurrence.  LamTraj (nullable) [H][13][B]: lambda_{k+1} per
// node, for the weight gradient.
int rollout_recur_composed(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G,
                           float* X0bar, float* Ubar, float* dtbar, float* LamTraj, float* ws, void* stream) {
    const size_t N = (size_t)B * (size_t)H;
    float* Xn = ws;
    float* A = Xn + 13 * N;
    float* Bm = A + 169 * N;
    float* c = Bm + 91 * N;
    const int rc = sens_impl(h, Xtraj, U, dt, nullptr, B * H, B, Xn, A, Bm, c, stream);
    if (rc != AC_OK) return rc;
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_vjp_recur, grid, kBlock, 0, (hipStream_t)stream, A, Bm, c, G, B, H, X0bar, Ubar, dtbar, LamTraj);
    note_launch(h, "k_vjp_recur", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}
}  // namespace

int ac_vjp_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats) {
    if (!h || !floats || n_or_B < 0 || H < 0 || which < AC_VJP_STEP || which > AC_VJP_DERIVATIVE) return AC_ERR_BAD_ARG;
    const int route = vjp_route_of(h);
    if (route < 0) return fail(route, "fused VJP route requested for a model without fused kernels (or too many sub-steps)");
    *floats = vjp_ws_floats(h, which, n_or_B, H);
    return AC_OK;
}

int ac_step_vjp_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                    float* Xbar, float* Ubar, float* dtbar, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Lam || !Xbar || !Ubar || n < 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const int route = vjp_route_of(h);
    if (route < 0) return fail(route, "fused VJP route requested for a model without fused kernels (or too many sub-steps)");
    hipStream_t st = (hipStream_t)stream;
    if (route == AC_VJP_FUSED) {
        const int grid = (int)((n + kVjpBlock - 1) / kVjpBlock);
        const int lds = vjp_lds_bytes(h);
        return pick_fused_model(h, [&](auto M) {
            return launch_kernel(h, st, "k_step_vjp", k_step_vjp<M()>, grid, kVjpBlock, lds, h->dp, X, U, dt, dt_per_unit, Lam, n, Xbar,
                                 Ubar, dtbar);
        });
    }
    const size_t N = (size_t)n;
    if (!ws || ws_floats < N * kVjpStepWs) return fail(AC_ERR_WORKSPACE, "VJP workspace too small: see ac_vjp_workspace_floats");
    float* Xn = ws;
    float* A = Xn + 13 * N;
    float* Bm = A + 169 * N;
    float* c = Bm + 91 * N;
    rc = sens_impl(h, X, U, dt, dt_per_unit, n, n, Xn, A, Bm, dtbar ? c : nullptr, stream);
    if (rc != AC_OK) return rc;
    return vjp_contract(h, st, A, Bm, dtbar ? c : nullptr, Lam, n, Xbar, Ubar, dtbar);
}

int ac_rollout_vjp_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                       float* Ubar, float* dtbar, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !Xtraj || !G || !X0bar || B < 0 || H < 0 || (H > 0 && (!U || !Ubar))) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const int route = vjp_route_of(h);
    if (route < 0) return fail(route, "fused VJP route requested for a model without fused kernels (or too many sub-steps)");
    hipStream_t st = (hipStream_t)stream;
    if (H == 0) {  // X[0] = x0: the cotangent passes through; dt does not enter
        AC_HIP(hipMemcpyAsync(X0bar, G, (size_t)B * 13 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (dtbar) AC_HIP(hipMemsetAsync(dtbar, 0, (size_t)B * sizeof(float), st));
        return AC_OK;
    }
    if (route == AC_VJP_FUSED) {
        const int grid = (int)((B + kVjpBlock - 1) / kVjpBlock);
        const int lds = vjp_lds_bytes(h);
        return pick_fused_model(h, [&](auto M) {
            return launch_kernel(h, st, "k_rollout_vjp", k_rollout_vjp<M()>, grid, kVjpBlock, lds, h->dp, Xtraj, U, dt, B, H, G, X0bar,
                                 Ubar, dtbar);
        });
    }
    if (!ws || ws_floats < (size_t)B * (size_t)H * kVjpStepWs)
        return fail(AC_ERR_WORKSPACE, "VJP workspace too small: see ac_vjp_workspace_floats");
    return rollout_recur_composed(h, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, nullptr, ws, stream);
}

int ac_state_derivative_vjp_f32(ac_handle* h, const float* X, const float* U, long n, const float* W, float* Xbar, float* Ubar,
                                float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !W || !Xbar || !Ubar || n < 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const int route = vjp_route_of(h);
    if (route < 0) return fail(route, "fused VJP route requested for a model without fused kernels (or too many sub-steps)");
    hipStream_t st = (hipStream_t)stream;
    if (route == AC_VJP_FUSED) {
        const int grid = (int)((n + kBlock - 1) / kBlock);
        return pick_fused_model(h, [&](auto M) {
            return launch_kernel(h, st, "k_deriv_vjp", k_deriv_vjp<M()>, grid, kBlock, 0, h->dp, X, U, W, n, Xbar, Ubar);
        });
    }
    const size_t N = (size_t)n;
    if (!ws || ws_floats < N * kVjpDerivWs) return fail(AC_ERR_WORKSPACE, "VJP workspace too small: see ac_vjp_workspace_floats");
    float* Xd = ws;
    float* Fx = Xd + 13 * N;
    float* Fu = Fx + 169 * N;
    rc = deriv_sens_impl(h, X, U, n, n, Xd, Fx, Fu, stream);
    if (rc != AC_OK) return rc;
    return vjp_contract(h, st, Fx, Fu, nullptr, W, n, Xbar, Ubar, nullptr);
}

// ---- reverse mode to the weights of the MLP surrogate (ac_wgrad.hpp) ----------------------------------------------------------
namespace {
// why the weight gradient cannot run on this handle (nullptr: it can); sets *code
const char* wgrad_refusal(const ac_handle* h, int* code) {
    *code = AC_ERR_UNSUPPORTED;
    if (h->dp.p.model_kind != AC_MODEL_NN) return "weight gradients exist for the MLP surrogate only (model_kind nn)";
    if (!h->has_mlp) { *code = AC_ERR_NO_MODEL; return "no MLP installed: call ac_set_mlp first"; }
    if (h->dp.p.substeps > 1) return "weight gradients run one RK4 sub-step (physical_integration_substeps = 1)";
    if (h->wg.act_last) return "weight gradients: tanh on the last layer is not supported";
    if (h->wg.n_layers - 2 > wgrad_max_hidden_products(h->wt))
        return "weight gradients: too many hidden-to-hidden layers for the accumulators of one workgroup (3 at width 128, 6 below)";
    return nullptr;
}
int wgrad_parts(const ac_handle* h, size_t units) {
    const size_t tiles = (4 * units + kWgSamples - 1) / kWgSamples, cus = h->num_cus > 0 ? (size_t)h->num_cus : 256;
    return (int)std::max<size_t>(1, std::min(tiles, cus));
}
// [stage table 144 n][Z 20 n][Ybar 24 n][partials]
size_t wgrad_seed_floats(size_t n) { return n * (size_t)kJacFloats; }
size_t wgrad_step_floats(const ac_handle* h, size_t n) {
    return wgrad_seed_floats(n) + 44 * n + (size_t)wgrad_parts(h, n) * (size_t)h->wg.grad_floats;
}
// rollout: [max(composed VJP workspace, step workspace) over the B H units][lambda 13 B H][X0bar 13 B][Ubar 7 B H][dtbar B]
size_t wgrad_rollout_head(const ac_handle* h, size_t N) { return std::max(N * kVjpStepWs, wgrad_step_floats(h, N)); }

int wgrad_seeds_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
                     const float* Lam, float* Z, float* Ybar, float* table, hipStream_t st) {
    const int grid_t = (int)((n + 63) / 64);
    const MlpPlan& plan = engine_plan(h);
    int rc = instance(pick_wt_mfma(h, [&](auto WT, auto MF) {
        return launch_kernel(h, st, "k_nn_stage_jac", k_nn_stage_jac<WT(), MF()>, grid_t, kBlock, plan.lds_total, h->dp, plan, h->d_blob,
                         X, U, dt, dt_per_unit, n, blk, table);
    }), kNoNnInstance);
    if (rc != AC_OK) return rc;
    const int grid = (int)((n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(k_wgrad_seeds, grid, kVjpBlock, 0, st, h->dp, X, U, dt, dt_per_unit, Lam, (const float*)table, n, blk, Z, Ybar);
    note_launch(h, "k_wgrad_seeds", grid, kVjpBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// seeds, weight gradient, reduction over n units; ws: wgrad_step_floats(h, n)
int wgrad_step_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
                    const float* Lam, float* Wbar, float* ws, hipStream_t st) {
    const size_t N = (size_t)n;
    float* table = ws;
    float* Z = table + wgrad_seed_floats(N);
    float* Ybar = Z + 20 * N;
    float* partial = Ybar + 24 * N;
    int rc = wgrad_seeds_impl(h, X, U, dt, dt_per_unit, n, blk, Lam, Z, Ybar, table, st);
    if (rc != AC_OK) return rc;
    const int parts = wgrad_parts(h, N), lds = wgrad_lds_bytes(h->wg.n_layers, h->wt);
    rc = instance(pick_wt_mfma(h, [&](auto WT, auto MF) {
        return launch_kernel(h, st, "k_mlp_wgrad", k_mlp_wgrad<WT(), MF()>, parts, kWgBlock, lds, h->wg, (const float*)h->d_wgimg,
                         (const float*)Z, (const float*)Ybar, n, 4 * n, partial);
    }), kNoNnInstance);
    if (rc != AC_OK) return rc;
    const int F = h->wg.grad_floats;
    hipLaunchKernelGGL(k_wgrad_reduce, (F + kBlock - 1) / kBlock, kBlock, 0, st, (const float*)partial, parts, F, Wbar);
    AC_HIP(hipGetLastError());
    return AC_OK;
}
}  // namespace

int ac_mlp_grad_floats(const ac_handle* h, size_t* floats) {
    if (!h || !floats) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    if (!h->has_mlp) return fail(AC_ERR_NO_MODEL, "no MLP installed: call ac_set_mlp first");
    *floats = (size_t)h->wg.grad_floats;
    return AC_OK;
}

int ac_wgrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats) {
    if (!h || !floats || n_or_B < 0 || H < 0 || which < AC_WGRAD_SEEDS || which > AC_WGRAD_ROLLOUT) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    int code;
    if (const char* why = wgrad_refusal(h, &code)) return fail(code, why);
    const size_t n = (size_t)n_or_B;
    if (which == AC_WGRAD_SEEDS) *floats = wgrad_seed_floats(n);
    else if (which == AC_WGRAD_STEP) *floats = wgrad_step_floats(h, n);
    else {
        const size_t N = n * (size_t)H;
        *floats = wgrad_rollout_head(h, N) + 13 * N + 13 * n + 7 * N + n;
    }
    return AC_OK;
}

int ac_step_wgrad_seeds_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n,
                            const float* Lam, float* Z, float* Ybar, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Lam || !Z || !Ybar || n < 0) return AC_ERR_BAD_ARG;
    int code;
    if (const char* why = wgrad_refusal(h, &code)) return fail(code, why);
    if (!ws || ws_floats < wgrad_seed_floats((size_t)n))
        return fail(AC_ERR_WORKSPACE, "weight-gradient workspace too small: see ac_wgrad_workspace_floats");
    return wgrad_seeds_impl(h, X, U, dt, dt_per_unit, n, n, Lam, Z, Ybar, ws, (hipStream_t)stream);
}

int ac_step_wgrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Wbar, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !Wbar || n < 0 || (n > 0 && (!X || !U || !Lam))) return AC_ERR_BAD_ARG;
    int code;
    if (const char* why = wgrad_refusal(h, &code)) return fail(code, why);
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        AC_HIP(hipMemsetAsync(Wbar, 0, (size_t)h->wg.grad_floats * sizeof(float), st));
        return AC_OK;
    }
    if (!ws || ws_floats < wgrad_step_floats(h, (size_t)n))
        return fail(AC_ERR_WORKSPACE, "weight-gradient workspace too small: see ac_wgrad_workspace_floats");
    return wgrad_step_impl(h, X, U, dt, dt_per_unit, n, n, Lam, Wbar, ws, st);
}

int ac_rollout_wgrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* Wbar,
                         float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !Wbar || B < 0 || H < 0 || (B > 0 && H > 0 && (!Xtraj || !U || !G))) return AC_ERR_BAD_ARG;
    int code;
    if (const char* why = wgrad_refusal(h, &code)) return fail(code, why);
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || H == 0) {  // no step, no weight enters
        AC_HIP(hipMemsetAsync(Wbar, 0, (size_t)h->wg.grad_floats * sizeof(float), st));
        return AC_OK;
    }
    const size_t Bs = (size_t)B, N = Bs * (size_t)H, head = wgrad_rollout_head(h, N);
    if (!ws || ws_floats < head + 13 * N + 13 * Bs + 7 * N + Bs)
        return fail(AC_ERR_WORKSPACE, "weight-gradient workspace too small: see ac_wgrad_workspace_floats");
    float* lam = ws + head;
    float* X0bar = lam + 13 * N;
    float* Ubar = X0bar + 13 * Bs;
    float* dtbar = Ubar + 7 * N;
    // the reverse recurrence of the composed VJP route, with lambda_{k+1} kept per node
    const int rc = rollout_recur_composed(h, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, lam, ws, stream);
    if (rc != AC_OK) return rc;
    // (the Jacobians are consumed: the step gradient's buffers reuse their place)
    return wgrad_step_impl(h, Xtraj, U, dt, nullptr, B * H, B, lam, Wbar, ws, st);
}

// ---- reverse mode to parameters: the coefficients of the cubic-fit and the linear model (ac_cgrad.hpp), and mass, inertia,
// inertia_inv and com (ac_agrad.hpp): the pgrad_* functions above with their descriptor ----------------------------------------
int ac_coef_grad_floats(const ac_handle* h, size_t* floats) {
    if (!h || !floats) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    const int F = cgrad_floats_of(h);
    if (!F) return fail(AC_ERR_UNSUPPORTED, "coefficient gradients exist for the cubic-fit (poly) and the linear model only");
    *floats = (size_t)F;
    return AC_OK;
}

int ac_cgrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats) {
    return pgrad_workspace_floats<CoefGrad>(h, which, n_or_B, H, floats);
}
int ac_step_cgrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Xbar, float* Ubar, float* dtbar, float* Thetabar, float* ws, size_t ws_floats, void* stream) {
    return pgrad_step<CoefGrad>(h, X, U, dt, dt_per_unit, n, Lam, Xbar, Ubar, dtbar, Thetabar, ws, ws_floats, stream);
}
int ac_rollout_cgrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                         float* Ubar, float* dtbar, float* Thetabar, float* ws, size_t ws_floats, void* stream) {
    return pgrad_rollout<CoefGrad>(h, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Thetabar, ws, ws_floats, stream);
}

int ac_agrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats) {
    return pgrad_workspace_floats<AirframeGrad>(h, which, n_or_B, H, floats);
}
int ac_step_agrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Xbar, float* Ubar, float* dtbar, float* Phibar, float* ws, size_t ws_floats, void* stream) {
    return pgrad_step<AirframeGrad>(h, X, U, dt, dt_per_unit, n, Lam, Xbar, Ubar, dtbar, Phibar, ws, ws_floats, stream);
}
int ac_rollout_agrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                         float* Ubar, float* dtbar, float* Phibar, float* ws, size_t ws_floats, void* stream) {
    return pgrad_rollout<AirframeGrad>(h, Xtraj, U, dt, B, H, G, X0bar, Ubar, dtbar, Phibar, ws, ws_floats, stream);
}

}  // extern "C"
