// aircraft_hip.hip — C ABI (include/aircraft_hip.h) + kernel dispatch for libaircraft_hip.so.
// gfx950 only.  No allocation or synchronisation inside the compute entry points (graph-capturable).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ac_mlp_model.hpp"
#include "ac_kernels_analytic.hpp"
#include "ac_nn_decl.hpp"
#include "ac_ilqr.hpp"
#include "ac_goal.hpp"
#include "ac_ilqr_rate.hpp"
#include "ac_shoot.hpp"
#include "ac_track.hpp"
#include "ac_hess.hpp"
#include "ac_hess_adj.hpp"
#include "ac_hess_nn.hpp"
#include "ac_hess_rev.hpp"
#include "ac_select.hpp"
#include "ac_vjp.hpp"
#include "ac_trim.hpp"
#include "ac_mppi.hpp"
#include "ac_lqr.hpp"
#include "ac_eig.hpp"
#include "ac_ekf.hpp"
#include "ac_rts.hpp"
#include "ac_em.hpp"
#include "ac_ieks.hpp"
#include "ac_ukf.hpp"
#include "ac_lqg.hpp"
#include "ac_wgrad.hpp"
#include "ac_cgrad.hpp"
#include "ac_agrad.hpp"

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

namespace {

thread_local char g_err[512] = "";

int hip_fail(hipError_t e, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return AC_ERR_HIP;
}
// every non-HIP error return that carries text goes through here, so ac_last_error() never shows a stale message
int fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
#define AC_HIP(call)                                           \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #call);      \
    } while (0)

}  // namespace

// The handle IS a model description (plans, wt, routes: MlpModelInfo, ac_mlp_model.hpp — what ac_set_mlp hands over from
// build_mlp_model) plus the device state around it.
struct ac_handle : MlpModelInfo {
    DevParams dp;
    int device;
    int num_cus;
    // measurement aids, diagnostic flavours only (-DAC_DIAG_ENV; always false in the product library):
    bool no_pair;  // AIRCRAFT_HIP_NO_PAIR=1: never route a remainder to k_nn_step_sens_pair
    bool all_pair; // AIRCRAFT_HIP_ALL_PAIR=1: every unit through k_nn_step_sens_pair
    bool f16_ring3; // AIRCRAFT_HIP_F16_RING3=1: the one-wave f16 kernel on the three-region ring (as a net whose fourth region does not fit)
    bool has_linear, has_poly, has_mlp;
    int hidden_route;       // ac_hidden_route (ac_set_hidden_route); 0 = AC_HIDDEN_AUTO
    float* d_rev_scratch;  // per-wave layer states of k_nn_stage_tensors_rev (ac_reserve_hess_workspace)
    size_t rev_scratch_floats;
    float* d_blob;  // packed MLP weights + biases (device)
    size_t blob_floats;
    float* d_vblob;    // weight image [layer][K][N] (+ biases) of the "MFMA off" engine, device
    float* d_wgimg;    // fragments of the folded net for the weight gradient (build_wgrad_image, ac_wgrad.hpp), device
    WgradPlan wg;
    unsigned* d_queue; // ticket counter of the persistent tiled kernels (GroupQueue, ac_mlp_valu.hpp); 0 between launches
    float* d_hess_ws;  // [n][4][126] stage tensors of the MLP Hessian path (ac_reserve_hess_workspace)
    size_t hess_ws_floats;
    float* d_hess_ws2;  // sub-step composition of the second-order blocks (substeps > 1)
    size_t hess_ws2_floats;
    float* d_poly_tab;  // coefficient, intercept and gradient tables of the cubic fits (DevParams::poly_tab)
    float* d_track;  // [nseg][3][4] segment cubics (device)
    TrackDev track;
    // kernels whose dynamic-LDS limit was already raised on this handle's device (hipFuncSetAttribute is not free)
    const void* lds_fn[48];
    int lds_bytes_set[48];
    int n_lds_fn;
    int vjp_route;   // ac_vjp_route (ac_set_vjp_route); 0 = AC_VJP_AUTO
    int cgrad_grid;  // most workgroups of the coefficient-gradient kernels (ac_set_cgrad_grid); 0 = auto
    // last launch (profiling aid)
    char last_name[64];
    int last_grid, last_block, last_lds;
};

namespace {

void note_launch(ac_handle* h, const char* name, int grid, int block, int lds) {
    snprintf(h->last_name, sizeof(h->last_name), "%s", name);
    h->last_grid = grid; h->last_block = block; h->last_lds = lds;
}

int check_params(const ac_params* p) {
    if (!p) return AC_ERR_BAD_ARG;
    if (p->substeps < 1) return AC_ERR_BAD_ARG;
    if (p->model_kind < AC_MODEL_DEFAULT || p->model_kind > AC_MODEL_QUAD) return AC_ERR_BAD_ARG;
    return AC_OK;
}

int model_ready(const ac_handle* h) {
    switch (h->dp.p.model_kind) {
        case AC_MODEL_LINEAR: return h->has_linear ? AC_OK : AC_ERR_NO_MODEL;
        case AC_MODEL_POLY: return h->has_poly ? AC_OK : AC_ERR_NO_MODEL;
        case AC_MODEL_NN: return h->has_mlp ? AC_OK : AC_ERR_NO_MODEL;
        default: return AC_OK;
    }
}

// Raise a kernel's dynamic-LDS limit once per (handle, kernel, size): the attribute is sticky per device, and the call
// costs a driver round trip that does not belong in front of every launch.
// why AC_HIDDEN_F16 cannot run on this handle's net
const char* hidden_f16_refusal(const ac_handle* h) {
    if (!(kBf16Hidden && h->use_mfma && h->wt == 8 && h->has_bf)) return "hidden route f16: only the width-128 matrix-core sensitivity kernels have an f16 form";
    switch (h->f16_gate) {
        case F16_GATE_WEIGHT: return "hidden route f16: a hidden-layer weight is outside the gate's range (|w| >= 2^15)";
        case F16_GATE_TANGENT_BOUND: return "hidden route f16: the bound of the hidden-layer tangents reaches 2^15";
        case F16_GATE_TANGENT_TINY: return "hidden route f16: the tangents entering a hidden layer are below 2^-14 (f16 subnormal range)";
        default: return "hidden route f16: the net has non-finite weights";
    }
}

template <class K> int set_lds_limit(ac_handle* h, K kernel, int bytes) {
    if (bytes <= 64 * 1024) return AC_OK;
    const void* fn = reinterpret_cast<const void*>(kernel);
    for (int i = 0; i < h->n_lds_fn; ++i)
        if (h->lds_fn[i] == fn) {
            if (h->lds_bytes_set[i] >= bytes) return AC_OK;
            AC_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
            h->lds_bytes_set[i] = bytes;
            return AC_OK;
        }
    AC_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (h->n_lds_fn < 48) { h->lds_fn[h->n_lds_fn] = fn; h->lds_bytes_set[h->n_lds_fn] = bytes; ++h->n_lds_fn; }
    return AC_OK;
}

// Launch on the handle's device whatever the caller's current device is (a process may hold handles on several GPUs);
// restores the caller's device on scope exit.  hipSetDevice is host state only: legal during stream capture.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const ac_handle* h) {
        if (h && hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};
#define AC_ENTER(h) g_err[0] = 0; DeviceGuard dev_guard_(h)

#ifndef AC_HESS_N_POLY
#define AC_HESS_N_POLY 1
#endif
#ifndef AC_HESS_N_OTHER
#define AC_HESS_N_OTHER 2
#endif
template <int MODEL> struct HessN { static constexpr int value = (MODEL == AC_MODEL_POLY) ? AC_HESS_N_POLY : AC_HESS_N_OTHER; };

// The reverse sweep in duals (ac_hess_adj.hpp), one wave per direction group and 64 units; -DAC_HESS_JETS keeps the
// second-order-jet kernel of rounds 1-3 (k_step_hess) as the A/B flavour.
// directions per lane: two where the sweep fits the register file with them (no scratch); the MLP provider's extra state
// (stage tensors, the 5 x 5 contraction) leaves room for one (AC_HESS_REV_N_NN: measured both)
#ifndef AC_HESS_REV_N
#define AC_HESS_REV_N 2
#endif
#ifndef AC_HESS_REV_N_POLY
#define AC_HESS_REV_N_POLY 1
#endif
#ifndef AC_HESS_REV_N_NN
#define AC_HESS_REV_N_NN 2
#endif
template <int MODEL>
void launch_hess(ac_handle* h, hipStream_t st, const float* X, const float* U, float dt, const float* dt_per_unit,
                        const float* Lam, long n, long blk, float* Hout, int* grid_out) {
#ifndef AC_HESS_JETS
    {
        constexpr int NR = MODEL == AC_MODEL_NN ? AC_HESS_REV_N_NN : (MODEL == AC_MODEL_POLY ? AC_HESS_REV_N_POLY : AC_HESS_REV_N);
        static_assert((16 / NR) % (kBlock / 64) == 0, "direction groups per workgroup");
        const dim3 grid((unsigned)((n + 63) / 64), (16 / NR) / (kBlock / 64));
        hipLaunchKernelGGL((k_step_hess_rev<MODEL, NR>), grid, kBlock, 0, st, h->dp, X, U, dt, dt_per_unit, Lam,
                           (const float*)h->d_hess_ws, n, blk, Hout);
        *grid_out = (int)(grid.x * grid.y);
        return;
    }
#endif
    constexpr int N = HessN<MODEL>::value;
    const long lanes = n * HessTasks<N>::value;  // upper-triangle tasks of every unit, packed across workgroups
    const int grid = (int)((lanes + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((k_step_hess<MODEL, N>), grid, kBlock, 0, st, h->dp, X, U, dt, dt_per_unit, Lam,
                       (const float*)h->d_hess_ws, n, blk, Hout);
    *grid_out = grid;
}

// ---- dispatch helpers --------------------------------------------------------------------------
#define AC_LAUNCH_ANALYTIC(KERNEL, GRID, BLOCK, ...)                                                        \
    do {                                                                                                    \
        switch (h->dp.p.model_kind) {                                                                       \
            case AC_MODEL_LINEAR: hipLaunchKernelGGL(KERNEL<AC_MODEL_LINEAR>, GRID, BLOCK, 0, st, h->dp, __VA_ARGS__); break; \
            case AC_MODEL_POLY: hipLaunchKernelGGL(KERNEL<AC_MODEL_POLY>, GRID, BLOCK, 0, st, h->dp, __VA_ARGS__); break;     \
            case AC_MODEL_QUAD: hipLaunchKernelGGL(KERNEL<AC_MODEL_QUAD>, GRID, BLOCK, 0, st, h->dp, __VA_ARGS__); break;     \
            default: hipLaunchKernelGGL(KERNEL<AC_MODEL_DEFAULT>, GRID, BLOCK, 0, st, h->dp, __VA_ARGS__); break;             \
        }                                                                                                   \
    } while (0)
// ... and as a function: f(std::integral_constant<int, MODEL>) for the handle's analytic model
template <class F> void with_analytic_model(const ac_handle* h, F&& f) {
    switch (h->dp.p.model_kind) {
        case AC_MODEL_LINEAR: f(std::integral_constant<int, AC_MODEL_LINEAR>{}); break;
        case AC_MODEL_POLY: f(std::integral_constant<int, AC_MODEL_POLY>{}); break;
        case AC_MODEL_QUAD: f(std::integral_constant<int, AC_MODEL_QUAD>{}); break;
        default: f(std::integral_constant<int, AC_MODEL_DEFAULT>{}); break;
    }
}

// One launch of a kernel with dynamic LDS (the NN kernels, the fused reverse sweeps): raise the kernel's dynamic-LDS limit,
// launch, record the launch for ac_last_launch when a name is given, and return the launch status.
template <class K, class... Args>
int launch_kernel(ac_handle* h, hipStream_t st, const char* name, K kern, int grid, int block, int lds, const Args&... args) {
    const int rc = set_lds_limit(h, kern, lds);
    if (rc != AC_OK) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
    if (name) note_launch(h, name, grid, block, lds);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// Instance selection: pick<Vs...>(v, f) hands the run-time v to the generic lambda f as a std::integral_constant and returns
// f's status, or kNoInstance when v is none of Vs; instance() turns that into the caller's error.  Only instances declared in
// ac_nn_decl.hpp may be named in f: every other one would be compiled into this unit.
constexpr int kNoInstance = 1;  // (no ac_status is positive)
const char* const kNoNnInstance = "no kernel instance for this MLP width / flavour";
const char* const kNoTiledInstance = "no tiled vector-ALU kernel instance for this hidden width";
template <int... Vs, class F> int pick(int v, F&& f) {
    int rc = kNoInstance;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
// ... over the handle's (wt, use_mfma): f(WT, MF) with MF a std::bool_constant
template <class F> int pick_wt_mfma(const ac_handle* h, F&& f) {
    return pick<2, 4, 8>(h->wt, [&](auto WT) { return h->use_mfma ? f(WT, std::true_type{}) : f(WT, std::false_type{}); });
}
int instance(int rc, const char* missing) { return rc == kNoInstance ? fail(AC_ERR_UNSUPPORTED, missing) : rc; }
// ... over the models of the fused reverse sweeps (ac_vjp.hpp): f(MODEL).  The callers' route and refusal checks have excluded
// the MLP surrogate and the quadrotor.
template <class F> int pick_fused_model(const ac_handle* h, F&& f) {
    return instance(pick<AC_MODEL_DEFAULT, AC_MODEL_LINEAR, AC_MODEL_POLY>(h->dp.p.model_kind, f),
                    "no fused reverse sweep for this model");
}

// The plan of the kernels on MlpEngine (sensitivity and forward): the matrix-core flavour runs its edge layers on the vector
// ALUs and takes plan_sens; the cross-lane validation flavour keeps plan.  (The second-order and the cooperative rollout
// engines: plan.)
const MlpPlan& engine_plan(const ac_handle* h) { return h->use_mfma ? h->plan_sens : h->plan; }

// T steps as a host loop over an estimator's step, for a caller that has run the estimator's *_check.  step: its *_step_impl
// on the handle, the options and the workspace; buf: the two (x, P) pairs of the ping-pong in that workspace; name: what the
// messages call it.  Xpreds, Ppreds, Abars: the per-step records a smoother reads (each may be NULL).
template <class Step>
int filter_loop(const char* name, bool predict, Step step, float* const buf[4], const float* X, const float* P, const float* U,
                float dt, const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                float* Ppreds, float* Abars, void* stream) {
    if (!X || !P || !Z || !Rd || !Xo || !Po || !ll) {
        snprintf(g_err, sizeof(g_err), "%s filter: a required pointer is NULL", name);
        return AC_ERR_BAD_ARG;
    }
    if (predict && (!U || !Qd)) {
        snprintf(g_err, sizeof(g_err), "%s filter: U and Qd are required when predict is set", name);
        return AC_ERR_BAD_ARG;
    }
    const size_t N = (size_t)n;
    const float *xin = X, *pin = P;
    for (long t = 0; t < T; ++t) {
        const bool last = t == T - 1;
        float* const xo = last ? Xo : buf[2 * (t & 1)];
        float* const po = last ? Po : buf[2 * (t & 1) + 1];
        const size_t k = (size_t)t;
        const int rc = step(xin, pin, U ? U + k * 7 * N : nullptr, dt, Z + k * 15 * N, mask ? mask + k * N : nullptr, Qd, Rd, n,
                            t ? ll : nullptr, xo, po, nu ? nu + k * 15 * N : nullptr, S ? S + k * 15 * N : nullptr,
                            nis ? nis + k * N : nullptr, ll, used ? used + k * N : nullptr, status ? status + k * N : nullptr,
                            Xpreds ? Xpreds + k * 13 * N : nullptr, Ppreds ? Ppreds + k * 144 * N : nullptr,
                            Abars ? Abars + k * 144 * N : nullptr);
        if (rc != AC_OK) return rc;
        if (Xs) AC_HIP(hipMemcpyAsync(Xs + k * 13 * N, xo, 13 * N * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        if (Ps) AC_HIP(hipMemcpyAsync(Ps + k * 144 * N, po, 144 * N * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        xin = xo;
        pin = po;
    }
    return AC_OK;
}

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

const char* ac_last_error(void) { return g_err; }
const char* ac_version(void) { return "aircraft_hip 0.1 (gfx950)"; }

int ac_device_arch(char* buf, size_t len) {
    if (!buf || len == 0) return AC_ERR_BAD_ARG;
    int dev = 0;
    AC_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    AC_HIP(hipGetDeviceProperties(&prop, dev));
    snprintf(buf, len, "%s", prop.gcnArchName);
    return AC_OK;
}

int ac_create(const ac_params* params, ac_handle** out) {
    if (!out) return AC_ERR_BAD_ARG;
    int rc = check_params(params);
    if (rc != AC_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        snprintf(g_err, sizeof(g_err), "no HIP device visible");
        return AC_ERR_NO_DEVICE;
    }
    ac_handle* h = new (std::nothrow) ac_handle();
    if (!h) return AC_ERR_BAD_ARG;
    memset(h, 0, sizeof(*h));
    h->dp.p = *params;
    {
        hipError_t e = hipGetDevice(&h->device);
        if (e != hipSuccess) { delete h; return hip_fail(e, "hipGetDevice"); }
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess) h->num_cus = cus;
    }
#ifdef AC_DIAG_ENV
    {   // measurement switches exist in the diagnostic flavours only (build.py --diag / tools/archive/variant_lib.sh -DAC_DIAG_ENV):
        // the product library's dispatch never depends on the environment
        const char* e = getenv("AIRCRAFT_HIP_NO_PAIR");
        h->no_pair = e && e[0] == '1';
        const char* ea = getenv("AIRCRAFT_HIP_ALL_PAIR");
        h->all_pair = ea && ea[0] == '1';
        const char* e3 = getenv("AIRCRAFT_HIP_F16_RING3");
        h->f16_ring3 = e3 && e3[0] == '1';
        // AIRCRAFT_HIP_HIDDEN_ROUTE=bf16|f16: the handle's initial hidden-layer route (ac_set_hidden_route overrides it)
        const char* er = getenv("AIRCRAFT_HIP_HIDDEN_ROUTE");
        if (er && !strcmp(er, "bf16")) h->hidden_route = AC_HIDDEN_BF16;
        if (er && !strcmp(er, "f16")) h->hidden_route = AC_HIDDEN_F16;
    }
#endif
#if defined(AC_STAMPS) || defined(AC_CLOCKS)
    h->no_pair = true;  // the diagnostic flavours pass their buffer through `c`; only k_nn_step_sens knows that
#endif
    {   // ticket counter of the persistent kernels' work queue: zero now, and left at zero by every launch that uses it
        hipError_t e = hipMalloc(&h->d_queue, 256);
        if (e == hipSuccess) e = hipMemset(h->d_queue, 0, 256);
        if (e != hipSuccess) { if (h->d_queue) (void)hipFree(h->d_queue); delete h; return hip_fail(e, "hipMalloc(work queue)"); }
    }
    *out = h;
    return AC_OK;
}

int ac_destroy(ac_handle* h) {
    AC_ENTER(h);
    if (!h) return AC_ERR_BAD_ARG;
    if (h->d_blob) (void)hipFree(h->d_blob);
    if (h->d_vblob) (void)hipFree(h->d_vblob);
    if (h->d_wgimg) (void)hipFree(h->d_wgimg);
    if (h->d_queue) (void)hipFree(h->d_queue);
    if (h->d_track) (void)hipFree(h->d_track);
    if (h->d_poly_tab) (void)hipFree(h->d_poly_tab);
    if (h->d_hess_ws) (void)hipFree(h->d_hess_ws);
    if (h->d_hess_ws2) (void)hipFree(h->d_hess_ws2);
    if (h->d_rev_scratch) (void)hipFree(h->d_rev_scratch);
    delete h;
    return AC_OK;
}

int ac_set_params(ac_handle* h, const ac_params* params) {
    if (!h) return AC_ERR_BAD_ARG;
    int rc = check_params(params);
    if (rc != AC_OK) return rc;
    h->dp.p = *params;
    return AC_OK;
}

int ac_set_linear(ac_handle* h, const float* W) {
    if (!h || !W) return AC_ERR_BAD_ARG;
    memcpy(h->dp.linear_W, W, sizeof(float) * 36);
    h->has_linear = true;
    return AC_OK;
}

int ac_set_poly(ac_handle* h, const float* coef, const float* intercept) {
    if (!h || !coef || !intercept) return AC_ERR_BAD_ARG;
    AC_ENTER(h);
    float tab[kPolyTabFloats], grad[6 * 4 * 15], hess[6 * 10 * 5];
    poly_gradient_tables(coef, grad);
    poly_hessian_tables(grad, hess);
    poly_pack_tables(coef, intercept, grad, hess, tab);
    if (!h->d_poly_tab) AC_HIP(hipMalloc((void**)&h->d_poly_tab, sizeof(tab)));
    AC_HIP(hipMemcpy(h->d_poly_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
    h->dp.poly_tab = h->d_poly_tab;
    h->has_poly = true;
    return AC_OK;
}

int ac_set_mlp(ac_handle* h, int n_layers, const int* widths, const int* act, const float* const* W,
               const float* const* b, const float* in_mean, const float* in_std, const float* out_mean,
               const float* out_std, int use_mfma) {
    AC_ENTER(h);
    if (!h || !widths || !act || !W || !b || !in_mean || !in_std || !out_mean || !out_std) return AC_ERR_BAD_ARG;
    // the folded net, the packed blob, the LDS plans and the vector-ALU image: host arithmetic, ac_mlp_model.hpp
    MlpModel m;
    const int rc = build_mlp_model(n_layers, widths, act, W, b, use_mfma, m, g_err, sizeof(g_err));
    if (rc != AC_OK) return rc;
    float* dv = nullptr;
    if (m.has_vplan) {
        AC_HIP(hipMalloc(&dv, m.vimage.size() * sizeof(float)));
        hipError_t ev = hipMemcpy(dv, m.vimage.data(), m.vimage.size() * sizeof(float), hipMemcpyHostToDevice);
        if (ev != hipSuccess) { (void)hipFree(dv); return hip_fail(ev, "hipMemcpy(valu image)"); }
    }
    WgradPlan wg;
    float* dw = nullptr;
    {
        std::vector<float> wimg;
        build_wgrad_image(m, wg, wimg);
        hipError_t ew = hipMalloc(&dw, wimg.size() * sizeof(float));
        if (ew == hipSuccess) ew = hipMemcpy(dw, wimg.data(), wimg.size() * sizeof(float), hipMemcpyHostToDevice);
        if (ew != hipSuccess) { if (dw) (void)hipFree(dw); if (dv) (void)hipFree(dv); return hip_fail(ew, "hipMalloc/hipMemcpy(wgrad image)"); }
    }
    float* d = nullptr;
    {
        hipError_t em = hipMalloc(&d, m.blob.size() * sizeof(float));
        if (em != hipSuccess) { if (dv) (void)hipFree(dv); (void)hipFree(dw); return hip_fail(em, "hipMalloc(mlp blob)"); }
    }
    hipError_t e = hipMemcpy(d, m.blob.data(), m.blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); if (dv) (void)hipFree(dv); (void)hipFree(dw); return hip_fail(e, "hipMemcpy(mlp blob)"); }
    if (h->d_wgimg) (void)hipFree(h->d_wgimg);
    h->d_wgimg = dw;
    h->wg = wg;
    if (h->d_vblob) (void)hipFree(h->d_vblob);
    h->d_vblob = dv;
    if (h->d_blob) (void)hipFree(h->d_blob);
    h->d_blob = d;
    h->blob_floats = m.blob.size();
    static_cast<MlpModelInfo&>(*h) = m;
    memcpy(h->dp.mlp_in_mean, in_mean, 5 * sizeof(float));
    memcpy(h->dp.mlp_in_std, in_std, 5 * sizeof(float));
    memcpy(h->dp.mlp_out_mean, out_mean, 6 * sizeof(float));
    memcpy(h->dp.mlp_out_std, out_std, 6 * sizeof(float));
    for (int k = 0; k < 6; ++k)
        for (int j = 0; j < 5; ++j) h->dp.mlp_jscale[k][j] = out_std[k] / in_std[j];  // float / float: one IEEE rounding
    h->has_mlp = true;
    return AC_OK;
}

// ---- compute entry points ------------------------------------------------------------------------
static int launch_nn_fwd(ac_handle* h, int op, const float* X, const float* U, float dt, const float* dtp, long n,
                         long blk, float* out, hipStream_t st) {
    auto name = [&](const char* deriv, const char* step, const char* aero) { return op == OP_DERIV ? deriv : (op == OP_STEP ? step : aero); };
    if (!h->use_mfma && h->has_vplan) {
        // "MFMA off": the value-only tile of ac_mlp_valu.hpp, 64 units per wave, 256 per workgroup
        const int grid = (int)((n + kBlock - 1) / kBlock);
        const int lds = h->vplan.image_floats * 4 + 4 * 64 * (h->vwidth + 4) * 4;
        return instance(pick<OP_DERIV, OP_STEP, OP_AERO>(op, [&](auto o) {
            constexpr int OP = o;
            return pick<32, 64>(h->vwidth, [&](auto W) {
                return launch_kernel(h, st, name("k_nn_fwd_tiled<deriv>", "k_nn_fwd_tiled<step>", "k_nn_fwd_tiled<aero>"),
                                 k_nn_fwd_tiled<W(), OP>, grid, kBlock, lds, h->dp, h->vplan, h->d_vblob, X, U, dt, dtp, n, blk, out);
            });
        }), kNoTiledInstance);
    }
    // Two kernels: k_nn_fwd (16 units per wave, 64 per workgroup) and k_nn_fwd4 (four value slabs per wave, 256 units per
    // workgroup: the per-layer fixed costs are shared, measured 3.4x the time of a 64-unit workgroup for 4x the units).
    // One workgroup per CU is resident, so time goes in whole ROUNDS over the CUs and the last, partly filled round costs
    // as much as a full one.  Split the batch: the units that fill whole rounds of k_nn_fwd4 go there, the remainder
    // (less than one such round) runs in the cheaper rounds of k_nn_fwd; take whichever of {all fwd, all fwd4, split}
    // has the lowest modelled cost (in k_nn_fwd rounds).
    const long cus = h->num_cus > 0 ? h->num_cus : 256;
    const double kFwd4Round = 3.4;
    auto rounds = [&](long units, long per_wg) { return (double)(((units + per_wg - 1) / per_wg + cus - 1) / cus); };
    const long full4 = h->use_mfma ? (n / (256 * cus)) * (256 * cus) : 0;
    const double cost_fwd = rounds(n, 64), cost_fwd4 = h->use_mfma ? kFwd4Round * rounds(n, 256) : 1e30;
    const double cost_split = (full4 > 0 && full4 < n) ? kFwd4Round * (double)(full4 / (256 * cus)) + rounds(n - full4, 64) + 0.05
                                                       : 1e30;
    long n4 = 0;  // units [0, n4) take k_nn_fwd4, [n4, n) take k_nn_fwd
    if (cost_fwd4 <= cost_fwd && cost_fwd4 <= cost_split) n4 = n;
    else if (cost_split < cost_fwd) n4 = full4;
    const MlpPlan& plan = engine_plan(h);
    if (n4 > 0) {
        const int grid4 = (int)((n4 + kBlock - 1) / kBlock);
        const long zero = 0;
        const int rc = instance(pick<OP_DERIV, OP_STEP, OP_AERO>(op, [&](auto o) {
            constexpr int OP = o;
            return pick<2, 4, 8>(h->wt, [&](auto WT) {
                return launch_kernel(h, st, name("k_nn_fwd4<deriv>", "k_nn_fwd4<step>", "k_nn_fwd4<aero>"), k_nn_fwd4<WT(), OP>, grid4,
                                 kBlock, plan.lds_total, h->dp, plan, h->d_blob, X, U, dt, dtp, n4, blk, out, zero);
            });
        }), kNoNnInstance);
        if (rc != AC_OK || n4 == n) return rc;
    }
    const int grid = (int)((n - n4 + 63) / 64);
    return instance(pick<OP_DERIV, OP_STEP, OP_AERO>(op, [&](auto o) {
        constexpr int OP = o;
        return pick_wt_mfma(h, [&](auto WT, auto MF) {  // (ac_last_launch keeps k_nn_fwd4 when it ran)
            return launch_kernel(h, st, n4 == 0 ? name("k_nn_fwd<deriv>", "k_nn_fwd<step>", "k_nn_fwd<aero>") : nullptr,
                             k_nn_fwd<WT(), MF(), OP>, grid, kBlock, plan.lds_total, h->dp, plan, h->d_blob, X, U, dt, dtp, n, blk, out, n4);
        });
    }), kNoNnInstance);
}

static int derivative_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;  // empty batch: nothing to do (pointers may be NULL)
    if (!h || !X || !U || !Xdot || n < 0 || blk <= 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (n == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN) return launch_nn_fwd(h, OP_DERIV, X, U, 0.f, nullptr, n, blk, Xdot, st);
    const int grid = (int)((n + kBlock - 1) / kBlock);
    AC_LAUNCH_ANALYTIC(k_state_derivative, grid, kBlock, X, U, n, blk, Xdot);
    note_launch(h, "k_state_derivative", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_state_derivative_f32(ac_handle* h, const float* X, const float* U, long n, float* Xdot, void* stream) {
    return derivative_impl(h, X, U, n, n > 0 ? n : 1, Xdot, stream);
}

int ac_shoot_derivative_f32(ac_handle* h, const float* X, const float* U, long B, long H, float* Xdot, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return derivative_impl(h, X, U, B * H, B > 0 ? B : 1, Xdot, stream);
}

static int step_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
                     float* Xn, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Xn || n < 0 || blk < 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (n == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN) return launch_nn_fwd(h, OP_STEP, X, U, dt, dt_per_unit, n, blk, Xn, st);
    const int grid = (int)((n + kBlock - 1) / kBlock);
    AC_LAUNCH_ANALYTIC(k_step, grid, kBlock, X, U, dt, dt_per_unit, n, blk, Xn);
    note_launch(h, "k_step", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_step_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, float* Xn,
                void* stream) {
    return step_impl(h, X, U, dt, dt_per_unit, n, n, Xn, stream);
}

int ac_shoot_step_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B, long H,
                      float* Xn, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return step_impl(h, X, U, dt, dt_per_unit, B * H, B, Xn, stream);
}

static int deriv_sens_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, float* Fx,
                           float* Fu, void* stream);

// ---- the defect rows of multiple shooting, written by the step / derivative kernels themselves (control/base.py:275-286) ----
namespace {
struct RowsScope {  // the launch takes a copy of h->dp: set for the launches in scope, plain again afterwards
    ac_handle* h;
    RowsScope(ac_handle* h_, int rows, float dt, const float* dtp, float* aux) : h(h_) {
        h->dp.rows = rows; h->dp.rows_dt = dt; h->dp.rows_dt_per_unit = dtp; h->dp.rows_aux = aux;
    }
    ~RowsScope() { h->dp.rows = AC_ROWS_PLAIN; h->dp.rows_dt = 0.f; h->dp.rows_dt_per_unit = nullptr; h->dp.rows_aux = nullptr; }
};
}  // namespace

int ac_shoot_defect_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B, long H,
                        float* R, void* stream) {
    if (!h || B < 0 || H < 0) return AC_ERR_BAD_ARG;
    RowsScope scope(h, AC_ROWS_DEFECT, 0.f, nullptr, nullptr);
    return step_impl(h, X, U, dt, dt_per_unit, B * H, B, R, stream);
}

int ac_shoot_implicit_defect_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                                 long H, float* R, void* stream) {
    if (!h || B < 0 || H < 0) return AC_ERR_BAD_ARG;
    if (h && B * H == 0) return AC_OK;
    if (!X) return AC_ERR_BAD_ARG;
    RowsScope scope(h, AC_ROWS_IMPLICIT, dt, dt_per_unit, nullptr);
    return derivative_impl(h, X + 13 * B, U, B * H, B > 0 ? B : 1, R, stream);  // f at the NEXT nodes, paired with u_k
}

int ac_shoot_implicit_rows_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                               long H, float* R, float* Jnext, float* Ju, float* Jdt, void* stream) {
    if (!h || B < 0 || H < 0) return AC_ERR_BAD_ARG;
    if (h && B * H == 0) return AC_OK;
    if (!X || !Jdt) return AC_ERR_BAD_ARG;
    RowsScope scope(h, AC_ROWS_IMPLICIT, dt, dt_per_unit, Jdt);
    return deriv_sens_impl(h, X + 13 * B, U, B * H, B > 0 ? B : 1, R, Jnext, Ju, stream);
}

int ac_aero_f32(ac_handle* h, const float* X, const float* U, long n, float* out, void* stream) {
    AC_ENTER(h);
    const long blk = n;
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !out || n < 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (n == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN) return launch_nn_fwd(h, OP_AERO, X, U, 0.f, nullptr, n, blk, out, st);
    const int grid = (int)((n + kBlock - 1) / kBlock);
    AC_LAUNCH_ANALYTIC(k_aero, grid, kBlock, X, U, n, blk, out);
    note_launch(h, "k_aero", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_rollout_f32(ac_handle* h, const float* X0, const float* U, float dt, long B, long H, float* Xout,
                   void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !X0 || !Xout || B < 0 || H < 0 || (H > 0 && !U)) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (B == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    const long roll_units = h->vwidth == 64 ? kRolloutUnits<64> : kRolloutUnits<32>;  // instances per wave of k_nn_rollout_tiled8
    if (h->dp.p.model_kind == AC_MODEL_NN && !h->use_mfma && h->has_vplan && B <= roll_units * 4 * (long)(h->num_cus > 0 ? h->num_cus : 256)) {
        // small batches (at most one wave per SIMD): the latency of the 4 H sequential network evaluations is what counts —
        // the value-only tile with 4 or 8 instances per wave, four waves per workgroup
        const int grid = (int)((B + 4 * roll_units - 1) / (4 * roll_units));
        const int lds = h->vplan.image_floats * 4 + 4 * (int)roll_units * (h->vwidth + 4) * 4;
        return instance(pick<32, 64>(h->vwidth, [&](auto W) {
            return launch_kernel(h, st, "k_nn_rollout_tiled8", k_nn_rollout_tiled8<W()>, grid, kBlock, lds, h->dp, h->vplan, h->d_vblob,
                             X0, U, dt, B, H, Xout);
        }), kNoTiledInstance);
    }
    if (h->dp.p.model_kind == AC_MODEL_NN && !h->use_mfma && h->has_vplan) {
        const int grid = (int)((B + kBlock - 1) / kBlock);
        const int lds = h->vplan.image_floats * 4 + 4 * 64 * (h->vwidth + 4) * 4;
        return instance(pick<32, 64>(h->vwidth, [&](auto W) {
            return launch_kernel(h, st, "k_nn_rollout_tiled", k_nn_rollout_tiled<W()>, grid, kBlock, lds, h->dp, h->vplan, h->d_vblob,
                             X0, U, dt, B, H, Xout);
        }), kNoTiledInstance);
    }
    if (h->dp.p.model_kind == AC_MODEL_NN) {
        const long groups = (B + 15) / 16;  // 16 instances per wave-slab
        const int nh = h->plan.n_layers - 2;  // hidden (width x width) layers
        if (h->use_mfma && groups < 4096 && nh >= 1 && nh <= 3) {
            // cooperative with register-resident weights: each wave keeps the fragments of its own output tiles
            const int grid = (int)groups;
            const int lds = 2 * h->wt * 1024;  // double-buffered activation exchange only
            return instance(pick<2, 4, 8>(h->wt, [&](auto wt) {
                constexpr int WT = wt;
                return pick<1, 2, 3>(nh, [&](auto NH) {
                    return launch_kernel(h, st, "k_nn_rollout_reg", k_nn_rollout_reg<WT, NH()>, grid, kBlock, lds, h->dp, h->plan,
                                     h->d_blob, X0, U, dt, B, H, Xout);
                });
            }), kNoNnInstance);
        }
        if (h->use_mfma && groups < 4096) {
            // cooperative: one 4-wave workgroup per 16 instances (4x the parallelism per instance)
            const int grid = (int)groups;
            const int lds = h->plan.lds_total + h->wt * 1024;  // + the activation exchange buffer
            return instance(pick<2, 4, 8>(h->wt, [&](auto WT) {
                return launch_kernel(h, st, "k_nn_rollout_coop", k_nn_rollout_coop<WT(), true>, grid, kBlock, lds, h->dp, h->plan,
                                 h->d_blob, X0, U, dt, B, H, Xout);
            }), kNoNnInstance);
        }
        const int grid = (int)((groups + 3) / 4);
        const MlpPlan& plan = engine_plan(h);
        return instance(pick_wt_mfma(h, [&](auto WT, auto MF) {
            return launch_kernel(h, st, "k_nn_rollout", k_nn_rollout<WT(), MF()>, grid, kBlock, plan.lds_total, h->dp, plan, h->d_blob,
                             X0, U, dt, B, H, Xout);
        }), kNoNnInstance);
    }
    const int grid = (int)((B + 63) / 64);
    AC_LAUNCH_ANALYTIC(k_rollout, grid, 64, X0, U, dt, B, H, Xout);
    note_launch(h, "k_rollout", grid, 64, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

static int sens_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
                     float* Xn, float* A, float* Bm, float* c, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Xn || !A || !Bm || n < 0 || blk < 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (n == 0) return AC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN) {
        // MLP: 16 units per wave, 4 waves (64 units) per workgroup, one workgroup resident per CU — time goes in whole
        // rounds over the CUs.  A remainder of at most half a round is given to k_nn_step_sens_pair (two waves per 16
        // units, 32 units per workgroup, ~0.73 of a full workgroup's time) instead of paying a full round for it.
        if (!h->use_mfma && h->has_vplan) {
            // "MFMA off": the tiled v_pk_fma_f32 engine (ac_mlp_valu.hpp)
            // 8 units per wave, eight waves per workgroup (two per SIMD), persistent: at most one workgroup per CU
            const long cus_t = h->num_cus > 0 ? h->num_cus : 256;
            // (a batch smaller than the chip fills whole workgroups: 200 full ones ran cfg2's 12 800 units in 0.120 ms, 256 of
            // six or seven working waves in 0.135)
            const int grid = (int)std::min<long>((n + 63) / 64, cus_t);
            const int lds = h->vplan.image_floats * 4 + 8 * 48 * (h->vwidth + 4) * 4;
            return instance(pick<32, 64>(h->vwidth, [&](auto W) {
                return launch_kernel(h, st, "k_nn_step_sens_tiled8", k_nn_step_sens_tiled8<W()>, grid, kBlock8, lds, h->dp, h->vplan,
                                 h->d_vblob, X, U, dt, dt_per_unit, n, blk, Xn, A, Bm, c, h->d_queue);
            }), kNoTiledInstance);
        }
        const long cus = h->num_cus > 0 ? h->num_cus : 256;
        const long per_round = 64 * cus;
        long n_main = n, n_pair = 0;
        // (the pair kernel wants >= 1 hidden layer: its no-value role forms the first layer's act' itself, and the barriers of
        // the hidden layers separate the reads of one evaluation's output exchange from the next one's writes)
        if (h->use_mfma && !h->no_pair && h->plan.n_layers >= 3 && h->dp.p.substeps <= 1) {  // (sub-stepped updates: one-wave kernel)
            const long rem = n % per_round;
            if (rem > 0 && rem <= 32 * cus) { n_main = n - rem; n_pair = rem; }
            if (h->all_pair) { n_main = 0; n_pair = n; }
        }
        // width 128 on the matrix cores: the hidden layers on bf16 MFMA (plan_bf; -DAC_HIDDEN_FP32: plan_sens, as round 4)
        const bool bf = kBf16Hidden && h->use_mfma && h->wt == 8 && h->has_bf;
        // ... and on two-plane f16 MFMA where the net passed the range gate (ac_set_mlp); the bf16 kernels are the fall-back.
        // AC_HIDDEN_F16 forced on a net the gate rejects (or on one without such kernels) is an error, never a fall-back.
        const bool f16_ok = bf && h->f16_gate == F16_GATE_OK;
        if (h->hidden_route == AC_HIDDEN_F16 && !f16_ok) return fail(AC_ERR_UNSUPPORTED, hidden_f16_refusal(h));
        const bool f16 = f16_ok && h->hidden_route != AC_HIDDEN_BF16;
        if (h->use_mfma && h->wt == 2 && h->dp.p.substeps <= 1) {
            // small nets: two persistent workgroups per CU = two waves per SIMD (k_nn_step_sens_w2)
            const int lds = ((h->plan_sens.lds_total + 15) & ~15) + kSensW2AccBytes;
            if (lds <= 80 * 1024) {
                const int grid = (int)std::min<long>((n + 63) / 64, 2 * cus);
                return launch_kernel(h, st, "k_nn_step_sens_w2", k_nn_step_sens_w2<2>, grid, kBlock, lds, h->dp, h->plan_sens, h->d_blob,
                                 X, U, dt, dt_per_unit, n, blk, Xn, A, Bm, c);
            }
        }
        if (n_main > 0) {
            // persistent: at most one workgroup per CU, each walks the 64-unit tasks b, b + grid, ... (k_nn_step_sens)
#ifndef AC_NO_PERSIST
            const int grid = (int)std::min<long>((n_main + 63) / 64, cus);
#else
            const int grid = (int)((n_main + 63) / 64);  // (A/B flavour: a workgroup per task, as in round 2)
#endif
            const MlpPlan& plan = f16 ? h->plan_f16 : bf ? h->plan_bf : engine_plan(h);
            // the f16 kernel streams whole layers through FOUR half-layer regions, the fourth behind the plan's three
            // (f16_ring4_lds, ac_mlp_plan.hpp); a net whose fourth region does not fit keeps the three-region kernel
            const bool ring4 = f16 && h->f16_ring4_lds > 0 && !h->f16_ring3;
            const int lds_main = ring4 ? h->f16_ring4_lds : plan.lds_total;
            auto launch_main = [&](auto kern) {
                return launch_kernel(h, st, "k_nn_step_sens", kern, grid, kBlock, lds_main, h->dp, plan, h->d_blob, X, U, dt,
                                 dt_per_unit, n_main, blk, Xn, A, Bm, c);
            };
            const int rc_m = ring4 ? launch_main(k_nn_step_sens<8, true, kHiddenF16>)
                                 : f16 ? launch_main(k_nn_step_sens<8, true, kHiddenF16Ring3>)
                                 : instance(pick_wt_mfma(h, [&](auto WT, auto MF) { return launch_main(k_nn_step_sens<WT(), MF()>); }),
                                            kNoNnInstance);
            if (rc_m != AC_OK) return rc_m;
        }
        if (n_pair > 0) {
            const int grid_p = (int)((n_pair + 31) / 32);
            const MlpPlan& plan_p = f16 ? h->plan_f16_pair : bf ? h->plan_bf_pair : h->plan_sens;
            const int lds_p = plan_p.lds_total + 2 * h->wt * 1024 + 2 * 16 * 36 * (int)sizeof(float);  // + the pairs' activation and output exchanges
            auto launch_pair = [&](auto kern) {  // (ac_last_launch keeps the main kernel when there is one)
                return launch_kernel(h, st, n_main == 0 ? "k_nn_step_sens_pair" : nullptr, kern, grid_p, kBlock, lds_p, h->dp, plan_p,
                                 h->d_blob, X, U, dt, dt_per_unit, n, blk, Xn, A, Bm, c, n_main);
            };
            return f16 ? launch_pair(k_nn_step_sens_pair<8, kHiddenF16>)
                       : instance(pick<2, 4, 8>(h->wt, [&](auto WT) { return launch_pair(k_nn_step_sens_pair<WT()>); }), kNoNnInstance);
        }
        return AC_OK;
    }
    // analytic: 4 N units per wave, N = directions per lane of the model (AnalyticSensN), 4 waves per workgroup
    const int upb = 16 * (h->dp.p.model_kind == AC_MODEL_POLY ? AnalyticSensN<AC_MODEL_POLY>::value : AnalyticSensN<AC_MODEL_DEFAULT>::value);
    static_assert(AnalyticSensN<AC_MODEL_DEFAULT>::value == AnalyticSensN<AC_MODEL_LINEAR>::value, "grid size below");
    const int grid_an = (int)((n + upb - 1) / upb);
    // (sub-stepped updates: a kernel of its own, so that the composition code does not set the registers of the common one)
    with_analytic_model(h, [&](auto M) {
        if (h->dp.p.substeps > 1) hipLaunchKernelGGL((k_step_sens<M(), true>), grid_an, kBlock, 0, st, h->dp, X, U, dt, dt_per_unit, n, blk, Xn, A, Bm, c);
        else hipLaunchKernelGGL((k_step_sens<M(), false>), grid_an, kBlock, 0, st, h->dp, X, U, dt, dt_per_unit, n, blk, Xn, A, Bm, c);
    });
    note_launch(h, "k_step_sens", grid_an, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_step_sens_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n,
                     float* Xn, float* A, float* Bm, float* c, void* stream) {
    return sens_impl(h, X, U, dt, dt_per_unit, n, n, Xn, A, Bm, c, stream);
}

int ac_shoot_sens_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B, long H,
                      float* Xn, float* A, float* Bm, float* c, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return sens_impl(h, X, U, dt, dt_per_unit, B * H, B, Xn, A, Bm, c, stream);
}

// ---- x_dot with df/dx, df/du; envelope rows; quaternion rows (control/base.py:282-304, control/aircraft.py:44-59) ----
static int deriv_sens_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, float* Fx,
                           float* Fu, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Xdot || !Fx || !Fu || n < 0 || blk <= 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN && !h->use_mfma && h->has_vplan) {
        const long cus_t = h->num_cus > 0 ? h->num_cus : 256;
        const int grid = (int)std::min<long>((n + 63) / 64, cus_t);  // persistent workgroups + work queue (GroupQueue, ac_mlp_valu.hpp)
        const int lds = h->vplan.image_floats * 4 + 8 * 48 * (h->vwidth + 4) * 4;
        return instance(pick<32, 64>(h->vwidth, [&](auto W) {
            return launch_kernel(h, st, "k_nn_deriv_sens_tiled8", k_nn_deriv_sens_tiled8<W()>, grid, kBlock8, lds, h->dp, h->vplan,
                             h->d_vblob, X, U, n, blk, Xdot, Fx, Fu, h->d_queue);
        }), kNoTiledInstance);
    }
    if (h->dp.p.model_kind == AC_MODEL_NN) {
        const int grid = (int)((n + 63) / 64);
        const MlpPlan& plan = engine_plan(h);
        return instance(pick_wt_mfma(h, [&](auto WT, auto MF) {
            return launch_kernel(h, st, "k_nn_deriv_sens", k_nn_deriv_sens<WT(), MF()>, grid, kBlock, plan.lds_total, h->dp, plan,
                             h->d_blob, X, U, n, blk, Xdot, Fx, Fu);
        }), kNoNnInstance);
    }
    const int upb = 16 * (h->dp.p.model_kind == AC_MODEL_POLY ? AnalyticSensN<AC_MODEL_POLY>::value : AnalyticSensN<AC_MODEL_DEFAULT>::value);
    const int grid = (int)((n + upb - 1) / upb);
    AC_LAUNCH_ANALYTIC(k_deriv_sens, grid, kBlock, X, U, n, blk, Xdot, Fx, Fu);
    note_launch(h, "k_deriv_sens", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_state_derivative_sens_f32(ac_handle* h, const float* X, const float* U, long n, float* Xdot, float* Fx, float* Fu,
                                 void* stream) {
    return deriv_sens_impl(h, X, U, n, n > 0 ? n : 1, Xdot, Fx, Fu, stream);
}

int ac_shoot_derivative_sens_f32(ac_handle* h, const float* X, const float* U, long B, long H, float* Xdot, float* Fx,
                                 float* Fu, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return deriv_sens_impl(h, X, U, B * H, B > 0 ? B : 1, Xdot, Fx, Fu, stream);
}

static int envelope_impl(ac_handle* h, const float* X, long n, long blk, float* rows, float* Jx, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !rows || n < 0 || blk <= 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "envelope rows are the fixed-wing plugin's (control/aircraft.py)");
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_envelope<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, X, n, blk, rows, Jx);
    note_launch(h, "k_envelope", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_envelope_f32(ac_handle* h, const float* X, long n, float* rows, float* Jx, void* stream) {
    return envelope_impl(h, X, n, n > 0 ? n : 1, rows, Jx, stream);
}

int ac_shoot_envelope_f32(ac_handle* h, const float* X, long B, long H, float* rows, float* Jx, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return envelope_impl(h, X, B * H, B > 0 ? B : 1, rows, Jx, stream);
}

static EnvelopePenalty to_dev_penalty(const ac_envelope_penalty* p) {
    EnvelopePenalty d;
    static_assert(sizeof(EnvelopePenalty) == sizeof(ac_envelope_penalty), "ac_envelope_penalty layout");
    memcpy(&d, p, sizeof(d));
    return d;
}

int ac_envelope_al_cost_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* lam, long Bl, const float* X, long B,
                            long H, float* cost, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !pen || !X || !cost || B < 0 || H < 0 || (lam && (!(pen->weight > 0.f) || Bl <= 0 || B % Bl != 0))) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "envelope rows are the fixed-wing plugin's (control/aircraft.py)");
    const int grid = (int)((B + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_envelope_cost<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_penalty(pen), lam, lam ? Bl : 1, X, B, H, cost);
    note_launch(h, "k_envelope_cost", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_envelope_cost_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* cost,
                         void* stream) {
    return ac_envelope_al_cost_f32(h, pen, nullptr, 1, X, B, H, cost, stream);
}

int ac_envelope_al_model_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* lam, const float* X, long B, long H,
                             float* node_glin, float* Hz, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !pen || !X || (!node_glin && !Hz) || B < 0 || H < 0 || (lam && !(pen->weight > 0.f))) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "envelope rows are the fixed-wing plugin's (control/aircraft.py)");
    const long n = (H + 1) * B;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_envelope_model<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_penalty(pen), lam, X, B, H, node_glin, Hz);
    note_launch(h, "k_envelope_model", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_envelope_model_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* node_glin,
                          float* Hz, void* stream) {
    return ac_envelope_al_model_f32(h, pen, nullptr, X, B, H, node_glin, Hz, stream);
}

int ac_envelope_al_update_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* lam,
                              float* viol_max, void* stream) {
    AC_ENTER(h);
    if (h && B == 0) return AC_OK;
    if (!h || !pen || !X || !lam || B < 0 || H < 0 || !(pen->weight > 0.f)) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "envelope rows are the fixed-wing plugin's (control/aircraft.py)");
    const long n = (H + 1) * B;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_envelope_multipliers<0>, grid, kBlock, 0, (hipStream_t)stream, h->dp, to_dev_penalty(pen), X, B, H, lam, viol_max);
    note_launch(h, "k_envelope_multipliers", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_quat_rows_f32(ac_handle* h, int mode, const float* X, const float* Xdot, const float* Fx, const float* Fu, long B,
                     long H, float* row, float* Jx, float* Ju, void* stream) {
    AC_ENTER(h);
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    const long n = B * H;
    if (h && n == 0) return AC_OK;
    if (!h || !X || !row || !Jx || !Ju || (mode != 0 && mode != 1)) return AC_ERR_BAD_ARG;
    if (mode == 1 && (!Xdot || !Fx || !Fu)) return AC_ERR_BAD_ARG;
    const int grid = (int)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_quat_rows<0>, grid, kBlock, 0, (hipStream_t)stream, X, Xdot, Fx, Fu, n, B, mode, row, Jx, Ju);
    note_launch(h, "k_quat_rows", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// ---- second-order step sensitivities ---------------------------------------------------------------
// persistent grid of k_nn_stage_tensors_rev: one workgroup per CU at most (its weight plan fills the LDS)
static int rev_grid(const ac_handle* h, long n) {
    const long tasks = (n + 63) / 64, cus = h->num_cus > 0 ? h->num_cus : 256;
    return (int)(tasks < cus ? tasks : cus);
}
// One RK4 sub-step's second-order block with the handle's CURRENT parameters (the caller sets substeps = 1).
static int hess_single(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, const float* Lam,
                       long n, long blk, float* Hout, hipStream_t st) {
    int grid = 0;
    AC_HIP(hipMemsetAsync(Hout, 0, (size_t)n * 441 * sizeof(float), st));
    if (h->dp.p.model_kind == AC_MODEL_NN) {
        // stage tensors (y, J, T at the four RK4 stage points) into the handle's workspace, then the same second-order
        // kernel with the tensor provider.  The workspace is sized by ac_reserve_hess_workspace (a host-side call that may
        // allocate); a compute call never allocates, frees or synchronises.
        if ((size_t)n * kStageFloats > h->hess_ws_floats)
            return fail(AC_ERR_WORKSPACE, "second-order workspace too small: call ac_reserve_hess_workspace(h, n) first");
        const int grid_t = (int)((n + 63) / 64);
#ifndef AC_NO_HESS_REV
        if (h->has_rev && h->wt == 8) {
            // width 128: forward tangents + reverse sweep (12 slab-layer products per hidden layer instead of 29), persistent grid
            const int grid_r = rev_grid(h, n);
            const size_t need_r = (size_t)grid_r * (kBlock / 64) * (size_t)rev_scratch_f32x4(h->wt, h->rev_layers - 2) * 4;
            if (need_r > h->rev_scratch_floats)
                return fail(AC_ERR_WORKSPACE, "second-order workspace too small: call ac_reserve_hess_workspace(h, n) first");
            auto launch_rev = [&](auto kern) {
                return launch_kernel(h, st, "k_nn_stage_tensors_rev", kern, grid_r, kBlock, h->plan_rev.lds_total, h->dp, h->plan_rev,
                                 h->d_blob, X, U, dt, dt_per_unit, n, blk, h->rev_layers, h->d_rev_scratch, h->d_hess_ws);
            };
#ifdef AC_HESS_REV6  // (A/B flavour: the six-slab reverse sweep, tools/archive/variant_lib.sh)
            const int rc = h->use_mfma ? launch_rev(k_nn_stage_tensors_rev<8>) : launch_rev(k_nn_stage_tensors_rev3<8, false>);
#else           // (MFMA off: the cross-lane validation form of the product)
            const int rc = h->use_mfma ? launch_rev(k_nn_stage_tensors_rev3<8, true>) : launch_rev(k_nn_stage_tensors_rev3<8, false>);
#endif
            if (rc != AC_OK) return rc;
        } else
#endif
        {
            auto launch_t = [&](auto kern) {
                return launch_kernel(h, st, nullptr, kern, grid_t, kBlock, h->plan.lds_total, h->dp, h->plan, h->d_blob, X, U, dt,
                                 dt_per_unit, n, blk, h->d_hess_ws);
            };
            int rc = instance(pick_wt_mfma(h, [&](auto WT, auto MF) {
                if constexpr (WT() == 8 && !MF()) return (int)kNoInstance;
                else return launch_t(k_nn_stage_tensors<WT(), MF(), 0>);
            }), "second-order blocks at width > 64 need the MFMA path (use_mfma = 1)");
            // width 128 on the matrix cores: the cross pairs between inputs {0, 1} and {3, 4} come from a second launch
            if (rc == AC_OK && h->wt == 8) rc = launch_t(k_nn_stage_tensors<8, true, 1>);
            if (rc != AC_OK) return rc;
        }
        launch_hess<AC_MODEL_NN>(h, st, X, U, dt, dt_per_unit, Lam, n, blk, Hout, &grid);
        note_launch(h, "k_step_hess", grid, kBlock, 0);
        AC_HIP(hipGetLastError());
        return AC_OK;
    }
    with_analytic_model(h, [&](auto M) { launch_hess<M()>(h, st, X, U, dt, dt_per_unit, Lam, n, blk, Hout, &grid); });
    note_launch(h, "k_step_hess", grid, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

// floats per unit of the sub-step composition workspace (ac_hess.hpp, "composition across RK4 sub-steps")
static size_t hess_compose_floats(int ns) { return ns > 1 ? (size_t)ns * (13 + 169 + 91 + 13 + 273) + 13 + 13 + 441 + 1 + 13 : 0; }

static int sens_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
                     float* Xn, float* A, float* Bm, float* c, void* stream);

static int hess_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, const float* Lam,
                     long n, long blk, float* Hout, void* stream) {
    AC_ENTER(h);
    if (h && n == 0) return AC_OK;
    if (!h || !X || !U || !Lam || !Hout || n < 0 || blk <= 0) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (h->dp.p.model_kind == AC_MODEL_NN && (size_t)n * kStageFloats > h->hess_ws_floats)
        return fail(AC_ERR_WORKSPACE, "second-order workspace too small: call ac_reserve_hess_workspace(h, n) first");
    const int ns = h->dp.p.substeps;
    if (ns == 1) return hess_single(h, X, U, dt, dt_per_unit, Lam, n, blk, Hout, st);

    // ---- physical_integration_substeps > 1: compose the per-sub-step blocks (ac_hess.hpp) -------------------------------
    if ((size_t)n * hess_compose_floats(ns) > h->hess_ws2_floats)
        return fail(AC_ERR_WORKSPACE, "sub-step composition workspace too small: call ac_reserve_hess_workspace(h, n) first");
    const size_t N = (size_t)n;
    float* w = h->d_hess_ws2;
    float* XS = w;                       w += N * 13 * ns;    // x_0 .. x_{ns-1}   (x_0 is a copy of the caller's X)
    float* JA = w;                       w += N * 169 * ns;
    float* JB = w;                       w += N * 91 * ns;
    float* JC = w;                       w += N * 13 * ns;
    float* XZ = w;                       w += N * 273 * ns;   // XZ[s] = d x_s / dz for s = 1 .. ns-1 (slot 0 unused)
    float* MU0 = w;                      w += N * 13;
    float* MU1 = w;                      w += N * 13;
    float* HS = w;                       w += N * 441;
    float* DT = w;                       w += N;
    float* XN = w;
    const ac_params saved = h->dp.p;
    const float inv_ns = 1.0f / (float)ns;
    const float hdt = dt * inv_ns;
    const float* hdtp = nullptr;
    const int g1 = (int)((n + kBlock - 1) / kBlock);
    if (dt_per_unit) {
        hipLaunchKernelGGL(k_scale_rows<0>, g1, kBlock, 0, st, dt_per_unit, inv_ns, n, DT);
        hdtp = DT;
    }
    rc = AC_OK;
    h->dp.p.substeps = 1;
    // forward: the sub-steps with their first-order blocks, and the chain of state sensitivities
    for (int s = 0; s < ns && rc == AC_OK; ++s) {
        const float* xs = s == 0 ? X : XS + N * 13 * s;
        float* xn = s + 1 < ns ? XS + N * 13 * (s + 1) : XN;
        h->dp.p.normalise = (s == ns - 1) ? saved.normalise : 0;  // q <- q/|q| once, after the last sub-step
        rc = sens_impl(h, xs, U, hdt, hdtp, n, blk, xn, JA + N * 169 * s, JB + N * 91 * s, JC + N * 13 * s, stream);
        if (rc == AC_OK && s + 1 < ns)
            hipLaunchKernelGGL(k_hess_chain<0>, dim3(g1, 21), kBlock, 0, st, JA + N * 169 * s, JB + N * 91 * s, JC + N * 13 * s,
                               s == 0 ? (const float*)nullptr : (const float*)(XZ + N * 273 * s), inv_ns, n, blk,
                               XZ + N * 273 * (s + 1));
    }
    // backward: adjoint of the later sub-steps, the block of each sub-step, its congruence into the caller's variables
    if (rc == AC_OK) rc = hipMemsetAsync(Hout, 0, N * 441 * sizeof(float), st) == hipSuccess ? AC_OK : AC_ERR_HIP;
    const float* mu = Lam;
    for (int s = ns - 1; s >= 0 && rc == AC_OK; --s) {
        const float* xs = s == 0 ? X : XS + N * 13 * s;
        h->dp.p.normalise = (s == ns - 1) ? saved.normalise : 0;
        rc = hess_single(h, xs, U, hdt, hdtp, mu, n, blk, HS, st);
        if (rc != AC_OK) break;
        hipLaunchKernelGGL(k_hess_accum<0>, dim3(g1, 21), kBlock, 0, st, HS,
                           s == 0 ? (const float*)nullptr : (const float*)(XZ + N * 273 * s), inv_ns, n, blk, Hout);
        if (s > 0) {
            float* mo = (mu == MU0) ? MU1 : MU0;
            hipLaunchKernelGGL(k_hess_adjoint<0>, g1, kBlock, 0, st, JA + N * 169 * s, mu, n, blk, mo);
            mu = mo;
        }
    }
    h->dp.p = saved;
    if (rc != AC_OK) return rc;
    note_launch(h, "k_step_hess (composed over sub-steps)", g1, kBlock, 0);
    AC_HIP(hipGetLastError());
    return AC_OK;
}

int ac_reserve_hess_workspace(ac_handle* h, long n) {
    AC_ENTER(h);
    if (!h || n < 0) return AC_ERR_BAD_ARG;
    const size_t need = (size_t)n * kStageFloats;
    if (need > h->hess_ws_floats) {
        if (h->d_hess_ws) (void)hipFree(h->d_hess_ws);
        h->d_hess_ws = nullptr; h->hess_ws_floats = 0;
        AC_HIP(hipMalloc((void**)&h->d_hess_ws, need * sizeof(float)));
        h->hess_ws_floats = need;
    }
    if (h->has_rev && n > 0) {  // the reverse-sweep kernel's layer states: one slot per wave of a persistent grid
        const size_t need_r = (size_t)rev_grid(h, n) * (kBlock / 64) * (size_t)rev_scratch_f32x4(h->wt, h->rev_layers - 2) * 4;
        if (need_r > h->rev_scratch_floats) {
            if (h->d_rev_scratch) (void)hipFree(h->d_rev_scratch);
            h->d_rev_scratch = nullptr; h->rev_scratch_floats = 0;
            AC_HIP(hipMalloc((void**)&h->d_rev_scratch, need_r * sizeof(float)));
            h->rev_scratch_floats = need_r;
        }
    }
    const size_t need2 = (size_t)n * hess_compose_floats(h->dp.p.substeps);  // sized for the handle's CURRENT sub-step count
    if (need2 > h->hess_ws2_floats) {
        if (h->d_hess_ws2) (void)hipFree(h->d_hess_ws2);
        h->d_hess_ws2 = nullptr; h->hess_ws2_floats = 0;
        AC_HIP(hipMalloc((void**)&h->d_hess_ws2, need2 * sizeof(float)));
        h->hess_ws2_floats = need2;
    }
    return AC_OK;
}

int ac_step_hess_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit,
                     const float* lambda, long n, float* Hout, void* stream) {
    return hess_impl(h, X, U, dt, dt_per_unit, lambda, n, n > 0 ? n : 1, Hout, stream);
}

int ac_shoot_hess_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit,
                      const float* lambda, long B, long H, float* Hout, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return hess_impl(h, X, U, dt, dt_per_unit, lambda, B * H, B > 0 ? B : 1, Hout, stream);
}

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

int ac_hess_workspace(const ac_handle* h, float** ptr, size_t* floats) {
    if (!h) return AC_ERR_BAD_ARG;
    if (ptr) *ptr = h->d_hess_ws;
    if (floats) *floats = h->hess_ws_floats;
    return AC_OK;
}

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

int ac_set_vjp_route(ac_handle* h, int route) {
    AC_ENTER(h);
    if (!h || route < AC_VJP_AUTO || route > AC_VJP_COMPOSED) return AC_ERR_BAD_ARG;
    h->vjp_route = route;
    return AC_OK;
}

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

int ac_mlp_folded_shape(const ac_handle* h, int* n_layers, int* widths) {
    if (!h || !n_layers || !widths) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    if (!h->has_mlp) return fail(AC_ERR_NO_MODEL, "no MLP installed: call ac_set_mlp first");
    *n_layers = h->wg.n_layers;
    widths[0] = h->wg.nin[0];
    for (int l = 0; l < h->wg.n_layers; ++l) widths[l + 1] = h->wg.nout[l];
    return AC_OK;
}

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

int ac_set_cgrad_grid(ac_handle* h, int max_workgroups) {
    if (!h || max_workgroups < 0) return AC_ERR_BAD_ARG;
    h->cgrad_grid = max_workgroups;
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

// ---- steady-flight trim (ac_trim.hpp) -----------------------------------------------------------------------------------------
namespace {
// the six workspace buffers each start on a 256-byte boundary, as a torch allocation would
constexpr size_t kTrimWsPad = 6 * 64;
size_t trim_ws_floats(long n) { return (size_t)n * (size_t)kTrimWsFloats + kTrimWsPad; }
float* align256(float* p) { return (float*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }
}  // namespace

int ac_trim_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "trim is defined for the fixed-wing models only");
    *floats = trim_ws_floats(n);
    return AC_OK;
}

int ac_trim_f32(ac_handle* h, const ac_trim_opts* o, const float* target, const float* Uhold, const float* Z0, int iters, long n,
                float* X, float* U, float* Z, float* R, int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !o || iters < 1 || n < 0 || (o->lateral != 0 && o->lateral != 1)) return AC_ERR_BAD_ARG;
    if (!(o->tol_v > 0.f) || !(o->tol_w > 0.f)) return fail(AC_ERR_BAD_ARG, "trim tolerances must be > 0");
    for (int j = 0; j < 6; ++j)
        if (!(o->lo[j] <= o->hi[j])) return fail(AC_ERR_BAD_ARG, "trim bounds: lo > hi (or NaN)");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, "trim is defined for the fixed-wing models only");
    if (n == 0) return AC_OK;
    if (!target || !Uhold || !Z0 || !X || !U || !Z || !R || !status) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    const size_t N = (size_t)n;
    if (!ws || ws_floats < trim_ws_floats(n))
        return fail(AC_ERR_WORKSPACE, "trim workspace too small: see ac_trim_workspace_floats");
    float* Xw = align256(ws);
    float* Uw = align256(Xw + 13 * N);
    float* Xd = align256(Uw + 7 * N);
    float* Fx = align256(Xd + 13 * N);
    float* Fu = align256(Fx + 169 * N);
    float* St = align256(Fu + 91 * N);  // ends at most ws + 350 N + 6 * 63 floats
    hipStream_t st = (hipStream_t)stream;
    const int grid = (int)((n + kTrimBlock - 1) / kTrimBlock);
    for (int k = 0; k < iters; ++k) {
        hipLaunchKernelGGL(k_trim_assemble, grid, kTrimBlock, 0, st, *o, target, Uhold, Z0, n, (int)(k == 0), Xw, Uw, St);
        AC_HIP(hipGetLastError());
        rc = deriv_sens_impl(h, Xw, Uw, n, n, Xd, Fx, Fu, stream);
        if (rc != AC_OK) return rc;
        hipLaunchKernelGGL(k_trim_update, grid, kTrimBlock, 0, st, *o, target, Uhold, Xd, Fx, Fu, n, (int)(k == iters - 1), St, X, U,
                           Z, R, status);
        AC_HIP(hipGetLastError());
    }
    note_launch(h, "k_trim_update", grid, kTrimBlock, 0);
    return AC_OK;
}

// ---- LQR about steady-flight trims (ac_lqr.hpp, lqr_inst.hip) ----------------------------------------------------------------------
namespace {
constexpr size_t kLqrWsPad = 3 * 64;  // the three workspace buffers each start on a 256-byte boundary
size_t lqr_ws_floats(long n) { return (size_t)n * (size_t)kLqrWsFloats + kLqrWsPad; }
const char* const kLqrFixedWing = "the LQR about a trim is defined for the fixed-wing models only";
}  // namespace

int ac_lqr_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    *floats = lqr_ws_floats(n);
    return AC_OK;
}

int ac_lqr_f32(ac_handle* h, const ac_lqr_opts* o, const float* X, const float* U, float dt, int iters, long n, float* Axi,
               float* Bxi, float* P, float* K, float* resid, int* status, int* used_iters, float* ws, size_t ws_floats,
               void* stream) {
    AC_ENTER(h);
    if (!h || !o || iters < 1 || n < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: dt must be finite and > 0");
    for (int i = 0; i < 12; ++i)
        if (!(o->q[i] >= 0.f) || !(o->q[i] <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: q must be finite and >= 0");
    for (int j = 0; j < 7; ++j)
        if (!(o->r[j] > 0.f) || !(o->r[j] <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "lqr: r must be finite and > 0");
    if (!(o->tol >= 0.f)) return fail(AC_ERR_BAD_ARG, "lqr: tol must be >= 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !U || !Axi || !Bxi || !P || !K || !resid || !status || !used_iters) return AC_ERR_BAD_ARG;
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < lqr_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "lqr workspace too small: see ac_lqr_workspace_floats");
    const size_t N = (size_t)n;
    float* const Xp = align256(ws);
    float* const A = align256(Xp + 13 * N);
    float* const Bm = align256(A + 169 * N);  // ends at most ws + 273 N + 3 * 63 floats
    rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    int grid = 0, lds = 0;
    AC_HIP(lqr_launch_project(X, U, Xp, A, Bm, n, Axi, Bxi, st, &grid));
    AC_HIP(lqr_launch_dare(*o, iters, Axi, Bxi, n, P, K, resid, status, used_iters, st, &grid, &lds));
    note_launch(h, "k_lqr_dare", grid, kLqrGroups * kLqrLanes, lds);
    return AC_OK;
}

int ac_lqr_gains_f32(ac_handle* h, const float* Xnom, const float* K, long n, long H, float* Kx, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || H < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0 || H == 0) return AC_OK;
    if (!Xnom || !K || !Kx) return AC_ERR_BAD_ARG;
    int grid = 0;
    AC_HIP(lqr_launch_gains(Xnom, K, n, H, Kx, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqr_gains", grid, kLqrBlock, 0);
    return AC_OK;
}

int ac_steady_error_f32(ac_handle* h, const float* X, const float* Xnom, long n, float* xi, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kLqrFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !Xnom || !xi) return AC_ERR_BAD_ARG;
    int grid = 0;
    AC_HIP(lqr_launch_error(X, Xnom, n, xi, (hipStream_t)stream, &grid));
    note_launch(h, "k_steady_error", grid, kLqrBlock, 0);
    return AC_OK;
}

// ---- extended Kalman filter over the step sensitivities (ac_ekf.hpp, ekf_inst.hip) -------------------------------------------------
namespace {
constexpr size_t kEkfWsPad = 7 * 64;  // the seven workspace buffers each start on a 256-byte boundary
size_t ekf_ws_floats(long n) { return (size_t)n * (size_t)(kEkfSensFloats + kEkfChainFloats) + kEkfWsPad; }
const char* const kEkfFixedWing = "the extended Kalman filter is defined for the fixed-wing models only";

// one step: the handle's sensitivity launch into the workspace, then k_ekf_step.  ll_in: added to this step's ll (or NULL).
int ekf_step_impl(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                  const int* mask, const float* Qd, const float* Rd, long n, const float* ll_in, float* Xo, float* Po, float* nu,
                  float* S, float* nis, float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws,
                  void* stream) {
    const size_t N = (size_t)n;
    float* const Xp = align256(ws);
    float* const A = align256(Xp + 13 * N);
    float* const Bm = align256(A + 169 * N);
    if (o->predict) {
        const int rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
        if (rc != AC_OK) return rc;
    }
    const EkfIo io{X, P, Xp, A, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
    int grid = 0, lds = 0;
    AC_HIP(ekf_launch_step(*o, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ekf_step", grid, kEkfGroups * kEkfLanes, lds);
    return AC_OK;
}

// the checks both entry points share; *go = false: nothing to do (AC_OK)
int ekf_check(ac_handle* h, const ac_ekf_opts* o, float dt, long n, long T, const float* ws, size_t ws_floats, bool* go) {
    *go = false;
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (o->predict && (!(dt > 0.f) || !(dt <= 3.0e38f))) return fail(AC_ERR_BAD_ARG, "ekf: dt must be finite and > 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0 || T == 0) return AC_OK;
    const int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < ekf_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "ekf workspace too small: see ac_ekf_workspace_floats");
    *go = true;
    return AC_OK;
}
}  // namespace

int ac_ekf_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = ekf_ws_floats(n);
    return AC_OK;
}

int ac_ekf_measure_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, long n, float* Z, void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !Z) return fail(AC_ERR_BAD_ARG, "ekf measure: X and Z must not be NULL");
    int grid = 0;
    AC_HIP(ekf_launch_measure(*o, h->dp.p.epsilon, X, n, Z, (hipStream_t)stream, &grid));
    note_launch(h, "k_ekf_measure", grid, kEkfBlock, 0);
    return AC_OK;
}

int ac_ekf_step_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                    const int* mask, const float* Qd, const float* Rd, long n, float* Xo, float* Po, float* nu, float* S, float* nis,
                    float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws, size_t ws_floats,
                    void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ekf_check(h, o, dt, n, 1, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X || !P || !Z || !Rd || !Xo || !Po || !nu || !S || !nis || !ll || !used || !status)
        return fail(AC_ERR_BAD_ARG, "ekf step: a required pointer is NULL");
    if (o->predict && (!U || !Qd)) return fail(AC_ERR_BAD_ARG, "ekf step: U and Qd are required when predict is set");
    return ekf_step_impl(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, nullptr, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, ws,
                         stream);
}

namespace {
// do two spans of floats share an element? (a NULL span shares none)
struct RtsSpan { const float* p; size_t floats; };
bool rts_overlap(const RtsSpan& a, const RtsSpan& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a0 < b0 + b.floats * sizeof(float) && b0 < a0 + a.floats * sizeof(float);
}
}  // namespace

int ac_ekf_filter_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                      const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po, float* ll, float* Xs,
                      float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* ws, size_t ws_floats, void* stream) {
    return ac_ekf_filter_rec_f32(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, nullptr,
                                 nullptr, nullptr, ws, ws_floats, stream);
}

int ac_ekf_filter_rec_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                          float* Ppreds, float* Abars, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ekf_check(h, o, dt, n, T, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    const size_t N = (size_t)n;
    float* buf[4];  // x, P | x, P behind the sensitivity outputs
    buf[0] = align256(align256(align256(align256(ws) + 13 * N) + 169 * N) + 91 * N);
    buf[1] = align256(buf[0] + 13 * N);
    buf[2] = align256(buf[1] + 144 * N);
    buf[3] = align256(buf[2] + 13 * N);  // ends at most ws + 587 N + 7 * 63 floats
    const auto step = [&](auto... a) { return ekf_step_impl(h, o, a..., ws, stream); };
    return filter_loop("ekf", o->predict, step, buf, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status,
                       Xpreds, Ppreds, Abars, stream);
}

// ---- unscented Kalman filter beside the EKF bank (ac_ukf.hpp, ukf_inst.hip) ---------------------------------------------------------
namespace {
constexpr size_t kUkfWsPad = 9 * 64;  // the nine workspace buffers each start on a 256-byte boundary
size_t ukf_ws_floats(long n) { return (size_t)n * (size_t)(kUkfInstFloats + kEkfChainFloats) + kUkfWsPad; }

// the workspace: points [13][25 n] | U [7][25 n] | images [13][25 n] | L [144][n] | flag [n] | the filter's two (x, P) pairs
struct UkfWs {
    float *Xw, *Uw, *Fw, *Lw;
    int* flag;
    float* buf[4];
    UkfWs(float* ws, size_t N) {
        Xw = align256(ws);
        Uw = align256(Xw + 13 * kUkfPts * N);
        Fw = align256(Uw + 7 * kUkfPts * N);
        Lw = align256(Fw + 13 * kUkfPts * N);
        flag = (int*)align256(Lw + 144 * N);
        buf[0] = align256((float*)flag + N);
        buf[1] = align256(buf[0] + 13 * N);
        buf[2] = align256(buf[1] + 144 * N);
        buf[3] = align256(buf[2] + 13 * N);  // ends at most ws + 1284 N + 9 * 63 floats
    }
};

// one step: k_ukf_sigma, the handle's forward step over the 25 n units, k_ukf_update.  ll_in: added to this step's ll (or NULL).
int ukf_step_impl(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                  const int* mask, const float* Qd, const float* Rd, long n, const float* ll_in, float* Xo, float* Po, float* nu,
                  float* S, float* nis, float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws,
                  void* stream) {
    const UkfWs w(ws, (size_t)n);
    const UkfWeights wt = ukf_weights(o->kappa);
    int grid = 0, lds = 0;
    if (o->predict) {
        const UkfSigIo sio{X, P, U, w.Xw, w.Uw, w.Lw, w.flag, n};
        AC_HIP(ukf_launch_sigma(wt, sio, (hipStream_t)stream, &grid, &lds));
        note_launch(h, "k_ukf_sigma", grid, kUkfGroups * kEkfLanes, lds);
        const int rc = step_impl(h, w.Xw, w.Uw, dt, nullptr, kUkfPts * n, kUkfPts * n, w.Fw, stream);
        if (rc != AC_OK) return rc;
    }
    const UkfIo io{X, P, w.Fw, w.Lw, w.flag, Z, Qd, Rd, mask, ll_in, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, n};
    AC_HIP(ukf_launch_update(*o, wt, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ukf_update", grid, kUkfGroups * kEkfLanes, lds);
    return AC_OK;
}

// the checks the entry points share; *go = false: nothing to do (AC_OK)
int ukf_check(ac_handle* h, const ac_ukf_opts* o, float dt, long n, long T, const float* ws, size_t ws_floats, bool* go) {
    *go = false;
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (o->predict && (!(dt > 0.f) || !(dt <= 3.0e38f))) return fail(AC_ERR_BAD_ARG, "ukf: dt must be finite and > 0");
    if (!(o->kappa >= 0.f) || !(o->kappa <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "ukf: kappa must be finite and >= 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0 || T == 0) return AC_OK;
    if (n > 0x7fffffffL / (kUkfPts * 13)) return fail(AC_ERR_BAD_ARG, "ukf: 25 n exceeds the step launch");
    const int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < ukf_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "ukf workspace too small: see ac_ukf_workspace_floats");
    *go = true;
    return AC_OK;
}
}  // namespace

int ac_ukf_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = ukf_ws_floats(n);
    return AC_OK;
}

int ac_ukf_step_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                    const int* mask, const float* Qd, const float* Rd, long n, float* Xo, float* Po, float* nu, float* S, float* nis,
                    float* ll, int* used, int* status, float* Xpred, float* Ppred, float* Abar, float* ws, size_t ws_floats,
                    void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ukf_check(h, o, dt, n, 1, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X || !P || !Z || !Rd || !Xo || !Po || !nu || !S || !nis || !ll || !used || !status)
        return fail(AC_ERR_BAD_ARG, "ukf step: a required pointer is NULL");
    if (o->predict && (!U || !Qd)) return fail(AC_ERR_BAD_ARG, "ukf step: U and Qd are required when predict is set");
    return ukf_step_impl(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, nullptr, Xo, Po, nu, S, nis, ll, used, status, Xpred, Ppred, Abar, ws,
                         stream);
}

int ac_ukf_filter_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt, const float* Z,
                      const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po, float* ll, float* Xs,
                      float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* ws, size_t ws_floats, void* stream) {
    return ac_ukf_filter_rec_f32(h, o, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status, nullptr,
                                 nullptr, nullptr, ws, ws_floats, stream);
}

int ac_ukf_filter_rec_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds,
                          float* Ppreds, float* Abars, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ukf_check(h, o, dt, n, T, ws, ws_floats, &go);
    if (rc != AC_OK || !go) return rc;
    const UkfWs w(ws, (size_t)n);
    const auto step = [&](auto... a) { return ukf_step_impl(h, o, a..., ws, stream); };
    return filter_loop("ukf", o->predict, step, w.buf, X, P, U, dt, Z, mask, Qd, Rd, n, T, Xo, Po, ll, Xs, Ps, nu, S, nis, used, status,
                       Xpreds, Ppreds, Abars, stream);
}

// ---- the loop closed through the estimator (ac_lqg.hpp, lqg_inst.hip) ---------------------------------------------------------------
namespace {
constexpr long kLqgLoopFloats = 2 * 13 + 2 * 13 + 2 * 144 + 7 + 15 + 1;  // truth x2 | x^ x2 | P x2 | u | z | mask per instance
constexpr size_t kLqgWsPad = 10 * 64;  // the loop's nine buffers and the estimator's workspace each start on a 256-byte boundary
size_t lqg_est_floats(int estimator, long n) { return estimator == AC_EST_UKF ? ukf_ws_floats(n) : ekf_ws_floats(n); }
size_t lqg_ws_floats(int estimator, long n) { return lqg_est_floats(estimator, n) + (size_t)n * (size_t)kLqgLoopFloats + kLqgWsPad; }

bool lqg_sense_opts_ok(const ac_sense_opts* o) {
    for (int j = 0; j < kLqgGroups; ++j)
        if (o->period[j] < 1 || !(o->dropout[j] >= 0.f) || !(o->dropout[j] < 1.f)) return false;
    return true;
}
bool lqg_limits_ok(const ac_ilqr_cost* c) {
    for (int i = 0; i < 7; ++i)
        if (!(c->u_min[i] <= c->u_max[i])) return false;  // (false for a NaN bound)
    return true;
}
LqgLimits lqg_limits(const ac_ilqr_cost* c) {
    LqgLimits l;
    memcpy(l.u_min, c->u_min, sizeof(l.u_min));
    memcpy(l.u_max, c->u_max, sizeof(l.u_max));
    return l;
}
// the checks every entry point here shares; *go = false: nothing to do (AC_OK)
int lqg_check(ac_handle* h, long n, bool* go) {
    *go = false;
    if (!h) return AC_ERR_BAD_ARG;
    if (n < 0) return fail(AC_ERR_BAD_ARG, "lqg: n must be >= 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *go = n > 0;
    return AC_OK;
}
}  // namespace

int ac_sense_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev, const float* X, const float* sigma_r, long n,
                 float* Z, int* mask, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!o || !lqg_sense_opts_ok(o)) return fail(AC_ERR_BAD_ARG, "sense: period must be >= 1 and dropout in [0, 1)");
    if (!go) return AC_OK;
    if (!X || !sigma_r || !Z || !mask) return fail(AC_ERR_BAD_ARG, "sense: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_sense(*o, h->dp.p.epsilon, step, step_dev, X, sigma_r, n, Z, mask, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_disturb_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev, const float* X, const float* sigma_q, long n,
                   float* Xo, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!o) return fail(AC_ERR_BAD_ARG, "disturb: the options are NULL");
    if (!go) return AC_OK;
    if (!X || !sigma_q || !Xo) return fail(AC_ERR_BAD_ARG, "disturb: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_disturb(*o, step, step_dev, X, sigma_q, n, Xo, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_policy_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* Fb, const float* Xnom, const float* Unom, const float* Kx,
                  long n, float* U, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK) return rc;
    if (!limits || !lqg_limits_ok(limits)) return fail(AC_ERR_BAD_ARG, "policy: limits with u_min <= u_max are required");
    if (!go) return AC_OK;
    if (!Fb || !Xnom || !Unom || !Kx || !U) return fail(AC_ERR_BAD_ARG, "policy: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_control(lqg_limits(limits), Fb, Xnom, Unom, Kx, n, U, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_control", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_estimate_score_f32(ac_handle* h, const float* X, const float* Xhat, const float* P, long n, float* e, float* nees, int* status,
                          void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = lqg_check(h, n, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X || !Xhat || !P || !e || !nees || !status) return fail(AC_ERR_BAD_ARG, "estimate score: a required pointer is NULL");
    int grid = 0;
    AC_HIP(lqg_launch_score(X, Xhat, P, n, e, nees, status, (hipStream_t)stream, &grid));
    note_launch(h, "k_lqg_score", grid, kLqgBlock, 0);
    return AC_OK;
}

int ac_lqg_workspace_floats(const ac_handle* h, int estimator, long n, size_t* floats) {
    if (!h || !floats || n < 0 || (estimator != AC_EST_EKF && estimator != AC_EST_UKF)) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = lqg_ws_floats(estimator, n);
    return AC_OK;
}

int ac_lqg_rollout_f32(ac_handle* h, const ac_lqg_opts* o, const ac_sense_opts* s, const ac_ilqr_cost* limits, const float* X0,
                       const float* Xhat0, const float* P0, const float* Xnom, const float* Unom, const float* Kx, const float* Qd,
                       const float* Rd, const float* sigma_q, const float* sigma_r, float dt, long n, long T, float* Xo, float* Po,
                       float* Xtrue, float* Xhat, float* U, float* Ps, float* Z, int* mask, float* nis, float* nees, int* used,
                       int* est_status, int* score_status, float* err, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h) return AC_ERR_BAD_ARG;
    if (!o || !s || !limits || n < 0 || T < 0) return fail(AC_ERR_BAD_ARG, "lqg: NULL options or limits, n < 0 or T < 0");
    if ((long long)o->step0 + (long long)T > 0x7fffffffLL) return fail(AC_ERR_BAD_ARG, "lqg: step0 + T exceeds the 32-bit step index");
    if (o->estimator != AC_EST_EKF && o->estimator != AC_EST_UKF) return fail(AC_ERR_BAD_ARG, "lqg: unknown estimator");
    if (o->feedback != AC_FB_ESTIMATE && o->feedback != AC_FB_TRUTH) return fail(AC_ERR_BAD_ARG, "lqg: unknown feedback");
    if (!lqg_sense_opts_ok(s)) return fail(AC_ERR_BAD_ARG, "lqg: period must be >= 1 and dropout in [0, 1)");
    if (!lqg_limits_ok(limits)) return fail(AC_ERR_BAD_ARG, "lqg: limits need u_min <= u_max");
    const bool ukf = o->estimator == AC_EST_UKF;
    const ac_ekf_opts eo{{s->mag_ned[0], s->mag_ned[1], s->mag_ned[2]}, 1};
    const ac_ukf_opts uo{{s->mag_ned[0], s->mag_ned[1], s->mag_ned[2]}, 1, ukf ? o->kappa : 0.f};
    // the estimator's own checks (dt, kappa, the quadrotor, the model, n == 0 or T == 0), against its part of the workspace
    bool go = false;
    const size_t est_floats = lqg_est_floats(o->estimator, n);
    const bool ws_ok = ws && ws_floats >= lqg_ws_floats(o->estimator, n);
    int rc = ukf ? ukf_check(h, &uo, dt, n, T, ws_ok ? ws : nullptr, est_floats, &go) : ekf_check(h, &eo, dt, n, T, ws_ok ? ws : nullptr, est_floats, &go);
    if (rc == AC_ERR_WORKSPACE) return fail(AC_ERR_WORKSPACE, "lqg workspace too small: see ac_lqg_workspace_floats");
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !Xhat0 || !P0 || !Xnom || !Unom || !Kx || !Qd || !Rd || !sigma_r || !Xo || !Po)
        return fail(AC_ERR_BAD_ARG, "lqg: a required pointer is NULL");
    const size_t N = (size_t)n;
    hipStream_t st = (hipStream_t)stream;
    // the loop's buffers behind the estimator's workspace
    float* xt[2];
    float* xh[2];
    float* pp[2];
    xt[0] = align256(ws + est_floats);
    xt[1] = align256(xt[0] + 13 * N);
    xh[0] = align256(xt[1] + 13 * N);
    xh[1] = align256(xh[0] + 13 * N);
    pp[0] = align256(xh[1] + 13 * N);
    pp[1] = align256(pp[0] + 144 * N);
    float* const ub = align256(pp[1] + 144 * N);
    float* const zb = align256(ub + 7 * N);
    int* const mb = (int*)align256(zb + 15 * N);  // ends at most ws + est_floats + 363 N + 9 * 63 floats
    const LqgLimits lim = lqg_limits(limits);
    const bool score = err || nees || score_status;
    auto copy = [&](void* dst, const void* src, size_t floats) { return hipMemcpyAsync(dst, src, floats * sizeof(float), hipMemcpyDeviceToDevice, st); };
    if (Xtrue) AC_HIP(copy(Xtrue, X0, 13 * N));
    if (Xhat) AC_HIP(copy(Xhat, Xhat0, 13 * N));
    const float *xt_in = X0, *xh_in = Xhat0, *p_in = P0;
    int grid = 0;
    for (long t = 0; t < T; ++t) {
        const size_t k = (size_t)t;
        const bool last = t == T - 1;
        float* const xt_o = xt[t & 1];
        float* const xh_o = last ? Xo : xh[t & 1];
        float* const p_o = last ? Po : pp[t & 1];
        float* const u_k = U ? U + k * 7 * N : ub;
        float* const z_k = Z ? Z + k * 15 * N : zb;
        int* const m_k = mask ? mask + k * N : mb;
        // 1. the control law on the estimate (or the truth)
        AC_HIP(lqg_launch_control(lim, o->feedback == AC_FB_TRUTH ? xt_in : xh_in, Xnom + k * 13 * N, Unom + k * 7 * N, Kx + k * 91 * N, n,
                                  u_k, st, &grid));
        note_launch(h, "k_lqg_control", grid, kLqgBlock, 0);
        // 2. the truth: the handle's forward step, then the process noise of step step0 + k
        rc = step_impl(h, xt_in, u_k, dt, nullptr, n, n, xt_o, stream);
        if (rc != AC_OK) return rc;
        if (sigma_q) {
            AC_HIP(lqg_launch_disturb(*s, o->step0 + (int)t, nullptr, xt_o, sigma_q, n, xt_o, st, &grid));
            note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
        }
        if (Xtrue) AC_HIP(copy(Xtrue + (k + 1) * 13 * N, xt_o, 13 * N));
        // 3. the sensors at step step0 + k + 1
        AC_HIP(lqg_launch_sense(*s, h->dp.p.epsilon, o->step0 + (int)t + 1, nullptr, xt_o, sigma_r, n, z_k, m_k, st, &grid));
        note_launch(h, "k_lqg_sense", grid, kLqgBlock, 0);
        // 4. the estimator's own step
        float* const nis_k = nis ? nis + k * N : nullptr;
        int* const used_k = used ? used + k * N : nullptr;
        int* const st_k = est_status ? est_status + k * N : nullptr;
        rc = ukf ? ukf_step_impl(h, &uo, xh_in, p_in, u_k, dt, z_k, m_k, Qd, Rd, n, nullptr, xh_o, p_o, nullptr, nullptr, nis_k, nullptr,
                                 used_k, st_k, nullptr, nullptr, nullptr, ws, stream)
                 : ekf_step_impl(h, &eo, xh_in, p_in, u_k, dt, z_k, m_k, Qd, Rd, n, nullptr, xh_o, p_o, nullptr, nullptr, nis_k, nullptr,
                                 used_k, st_k, nullptr, nullptr, nullptr, ws, stream);
        if (rc != AC_OK) return rc;
        if (Xhat) AC_HIP(copy(Xhat + (k + 1) * 13 * N, xh_o, 13 * N));
        if (Ps) AC_HIP(copy(Ps + k * 144 * N, p_o, 144 * N));
        // 5. the estimate against the truth
        if (score) {
            AC_HIP(lqg_launch_score(xt_o, xh_o, p_o, n, err ? err + k * 12 * N : nullptr, nees ? nees + k * N : nullptr,
                                    score_status ? score_status + k * N : nullptr, st, &grid));
            note_launch(h, "k_lqg_score", grid, kLqgBlock, 0);
        }
        xt_in = xt_o;
        xh_in = xh_o;
        p_in = p_o;
    }
    return AC_OK;
}

// ---- RTS smoother over the EKF trace (ac_rts.hpp, rts_inst.hip) ---------------------------------------------------------------------
int ac_ekf_smooth_f32(ac_handle* h, const float* X0, const float* P0, const float* Xf, const float* Pf, const float* Xpred,
                      const float* Ppred, const float* Abar, long n, long T, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Cg,
                      int* status, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    const int given = (X0 != nullptr) + (P0 != nullptr) + (Xs0 != nullptr) + (Ps0 != nullptr);
    if (given != 0 && given != 4) return fail(AC_ERR_BAD_ARG, "ekf smooth: X0, P0, Xs0, Ps0 go together (all or none)");
    if (n == 0 || T == 0) return AC_OK;
    if (!Xf || !Pf || !Xpred || !Ppred || !Abar || !Xs || !Ps || !status)
        return fail(AC_ERR_BAD_ARG, "ekf smooth: a required pointer is NULL");
    const size_t N = (size_t)n, K = (size_t)T;
    const RtsSpan in[] = {{X0, 13 * N}, {P0, 144 * N}, {Xf, K * 13 * N}, {Pf, K * 144 * N}, {Xpred, K * 13 * N}, {Ppred, K * 144 * N},
                          {Abar, K * 144 * N}};
    const RtsSpan out[] = {{Xs, K * 13 * N}, {Ps, K * 144 * N}, {Xs0, 13 * N}, {Ps0, 144 * N}, {Cg, K * 144 * N}};
    for (const RtsSpan& a : out)
        for (const RtsSpan& b : in)
            if (rts_overlap(a, b)) return fail(AC_ERR_BAD_ARG, "ekf smooth: an output overlaps an input");
    const RtsIo io{X0, P0, Xf, Pf, Xpred, Ppred, Abar, Xs, Ps, Xs0, Ps0, Cg, status, n, T};
    int grid = 0, lds = 0;
    AC_HIP(rts_launch_smooth(io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ekf_smooth", grid, kRtsGroups * kEkfLanes, lds);
    return AC_OK;
}

// ---- flight modes: batched eigenvalues of the trim linearisation (ac_eig.hpp, modes_inst.hip) ---------------------------------------
namespace {
constexpr size_t kModesWsPad = 5 * 64;  // the five workspace buffers each start on a 256-byte boundary
size_t modes_ws_floats(long n) { return (size_t)n * (size_t)kModesWsFloats + kModesWsPad; }
const char* const kModesFixedWing = "the flight modes about a trim are defined for the fixed-wing models only";
bool modes_overlap(const RtsSpan* out, int n_out, const RtsSpan* in, int n_in) {
    for (int a = 0; a < n_out; ++a)
        for (int b = 0; b < n_in; ++b)
            if (rts_overlap(out[a], in[b])) return true;
    return false;
}
}  // namespace

int ac_eig_f32(ac_handle* h, const float* M, int m, int max_iters, long n, float* wr, float* wi, int* status, int* iters,
               void* stream) {
    AC_ENTER(h);
    if (!h || n < 0) return AC_ERR_BAD_ARG;
    if (m < 1 || m > kEigMaxM) return fail(AC_ERR_BAD_ARG, "eig: m must be 1 .. 13");
    if (max_iters < 0) return fail(AC_ERR_BAD_ARG, "eig: max_iters must be >= 0 (0: 30)");
    if (n == 0) return AC_OK;
    if (!M || !wr || !wi || !status) return fail(AC_ERR_BAD_ARG, "eig: a required pointer is NULL");
    const size_t N = (size_t)n, mm = (size_t)m;
    const RtsSpan in[] = {{M, mm * mm * N}};
    const RtsSpan out[] = {{wr, mm * N}, {wi, mm * N}, {(const float*)status, N}, {(const float*)iters, N}};
    if (modes_overlap(out, 4, in, 1)) return fail(AC_ERR_BAD_ARG, "eig: an output overlaps an input");
    int grid = 0, lds = 0;
    AC_HIP(eig_launch(M, m, max_iters ? max_iters : kEigDefaultIters, n, wr, wi, status, iters, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_eig", grid, eig_lanes(m), lds);
    return AC_OK;
}

int ac_modes_workspace_floats(const ac_handle* h, long n, size_t* floats) {
    if (!h || !floats || n < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kModesFixedWing);
    *floats = modes_ws_floats(n);
    return AC_OK;
}

int ac_modes_f32(ac_handle* h, const ac_modes_opts* o, const float* X, const float* U, float dt, const float* K, long n, float* Axi,
                 float* Bxi, float* wr, float* wi, float* sigma, float* omega, int* status, int* iters, float* ws, size_t ws_floats,
                 void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "modes: dt must be finite and > 0");
    if (o->max_iters < 0) return fail(AC_ERR_BAD_ARG, "modes: max_iters must be >= 0 (0: 30)");
    const unsigned coords = o->coords ? o->coords : kModesFlight;
    if ((coords & kModesFlight) != kModesFlight || (coords >> 12) != 0u)
        return fail(AC_ERR_BAD_ARG, "modes: coords must keep the chart coordinates 3-7 and 9-11 and set no bit >= 12");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kModesFixedWing);
    if (n == 0) return AC_OK;
    if (!X || !U || !wr || !wi || !sigma || !omega || !status) return fail(AC_ERR_BAD_ARG, "modes: a required pointer is NULL");
    int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    if (!ws || ws_floats < modes_ws_floats(n)) return fail(AC_ERR_WORKSPACE, "modes workspace too small: see ac_modes_workspace_floats");
    const size_t N = (size_t)n;
    const RtsSpan in[] = {{X, 13 * N}, {U, 7 * N}, {K, 84 * N}};
    const RtsSpan out[] = {{Axi, 144 * N}, {Bxi, 84 * N}, {wr, 12 * N}, {wi, 12 * N}, {sigma, 12 * N}, {omega, 12 * N},
                           {(const float*)status, N}, {(const float*)iters, N}, {ws, ws_floats}};
    if (modes_overlap(out, 9, in, 3)) return fail(AC_ERR_BAD_ARG, "modes: an output overlaps an input");
    float* const Xp = align256(ws);
    float* const A = align256(Xp + 13 * N);
    float* const Bm = align256(A + 169 * N);
    float* const Aw = align256(Bm + 91 * N);
    float* const Bw = align256(Aw + 144 * N);  // ends at most ws + 501 N + 5 * 63 floats
    if (!Axi) Axi = Aw;
    if (!Bxi) Bxi = Bw;
    rc = sens_impl(h, X, U, dt, nullptr, n, n, Xp, A, Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    int grid = 0, lds = 0, m = 0;
    for (int i = 0; i < 12; ++i) m += (int)((coords >> i) & 1u);
    AC_HIP(lqr_launch_project(X, U, Xp, A, Bm, n, Axi, Bxi, st, &grid));
    AC_HIP(modes_launch_eig(Axi, Bxi, K, coords, m, o->max_iters ? o->max_iters : kEigDefaultIters, dt, n, wr, wi, sigma, omega,
                            status, iters, st, &grid, &lds));
    note_launch(h, "k_modes_eig", grid, eig_lanes(m), lds);
    return AC_OK;
}

// ---- EM statistics for the noise variances of the EKF (ac_em.hpp, em_inst.hip) --------------------------------------------------------
namespace {
constexpr size_t kEmWsPad = 2 * 64;  // the two workspace buffers each start on a 256-byte boundary
// [chunks][27][n] float64, then [chunks][16][n] int32
size_t em_ws_floats(long n, long T) { return (size_t)em_chunks(T) * (size_t)n * (size_t)(2 * kEmRows + kEmCounts) + kEmWsPad; }
}  // namespace

int ac_ekf_em_workspace_floats(const ac_handle* h, long n, long T, size_t* floats) {
    if (!h || !floats || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    *floats = em_ws_floats(n, T);
    return AC_OK;
}

int ac_ekf_em_f32(ac_handle* h, const ac_ekf_em_opts* o, const float* Xpred, const float* Ppred, const float* Xs, const float* Ps,
                  const float* Z, const int* used, const float* Qd, const float* Rd, long n, long T, float* Qsum, float* Rsum,
                  int* nq, int* nr, int* status, float* Qn, float* Rn, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (!(o->floor_rel >= 0.f) || !(o->floor_rel <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "ekf em: floor_rel must be finite and >= 0 (0: 1e-4)");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kEkfFixedWing);
    if (n == 0) return AC_OK;
    if (!Qd || !Rd || !Qsum || !Rsum || !nq || !nr || (T > 0 && (!Xpred || !Ppred || !Xs || !Ps || !Z || !used || !status)))
        return fail(AC_ERR_BAD_ARG, "ekf em: a required pointer is NULL");
    const size_t N = (size_t)n, K = (size_t)T;
    const long gb = (n + kEmGroups - 1) / kEmGroups;
    if (em_chunks(T) > 2147483647L / gb || (long)kEmRows * n / kEmBlock >= 2147483647L)
        return fail(AC_ERR_BAD_ARG, "ekf em: n * T exceeds the launch dimension");
    if (!ws || ws_floats < em_ws_floats(n, T)) return fail(AC_ERR_WORKSPACE, "ekf em workspace too small: see ac_ekf_em_workspace_floats");
    const RtsSpan in[] = {{Xpred, K * 13 * N}, {Ppred, K * 144 * N}, {Xs, K * 13 * N}, {Ps, K * 144 * N}, {Z, K * 15 * N},
                          {(const float*)used, K * N}, {Qd, 12 * N}, {Rd, 15 * N}};
    const RtsSpan out[] = {{Qsum, 12 * N}, {Rsum, 15 * N}, {(const float*)nq, N}, {(const float*)nr, 15 * N},
                           {(const float*)status, K * N}, {Qn, 12 * N}, {Rn, 15 * N}, {ws, ws_floats}};
    if (modes_overlap(out, 8, in, 8)) return fail(AC_ERR_BAD_ARG, "ekf em: an output overlaps an input");
    double* const part = (double*)align256(ws);
    int* const cnt = (int*)align256((float*)part + (size_t)em_chunks(T) * 2 * kEmRows * N);  // ends at most ws + 70 chunks N + 2 * 63 floats
    EmIo io{Xpred, Ppred, Xs, Ps, Z, used, Qd, Rd, part, cnt, Qsum, Rsum, nq, nr, status, Qn, Rn, {o->mag_ned[0], o->mag_ned[1], o->mag_ned[2]},
            h->dp.p.epsilon, o->floor_rel, n, T};
    int grid = 0, lds = 0;
    AC_HIP(em_launch(io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, T > 0 ? "k_ekf_em_nodes" : "k_ekf_em_reduce", grid, kEmGroups * kEkfLanes, lds);
    return AC_OK;
}

// ---- iterated extended Kalman smoother (ac_ieks.hpp, ieks_inst.hip) -----------------------------------------------------------------
namespace {
// The workspace: F [T][13][n] | A [T][169][n] | B [T][91][n] (the pass) | the cost's region for `cols` columns: F [T][13][cols] |
// partial sums [chunks][2][cols] float64 | status [chunks][cols] int32 | then the solve's own: Xc [T+1][13][cols] | Uc [T][7][cols] |
// Jc [cols] | stc [cols] int32 | the smoother's status [T][n] int32.  Every buffer starts on a 256-byte boundary.
struct IeksCostWs {
    float* Fc;
    double* part;
    int* pst;
    float* end;
    IeksCostWs(float* ws, size_t cols, size_t K) {
        Fc = align256(ws);
        part = (double*)align256(Fc + K * 13 * cols);
        pst = (int*)align256((float*)part + (size_t)ieks_chunks((long)K) * 4 * cols);
        end = (float*)pst + (size_t)ieks_chunks((long)K) * cols;
    }
};
struct IeksWs {
    float *F, *A, *Bm, *cost, *Xc, *Uc, *Jc, *end;
    int *stc, *rst;
    float* pass_end;
    IeksWs(float* ws, size_t N, size_t K, size_t C) {
        const size_t cols = N * (C ? C : 1);
        F = align256(ws);
        A = align256(F + K * 13 * N);
        Bm = align256(A + K * 169 * N);
        pass_end = Bm + K * 91 * N;
        cost = align256(pass_end);
        Xc = align256(IeksCostWs(cost, cols, K).end);
        Uc = align256(Xc + (K + 1) * 13 * cols);
        Jc = align256(Uc + K * 7 * cols);
        stc = (int*)align256(Jc + cols);
        rst = (int*)align256((float*)stc + cols);
        end = (float*)rst + K * N;
    }
};
constexpr size_t kIeksWsPad = 11 * 64;
size_t ieks_pass_floats(long n, long T) { return (size_t)(IeksWs(nullptr, (size_t)n, (size_t)T, 1).pass_end - (float*)nullptr) + 3 * 64; }
size_t ieks_cost_floats(long cols, long T) { return (size_t)(IeksCostWs(nullptr, (size_t)cols, (size_t)T).end - (float*)nullptr) + 3 * 64; }
size_t ieks_ws_floats(long n, long T, int C) { return (size_t)(IeksWs(nullptr, (size_t)n, (size_t)T, (size_t)C).end - (float*)nullptr) + kIeksWsPad; }
const char* const kIeksFixedWing = "the iterated Kalman smoother is defined for the fixed-wing models only";

int ieks_ladder(const float* ladder, int candidates, IeksLadder* lad) {
    if (!ladder || candidates < 1 || candidates > kIeksMaxCand) return fail(AC_ERR_BAD_ARG, "ieks: the ladder has 1 .. 8 values");
    lad->count = candidates;
    for (int c = 0; c < kIeksMaxCand; ++c) lad->a[c] = 0.f;
    for (int c = 0; c < candidates; ++c) {
        if (!(ladder[c] > 0.f) || !(ladder[c] <= 1.0f)) return fail(AC_ERR_BAD_ARG, "ieks: the ladder's values must lie in (0, 1]");
        lad->a[c] = ladder[c];
    }
    return AC_OK;
}

// the checks the entry points share; *go = false: nothing to do (AC_OK)
int ieks_check(ac_handle* h, const ac_ekf_opts* o, float dt, long n, long T, bool* go) {
    *go = false;
    if (!h || !o || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (!(dt > 0.f) || !(dt <= 3.0e38f)) return fail(AC_ERR_BAD_ARG, "ieks: dt must be finite and > 0");
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    if (n == 0 || T == 0) return AC_OK;
    if (T + 1 > 2147483647L / ((n * kIeksMaxCand + kIeksBlock - 1) / kIeksBlock + 1)) return fail(AC_ERR_BAD_ARG, "ieks: n * T exceeds the launch dimension");
    const int rc = model_ready(h);
    if (rc != AC_OK) return rc;
    *go = true;
    return AC_OK;
}

int ieks_pass_impl(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xbar, const float* U, float dt,
                   const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps, float* ll,
                   float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars, float* ws,
                   void* stream) {
    const IeksWs w(ws, (size_t)n, (size_t)T, 1);
    const int rc = sens_impl(h, Xbar, U, dt, nullptr, n * T, n, w.F, w.A, w.Bm, nullptr, stream);
    if (rc != AC_OK) return rc;
    const IeksIo io{X0, P0, Xbar, w.F, w.A, Z, Qd, Rd, mask, Xs, Ps, ll, nu, S, nis, used, status, Xpreds, Ppreds, Abars, n, T};
    int grid = 0, lds = 0;
    AC_HIP(ieks_launch_filter(*o, h->dp.p.epsilon, io, (hipStream_t)stream, &grid, &lds));
    note_launch(h, "k_ieks_filter", grid, kIeksGroups * kEkfLanes, lds);
    return AC_OK;
}

// wsc: a region of at least ieks_cost_floats(reps n, T) floats
int ieks_cost_impl(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xt, const float* Ut, float dt,
                   const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long reps, long T, float* J, float* Jprior,
                   float* Jproc, float* Jmeas, int* status, float* wsc, void* stream) {
    const long cols = n * reps;
    const IeksCostWs w(wsc, (size_t)cols, (size_t)T);
    const int rc = step_impl(h, Xt, Ut, dt, nullptr, cols * T, cols, w.Fc, stream);
    if (rc != AC_OK) return rc;
    const IeksCostIo io{X0, P0, Xt, w.Fc, Z, Qd, Rd, mask, w.part, w.pst, J, Jprior, Jproc, Jmeas, status,
                        {o->mag_ned[0], o->mag_ned[1], o->mag_ned[2]}, h->dp.p.epsilon, n, reps, T};
    int grid = 0;
    AC_HIP(ieks_launch_cost(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_cost_nodes", grid, kIeksBlock, 0);
    return AC_OK;
}
}  // namespace

int ac_ieks_workspace_floats(const ac_handle* h, long n, long T, int candidates, size_t* floats) {
    if (!h || !floats || n < 0 || T < 0 || candidates < 0 || candidates > kIeksMaxCand) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    *floats = ieks_ws_floats(n, T, candidates);
    return AC_OK;
}

int ac_ieks_pass_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xbar, const float* U, float dt,
                     const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps, float* ll,
                     float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars, float* ws,
                     size_t ws_floats, void* stream) {
    AC_ENTER(h);
    bool go = false;
    const int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xbar || !U || !Z || !Qd || !Rd || !Xs || !Ps || !Xpreds || !Ppreds || !Abars)
        return fail(AC_ERR_BAD_ARG, "ieks pass: a required pointer is NULL");
    if (!ws || ws_floats < ieks_pass_floats(n, T)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    return ieks_pass_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, T, Xs, Ps, ll, nu, S, nis, used, status, Xpreds, Ppreds, Abars,
                          ws, stream);
}

int ac_ieks_cost_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xtraj, const float* Utraj,
                     float dt, const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long reps, long T, float* J,
                     float* Jprior, float* Jproc, float* Jmeas, int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (reps < 1 || reps > kIeksMaxCand) return fail(AC_ERR_BAD_ARG, "ieks cost: reps must be 1 .. 8");
    bool go = false;
    const int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xtraj || !Utraj || !Z || !Qd || !Rd || !J || !status)
        return fail(AC_ERR_BAD_ARG, "ieks cost: a required pointer is NULL");
    if (!ws || ws_floats < ieks_cost_floats(n * reps, T)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    return ieks_cost_impl(h, o, X0, P0, Xtraj, Utraj, dt, Z, mask, Qd, Rd, n, reps, T, J, Jprior, Jproc, Jmeas, status, ws, stream);
}

int ac_ieks_candidates_f32(ac_handle* h, const float* Xbar, const float* Xs0, const float* Xs, const float* U, const float* ladder,
                           int candidates, long n, long T, float* Xc, float* Uc, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    IeksLadder lad;
    const int rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK) return rc;
    if (n == 0 || T == 0) return AC_OK;
    if (!Xbar || !Xs0 || !Xs || !U || !Xc || !Uc) return fail(AC_ERR_BAD_ARG, "ieks candidates: a required pointer is NULL");
    const IeksCandIo io{Xbar, Xs0, Xs, U, Xc, Uc, lad, n, T};
    int grid = 0;
    AC_HIP(ieks_launch_candidates(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_candidates", grid, kIeksBlock, 0);
    return AC_OK;
}

int ac_ieks_accept_f32(ac_handle* h, const float* Jcur, const float* Jc, const int* stc, const float* Xc, const float* ladder,
                       int candidates, long n, long T, float* Xbar, float* alpha, float* Jout, int* status, void* stream) {
    AC_ENTER(h);
    if (!h || n < 0 || T < 0) return AC_ERR_BAD_ARG;
    if (h->dp.p.model_kind == AC_MODEL_QUAD) return fail(AC_ERR_UNSUPPORTED, kIeksFixedWing);
    IeksLadder lad;
    const int rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK) return rc;
    if (n == 0 || T == 0) return AC_OK;
    if (!Jcur || !Jc || !stc || !Xc || !Xbar || !alpha || !Jout || !status) return fail(AC_ERR_BAD_ARG, "ieks accept: a required pointer is NULL");
    if (rts_overlap({Jcur, (size_t)n}, {Jout, (size_t)n})) return fail(AC_ERR_BAD_ARG, "ieks accept: Jout overlaps Jcur");
    const IeksAcceptIo io{Jcur, Jc, stc, Xc, Xbar, alpha, Jout, status, lad, n, T};
    int grid = 0;
    AC_HIP(ieks_launch_accept(io, (hipStream_t)stream, &grid));
    note_launch(h, "k_ieks_accept", grid, kIeksBlock, 0);
    return AC_OK;
}

int ac_ieks_solve_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, float* Xbar, const float* U, float dt,
                      const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, int iters, const float* ladder,
                      int candidates, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Xf, float* Pf, float* ll, float* nu, float* S,
                      float* nis, int* used, int* fstatus, float* Xpreds, float* Ppreds, float* Abars, float* cost, float* alpha,
                      int* status, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    if (iters < 0) return fail(AC_ERR_BAD_ARG, "ieks solve: iters must be >= 0");
    bool go = false;
    int rc = ieks_check(h, o, dt, n, T, &go);
    if (rc != AC_OK) return rc;
    IeksLadder lad;
    rc = ieks_ladder(ladder, candidates, &lad);
    if (rc != AC_OK || !go) return rc;
    if (!X0 || !P0 || !Xbar || !U || !Z || !Qd || !Rd || !Xs || !Ps || !Xs0 || !Ps0 || !Xf || !Pf || !Xpreds || !Ppreds || !Abars || !cost ||
        !status || (iters > 0 && !alpha))
        return fail(AC_ERR_BAD_ARG, "ieks solve: a required pointer is NULL");
    if (!ws || ws_floats < ieks_ws_floats(n, T, candidates)) return fail(AC_ERR_WORKSPACE, "ieks workspace too small: see ac_ieks_workspace_floats");
    const IeksWs w(ws, (size_t)n, (size_t)T, (size_t)candidates);
    const size_t N = (size_t)n;
    rc = ieks_cost_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, 1, T, cost, nullptr, nullptr, nullptr, status, w.cost, stream);
    for (int it = 0; it <= iters && rc == AC_OK; ++it) {
        rc = ieks_pass_impl(h, o, X0, P0, Xbar, U, dt, Z, mask, Qd, Rd, n, T, Xf, Pf, ll, nu, S, nis, used, fstatus, Xpreds, Ppreds, Abars,
                            ws, stream);
        if (rc != AC_OK) break;
        rc = ac_ekf_smooth_f32(h, X0, P0, Xf, Pf, Xpreds, Ppreds, Abars, n, T, Xs, Ps, Xs0, Ps0, nullptr, w.rst, stream);
        if (rc != AC_OK || it == iters) break;
        rc = ac_ieks_candidates_f32(h, Xbar, Xs0, Xs, U, ladder, candidates, n, T, w.Xc, w.Uc, stream);
        if (rc != AC_OK) break;
        rc = ieks_cost_impl(h, o, X0, P0, w.Xc, w.Uc, dt, Z, mask, Qd, Rd, n, candidates, T, w.Jc, nullptr, nullptr, nullptr, w.stc, w.cost,
                            stream);
        if (rc != AC_OK) break;
        rc = ac_ieks_accept_f32(h, cost + (size_t)it * N, w.Jc, w.stc, w.Xc, ladder, candidates, n, T, Xbar, alpha + (size_t)it * N,
                                cost + (size_t)(it + 1) * N, status, stream);
    }
    return rc;
}

// ---- MPPI: sampler and softmin update (ac_mppi.hpp, mppi_inst.hip) ---------------------------------------------------------------
namespace {
int mppi_check(const ac_handle* h, const ac_mppi_opts* o, int K, long B, long H) {
    if (!h || !o || K < 1 || B < 1 || H < 1) return AC_ERR_BAD_ARG;
    if ((long)K > 2147483647L / B) return fail(AC_ERR_BAD_ARG, "mppi: K * B exceeds 2^31 - 1");
    if (!(o->lambda > 0.f) || !(o->lambda <= 3.4028235e38f)) return fail(AC_ERR_BAD_ARG, "mppi: lambda must be finite and > 0");
    for (int r = 0; r < 7; ++r) {
        if (!(o->sigma[r] >= 0.f) || !(o->sigma[r] <= 3.4028235e38f))
            return fail(AC_ERR_BAD_ARG, "mppi: sigma must be finite and >= 0");
        if (!(o->u_min[r] <= o->u_max[r])) return fail(AC_ERR_BAD_ARG, "mppi: u_min > u_max (or NaN)");
    }
    return AC_OK;
}
}  // namespace

int ac_mppi_workspace_floats(const ac_handle* h, int K, long B, long H, size_t* floats) {
    if (!h || !floats || K < 1 || B < 1 || H < 1 || (long)K > 2147483647L / B) return AC_ERR_BAD_ARG;
    *floats = (size_t)K * (size_t)B;  // the normalised weights
    return AC_OK;
}

int ac_mppi_sample_f32(ac_handle* h, const ac_mppi_opts* o, const unsigned int* it_dev, const float* Unom, const float* X0, int K,
                       long B, long H, float* Uc, float* X0c, void* stream) {
    AC_ENTER(h);
    const int rc = mppi_check(h, o, K, B, H);
    if (rc != AC_OK) return rc;
    if (!Unom || !Uc) return AC_ERR_BAD_ARG;
    if ((X0 == nullptr) != (X0c == nullptr)) return fail(AC_ERR_BAD_ARG, "mppi: X0 and X0c go together");
    int grid = 0;
    AC_HIP(mppi_launch_sample(*o, it_dev, Unom, X0, K, B, H, Uc, X0c, (hipStream_t)stream, &grid));
    note_launch(h, "k_mppi_sample", grid, kMppiBlock, 0);
    return AC_OK;
}

int ac_mppi_update_f32(ac_handle* h, const ac_mppi_opts* o, unsigned int* it_dev, const float* J, const float* Uc, const float* Unom,
                       int K, long B, long H, float* Unew, float* stats, float* ws, size_t ws_floats, void* stream) {
    AC_ENTER(h);
    const int rc = mppi_check(h, o, K, B, H);
    if (rc != AC_OK) return rc;
    if (!J || !Uc || !Unom || !Unew || !stats) return AC_ERR_BAD_ARG;
    if (!ws || ws_floats < (size_t)K * (size_t)B)
        return fail(AC_ERR_WORKSPACE, "mppi workspace too small: see ac_mppi_workspace_floats");
    int grid = 0;
    AC_HIP(mppi_launch_update(*o, it_dev, J, Uc, Unom, K, B, H, Unew, stats, ws, (hipStream_t)stream, &grid));
    note_launch(h, "k_mppi_blend", grid, kMppiBlock, 0);
    return AC_OK;
}

int ac_set_hidden_route(ac_handle* h, int route) {
    if (!h || route < AC_HIDDEN_AUTO || route > AC_HIDDEN_F16) return AC_ERR_BAD_ARG;
    if (route == AC_HIDDEN_F16 && h->has_mlp) {
        const bool ok = kBf16Hidden && h->use_mfma && h->wt == 8 && h->has_bf && h->f16_gate == F16_GATE_OK;
        if (!ok) return fail(AC_ERR_UNSUPPORTED, hidden_f16_refusal(h));
    }
    h->hidden_route = route;
    return AC_OK;
}

int ac_hidden_route_of(const ac_handle* h, int* route, int* gate) {
    if (!h || !h->has_mlp) return AC_ERR_BAD_ARG;
    const bool bf = kBf16Hidden && h->use_mfma && h->wt == 8 && h->has_bf;
    const bool f16 = bf && h->f16_gate == F16_GATE_OK && h->hidden_route != AC_HIDDEN_BF16;
    if (route) *route = f16 ? AC_HIDDEN_F16 : bf ? AC_HIDDEN_BF16 : AC_HIDDEN_AUTO;
    if (gate) *gate = bf ? h->f16_gate : -1;
    return AC_OK;
}

int ac_last_launch(const ac_handle* h, char* name, size_t len, int* grid, int* block, int* lds_bytes) {
    if (!h) return AC_ERR_BAD_ARG;
    if (name && len) snprintf(name, len, "%s", h->last_name);
    if (grid) *grid = h->last_grid;
    if (block) *block = h->last_block;
    if (lds_bytes) *lds_bytes = h->last_lds;
    return AC_OK;
}

}  // extern "C"
