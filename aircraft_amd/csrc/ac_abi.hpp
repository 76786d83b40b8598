// ac_abi.hpp — what the units of the C ABI (abi_*.hip: include/aircraft_hip.h) share: the handle, the error and launch helpers,
// instance selection, and the entry-free cores one unit calls in another.  gfx950 only.  No allocation or synchronisation
// inside the compute entry points (graph-capturable).
// It includes what its declarations need and no engine header: a unit includes its own.  It defines no kernel, and the only
// state behind it (g_err) is defined in abi_core.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "ac_dynamics.hpp"     // DevParams
#include "ac_mlp_model.hpp"    // MlpModelInfo, MlpPlan
#include "ac_track_dev.hpp"    // TrackDev
#include "ac_wgrad_plan.hpp"   // WgradPlan

namespace ac {

extern thread_local char g_err[512];  // ac_last_error's text (abi_core.hip)

inline int hip_fail(hipError_t e, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return AC_ERR_HIP;
}
// every non-HIP error return that carries text goes through here, so ac_last_error() never shows a stale message
inline int fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}
#define AC_HIP(call)                                           \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #call);      \
    } while (0)

}  // namespace ac

// The handle IS a model description (plans, wt, routes: MlpModelInfo, ac_mlp_model.hpp — what ac_set_mlp hands over from
// build_mlp_model) plus the device state around it.
struct ac_handle : ac::MlpModelInfo {
    ac::DevParams dp;
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
    float* d_wgimg;    // fragments of the folded net for the weight gradient (build_wgrad_image, ac_wgrad_plan.hpp), device
    ac::WgradPlan wg;
    unsigned* d_queue; // ticket counter of the persistent tiled kernels (GroupQueue, ac_mlp_valu.hpp); 0 between launches
    float* d_hess_ws;  // [n][4][126] stage tensors of the MLP Hessian path (ac_reserve_hess_workspace)
    size_t hess_ws_floats;
    float* d_hess_ws2;  // sub-step composition of the second-order blocks (substeps > 1)
    size_t hess_ws2_floats;
    float* d_poly_tab;  // coefficient, intercept and gradient tables of the cubic fits (DevParams::poly_tab)
    float* d_track;  // [nseg][3][4] segment cubics (device)
    ac::TrackDev track;
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

namespace ac {

inline void note_launch(ac_handle* h, const char* name, int grid, int block, int lds) {
    snprintf(h->last_name, sizeof(h->last_name), "%s", name);
    h->last_grid = grid; h->last_block = block; h->last_lds = lds;
}

inline int check_params(const ac_params* p) {
    if (!p) return AC_ERR_BAD_ARG;
    if (p->substeps < 1) return AC_ERR_BAD_ARG;
    if (p->model_kind < AC_MODEL_DEFAULT || p->model_kind > AC_MODEL_QUAD) return AC_ERR_BAD_ARG;
    return AC_OK;
}

inline int model_ready(const ac_handle* h) {
    switch (h->dp.p.model_kind) {
        case AC_MODEL_LINEAR: return h->has_linear ? AC_OK : AC_ERR_NO_MODEL;
        case AC_MODEL_POLY: return h->has_poly ? AC_OK : AC_ERR_NO_MODEL;
        case AC_MODEL_NN: return h->has_mlp ? AC_OK : AC_ERR_NO_MODEL;
        default: return AC_OK;
    }
}

// Raise a kernel's dynamic-LDS limit once per (handle, kernel, size): the attribute is sticky per device, and the call
// costs a driver round trip that does not belong in front of every launch.
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
// ac_nn_decl.hpp may be named in f: every other one would be compiled into the unit that names it.
constexpr int kNoInstance = 1;  // (no ac_status is positive)
constexpr const char* kNoNnInstance = "no kernel instance for this MLP width / flavour";
constexpr const char* kNoTiledInstance = "no tiled vector-ALU kernel instance for this hidden width";
template <int... Vs, class F> int pick(int v, F&& f) {
    int rc = kNoInstance;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
// ... over the handle's (wt, use_mfma): f(WT, MF) with MF a std::bool_constant
template <class F> int pick_wt_mfma(const ac_handle* h, F&& f) {
    return pick<2, 4, 8>(h->wt, [&](auto WT) { return h->use_mfma ? f(WT, std::true_type{}) : f(WT, std::false_type{}); });
}
inline int instance(int rc, const char* missing) { return rc == kNoInstance ? fail(AC_ERR_UNSUPPORTED, missing) : rc; }
// ... over the models of the fused reverse sweeps (ac_vjp.hpp): f(MODEL).  The callers' route and refusal checks have excluded
// the MLP surrogate and the quadrotor.
template <class F> int pick_fused_model(const ac_handle* h, F&& f) {
    return instance(pick<AC_MODEL_DEFAULT, AC_MODEL_LINEAR, AC_MODEL_POLY>(h->dp.p.model_kind, f),
                    "no fused reverse sweep for this model");
}

// The plan of the kernels on MlpEngine (sensitivity and forward): the matrix-core flavour runs its edge layers on the vector
// ALUs and takes plan_sens; the cross-lane validation flavour keeps plan.  (The second-order and the cooperative rollout
// engines: plan.)
inline const MlpPlan& engine_plan(const ac_handle* h) { return h->use_mfma ? h->plan_sens : h->plan; }

// a workspace buffer's start on a 256-byte boundary, as a torch allocation would have it
inline float* align256(float* p) { return (float*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// do two spans of floats share an element? (a NULL span shares none)
struct RtsSpan { const float* p; size_t floats; };
inline bool rts_overlap(const RtsSpan& a, const RtsSpan& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a0 < b0 + b.floats * sizeof(float) && b0 < a0 + a.floats * sizeof(float);
}
inline bool modes_overlap(const RtsSpan* out, int n_out, const RtsSpan* in, int n_in) {
    for (int a = 0; a < n_out; ++a)
        for (int b = 0; b < n_in; ++b)
            if (rts_overlap(out[a], in[b])) return true;
    return false;
}

// ---- the entry-free cores (abi_core.hip) that the other units launch through: the handle's derivative, step and sensitivity
// kernels over n units in blocks of blk, with the checks and the dispatch of their entry points ----------------------------------
int derivative_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, void* stream);
int step_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk, float* Xn,
              void* stream);
int sens_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk, float* Xn,
              float* A, float* Bm, float* c, void* stream);
int deriv_sens_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, float* Fx, float* Fu,
                    void* stream);

}  // namespace ac
