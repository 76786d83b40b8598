// abi_core.hip — the handle's life and models, and the forward kernels: derivative, step, aero, rollout, the first-order
// sensitivities, the shooting rows, the envelope and quaternion rows.  The only unit that defines state (g_err).
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ac_abi.hpp"
#include "ac_kernels_analytic.hpp"
#include "ac_nn_decl.hpp"

using namespace ac;

thread_local char ac::g_err[512] = "";

namespace {
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
}  // namespace

// ---- the cores behind the entry points; the other units call them too (ac_abi.hpp) ------------------------------------------
namespace ac {
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

int derivative_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, void* stream) {
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

int step_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
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

int sens_impl(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, long blk,
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

int deriv_sens_impl(ac_handle* h, const float* X, const float* U, long n, long blk, float* Xdot, float* Fx,
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
}  // namespace ac

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

int ac_set_vjp_route(ac_handle* h, int route) {
    AC_ENTER(h);
    if (!h || route < AC_VJP_AUTO || route > AC_VJP_COMPOSED) return AC_ERR_BAD_ARG;
    h->vjp_route = route;
    return AC_OK;
}

int ac_set_cgrad_grid(ac_handle* h, int max_workgroups) {
    if (!h || max_workgroups < 0) return AC_ERR_BAD_ARG;
    h->cgrad_grid = max_workgroups;
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

int ac_mlp_folded_shape(const ac_handle* h, int* n_layers, int* widths) {
    if (!h || !n_layers || !widths) return AC_ERR_BAD_ARG;
    g_err[0] = 0;
    if (!h->has_mlp) return fail(AC_ERR_NO_MODEL, "no MLP installed: call ac_set_mlp first");
    *n_layers = h->wg.n_layers;
    widths[0] = h->wg.nin[0];
    for (int l = 0; l < h->wg.n_layers; ++l) widths[l + 1] = h->wg.nout[l];
    return AC_OK;
}

// ---- compute entry points ------------------------------------------------------------------------
int ac_state_derivative_f32(ac_handle* h, const float* X, const float* U, long n, float* Xdot, void* stream) {
    return derivative_impl(h, X, U, n, n > 0 ? n : 1, Xdot, stream);
}

int ac_shoot_derivative_f32(ac_handle* h, const float* X, const float* U, long B, long H, float* Xdot, void* stream) {
    if (B < 0 || H < 0) return AC_ERR_BAD_ARG;
    return derivative_impl(h, X, U, B * H, B > 0 ? B : 1, Xdot, stream);
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

}  // extern "C"
