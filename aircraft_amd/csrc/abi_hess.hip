// abi_hess.hip — second-order step sensitivities: the blocks of one RK4 sub-step, their composition across sub-steps, and the
// workspace they run in.
// One unit of the C ABI (include/aircraft_hip.h); the handle and the helpers every unit shares: ac_abi.hpp.
#include "ac_abi.hpp"
#include "ac_hess.hpp"
#include "ac_hess_adj.hpp"
#include "ac_nn_decl.hpp"

using namespace ac;

namespace {

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

}  // namespace

extern "C" {

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

int ac_hess_workspace(const ac_handle* h, float** ptr, size_t* floats) {
    if (!h) return AC_ERR_BAD_ARG;
    if (ptr) *ptr = h->d_hess_ws;
    if (floats) *floats = h->hess_ws_floats;
    return AC_OK;
}

}  // extern "C"
