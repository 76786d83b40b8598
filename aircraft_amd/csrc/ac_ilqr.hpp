// ac_ilqr.hpp — batched iLQR / Gauss-Newton sweep on top of the step sensitivities.
//
// Build-side component: the reference solves its NLP with IPOPT on one instance (control/base.py:455-477); what is
// built here plays the `loss` / control-limit roles of ControlProblem (control/base.py:323-337,
// control/aircraft.py:29-41, main/control/control.py:35-70) for B independent instances at once:
//
//   cost      J = sum_k 1/2 (x_k - x_ref)' Q (x_k - x_ref) + 1/2 u_k' R u_k  +  1/2 (x_N - x_goal)' Qf (x_N - x_goal)
//   backward  Q-function expansion with the kernel-computed A_k = dF/dx, B_k = dF/du (no second-order dynamics terms),
//             Levenberg regularisation mu on Q_uu, gains  K_k = -Quu^-1 Qux,  k_k = -Quu^-1 Qu
//             with BOX (control-limited DDP): k_k = argmin 1/2 d'Quu d + Qu'd over u_min - u_k <= d <= u_max - u_k (ac_boxqp.hpp),
//             rows of K_k at clamped controls zero, the others from the free block of Quu
//   forward   closed-loop rollout  u = clip(u_k + alpha k_k + K_k (x - x_k)),  several alpha per instance in one launch
//
// Layouts: X [H+1][13][B], U [H][7][B], A [H][13][13][B], Bm [H][13][7][B], K [H][7][13][B], kff [H][7][B].
#pragma once
#include "ac_kernels_analytic.hpp"
#include "ac_boxqp.hpp"

namespace ac {

// quadratic cost + box limits, passed by value
struct IlqrCost {
    float q[13], qf[13], r[7];
    float x_ref[13], x_goal[13];
    float u_min[7], u_max[7];
    float reg;  // Levenberg term added to the diagonal of Quu
    float u_lin[7];  // linear control cost  u_lin . u_k  per node (the time term: w_time * dt_k on the time row)
    int dt_row;      // <= 0: fixed step (a zeroed struct means that); r > 0: control row r carries dt_k as a decision variable (Policy::step)
};

// Optional per-node, per-instance state cost  l_k(x) = 1/2 sum_j q_k[j] (x_j - xref_k[j])^2 + glin_k . x  (k = 0..H,
// node H is the terminal one).  When q != nullptr these arrays [H+1][13][Bn] replace q / qf / x_ref / x_goal of
// IlqrCost; a candidate batch wider than Bn (line search) reads instance b % Bn.
struct NodeCost {
    const float* __restrict__ q;
    const float* __restrict__ xref;
    const float* __restrict__ glin;
    long Bn;
    // optional per-node, per-instance CONTROL gradient [H][7][Bn] added to Q_u (the backward pass with second-order blocks
    // only: k_ilqr_backward<true, true>): the control-rate term of the goal-acquisition loss (ac_goal.hpp), whose curvature
    // arrives in the (u, u) block of Hz
    const float* __restrict__ uglin = nullptr;
    AC_DI bool on() const { return q != nullptr; }
    // value and gradient pieces of row j at node k
    // NODE is a compile-time switch of the kernels (constant cost = the original straight-line code); bn = b % Bn
    template <bool NODE>
    AC_DI void row(const IlqrCost& C, long k, bool terminal, int j, long bn, float& qj, float& xr, float& gl) const {
        if constexpr (NODE) {
            const long o = (k * 13 + j) * Bn + bn;
            qj = q[o]; xr = xref[o]; gl = glin[o];
        } else {
            qj = terminal ? C.qf[j] : C.q[j];
            xr = terminal ? C.x_goal[j] : C.x_ref[j];
            gl = 0.f;
        }
    }
};

struct AlphaSet {
    int n;
    float a[8];
};

// ---- backward (Riccati) pass ------------------------------------------------------------------
// One wave per instance: lane (j, rb) = (t & 15, t >> 4) owns rows rb, rb+4, rb+8, (rb+12) of column j of the 13-wide
// matrices (and of the 7-wide ones), all matrices of the instance in LDS.  The 7x7 Cholesky and the triangular solves
// run redundantly in registers on every lane.  Sequential in k; ~15 kflop per node, so what matters is latency:
//  * the inputs of a node (A_k, B_k, x_k, u_k, its cost rows, its second-order block) are 260-760 floats that sit
//    B floats apart in HBM (the arrays are instance-minor for the kernels that produce them), i.e. one cache line and
//    one page each — fetched on demand they cost ~10 us per node.  They are gathered by LDS-DMA (per-lane source
//    address, lane-linear LDS image) into a ring kRing nodes deep, several nodes ahead of the one being processed,
//    with a counted s_waitcnt vmcnt(N): nothing in the loop waits on an ordinary global load;
//  * one wave = one workgroup, so LDS hand-offs need only lgkmcnt(0), never a cross-wave barrier.
// RATE (k_ilqr_backward_rate, ac_ilqr_rate.hpp): g and h travel as one more 14-lane instruction per node; uglin does not.
template <bool NODE, bool NEWTON, bool SHOOT = false, bool RATE = false> struct IlqrRing {
    static constexpr int kWork = 736 + (RATE ? 208 : 0);         // LDS floats of the per-instance work area (layout in the body); RATE: then Vxp, Vpp, Kp, Vp
    static constexpr bool kUglin = NODE && NEWTON && !RATE;      // the control-gradient row (NodeCost::uglin) travels in the ring
    static constexpr int kInstr = 6 + (NEWTON ? 7 : 0) + (kUglin ? 1 : 0) + (SHOOT ? 1 : 0) + (RATE ? 1 : 0);  // LDS-DMA wave-instructions per node
    static constexpr int kShoot = NEWTON ? 768 : 320;            // SHOOT: F_k at kShoot..+12, x_{k+1} at kShoot+13..+25
    static constexpr int kRate = NEWTON ? 761 : 320;             // RATE: g at kRate..+6, h at kRate+7..+13 (after Hz / after glin)
    static constexpr int kNodeFloats = RATE ? (NEWTON ? 776 : 336) : kShoot + (SHOOT ? 26 : 0);  // A 0..168, B 169..259, x 260, u 273, q 280, xref 293, glin 306, Hz 320..760, uglin 761..767
    static constexpr int kDepth = NEWTON ? 5 : 8;                // nodes in flight (kInstr * (kDepth - 1) <= 63)
    static_assert(kInstr * (kDepth - 1) <= 63, "vmcnt is a 6-bit counter");
    static_assert(!RATE || kRate + 14 <= kNodeFloats, "node image");
};

// Outputs of the box-constrained pass (BOX, control-limited DDP: the control box enters the backward pass as a QP per node,
// ac_boxqp.hpp) — an empty struct for the unconstrained kernels.
template <bool BOX> struct IlqrBoxOut {};
template <> struct IlqrBoxOut<true> {
    signed char* __restrict__ act;  // [H][7][B] or NULL: 0 free, -1 / +1 clamped at the lower / upper bound, 2 pinned (u_min >= u_max)
    int* __restrict__ stat;         // [2][B] or NULL: largest Newton-iteration count over the nodes, nodes whose QP hit a cap
};

// Multiple shooting (SHOOT): the iterate's states are decision variables, node k has the gap  d_k = F_k - x_{k+1}  and the
// linearised dynamics read  dx_{k+1} = A_k dx_k + B_k du_k + d_k.  The only change to the recursion: node k reads
// v = V'_x + V'_xx d_k  wherever it read V'_x (in Q_x and Q_u).  F_k and x_{k+1} travel in the ring (ONE more LDS-DMA
// wave-instruction per node).  Optionally the value expansion each node STARTS from is written out for the direction sweep
// (k_shoot_direction: lam_k = V_x^{k+1} + V_xx^{k+1} dx_{k+1}) — an empty struct for the single-shooting kernels.
template <bool SHOOT> struct IlqrShootIn {};
template <> struct IlqrShootIn<true> {
    const float* __restrict__ F;  // [H][13][B]: F(x_k, u_k)
    float* __restrict__ Vx;       // [H][13][B] or NULL: Vx[k] = V_x^{k+1}
    float* __restrict__ Vxx;      // [H][13][13][B] or NULL (both or neither): Vxx[k] = V_xx^{k+1}
};

// Per node of a BOX kernel: delta* of  min 1/2 d'Quu d + Qu'd,  u_min - U_k <= d <= u_max - U_k  becomes kff, and Quu is replaced
// by its free block (unit rows and columns at the clamped controls) for the factorisation that gives the gains.
struct IlqrBoxNode {
    unsigned clamped = 0u;
    int iters = 0, capped = 0;
    AC_DI bool on(int i) const { return (clamped >> i) & 1u; }
    AC_DI void solve(const IlqrCost& C, const float* u_k, const float (&Qs)[7][7], const float (&qu)[7], float (&Qf)[7][7],
                     float (&kf)[7], signed char* act, long stride) {
        float lo[7], hi[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) { lo[i] = C.u_min[i] - u_k[i]; hi[i] = C.u_max[i] - u_k[i]; }
        BoxQp r;
        boxqp7(Qs, qu, lo, hi, r);
        clamped = r.clamped;
        iters = iters > r.iters ? iters : r.iters;
        capped += r.capped;
        boxqp_mask(Qs, clamped, Qf);
#pragma unroll
        for (int i = 0; i < 7; ++i) kf[i] = r.x[i];
        if (act != nullptr) {
#pragma unroll
            for (int i = 0; i < 7; ++i) act[i * stride] = (signed char)r.act(i);
        }
    }
};

AC_DI void ilqr_glds(const float* g, float* lds_dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_dst, 4, 0, 0);
}
// wave-level hand-off through LDS (single-wave workgroup): LDS traffic retired, no reordering across this point
AC_DI void ilqr_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); }

// per-node cost arrays or the constant cost; second-order dynamics blocks or none; the control box as a QP per node or not at all.
// The body is ac_ilqr_backward_body.hpp, shared with k_ilqr_backward_shoot below (switch AC_ILQR_SHOOT) and with
// k_ilqr_backward_rate of ac_ilqr_rate.hpp (switch AC_ILQR_RATE): one recursion, one ring, one Cholesky, one BOX hook.
// A textual include under a further kernel name, not a fourth template parameter and not a body function: the mangled names of
// these kernels are pinned (tests/test_host_box.py looks for `Lb1EEEv`), a further parameter changes them, and a body inlined from
// a function gives the existing kernels another schedule (the __restrict__ kernel arguments reach it as scoped alias information).
template <bool NODE, bool NEWTON, bool BOX = false>
__global__ __launch_bounds__(64) void k_ilqr_backward(const IlqrCost C, const NodeCost N, const float* __restrict__ X,
                                                      const float* __restrict__ U, const float* __restrict__ A,
                                                      const float* __restrict__ Bm, const float* __restrict__ Hz, long B, long H,
                                                      float* __restrict__ K, float* __restrict__ kff,
                                                      float* __restrict__ dV, const IlqrBoxOut<BOX> box = {}) {
#define AC_ILQR_SHOOT 0
#define AC_ILQR_RATE 0
#include "ac_ilqr_backward_body.hpp"
#undef AC_ILQR_RATE
#undef AC_ILQR_SHOOT
}

// the same pass over a multiple-shooting iterate
template <bool NODE, bool NEWTON, bool BOX>
__global__ __launch_bounds__(64) void k_ilqr_backward_shoot(const IlqrCost C, const NodeCost N, const float* __restrict__ X,
                                                            const float* __restrict__ U, const float* __restrict__ A,
                                                            const float* __restrict__ Bm, const float* __restrict__ Hz, long B,
                                                            long H, float* __restrict__ K, float* __restrict__ kff,
                                                            float* __restrict__ dV, const IlqrShootIn<true> sh,
                                                            const IlqrBoxOut<BOX> box = {}) {
#define AC_ILQR_SHOOT 1
#define AC_ILQR_RATE 0
#include "ac_ilqr_backward_body.hpp"
#undef AC_ILQR_RATE
#undef AC_ILQR_SHOOT
}

// Everything a backward pass takes.  ilqr_launch_backward (ilqr_backward_inst.hip: all 24 kernels) picks the family by F / rate_g
// (never both), BOX by `box`, NODE by N.q and NEWTON by Hz; the C entry points fill this and share ONE validation.
struct IlqrBackwardArgs {
    IlqrCost C;
    NodeCost N;
    const float *X, *U, *A, *Bm, *Hz;
    const float *rate_g, *rate_h;  // k_ilqr_backward_rate when rate_g != NULL (Kp then too)
    const float* F;                // k_ilqr_backward_shoot when F != NULL (Vx, Vxx optional)
    long B, H;
    float *K, *Kp, *kff, *dV, *Vx, *Vxx;
    bool box;
    signed char* act;  // (box only)
    int* stat;         // (box only)
};
hipError_t ilqr_launch_backward(const IlqrBackwardArgs& a, hipStream_t st);

// ---- costate sweep ------------------------------------------------------------------------------------
// Multipliers of the defect rows x_{k+1} = F(x_k, u_k) at the current iterate (the NLP's lambda estimate):
//   Lam[H-1] = grad l_N(x_N),   Lam[k-1] = grad l_k(x_k) + A_k' Lam[k]
// One lane per instance, sequential in k; feeds ac_shoot_hess_f32 for the exact-Hessian (Newton) backward pass.
template <bool NODE>
__global__ __launch_bounds__(kBlock) void k_ilqr_costate(const IlqrCost C, const NodeCost N, const float* __restrict__ X,
                                                         const float* __restrict__ A, long B, long H,
                                                         float* __restrict__ Lam) {
    const long b = (long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    float lam[13];
#pragma unroll
    for (int j = 0; j < 13; ++j) {
        float qj, xr, gl;
        N.template row<NODE>(C, H, true, j, b, qj, xr, gl);
        lam[j] = fmaf(qj, X[(H * 13 + j) * B + b] - xr, gl);
    }
    for (long k = H - 1;; --k) {
#pragma unroll
        for (int j = 0; j < 13; ++j) Lam[(k * 13 + j) * B + b] = lam[j];
        if (k == 0) break;
        float nxt[13];
#pragma unroll
        for (int j = 0; j < 13; ++j) {
            float qj, xr, gl;
            N.template row<NODE>(C, k, false, j, b, qj, xr, gl);
            float s = fmaf(qj, X[(k * 13 + j) * B + b] - xr, gl);
#pragma unroll
            for (int m = 0; m < 13; ++m) s = fmaf(A[((k * 13 + m) * 13 + j) * B + b], lam[m], s);
            nxt[j] = s;
        }
#pragma unroll
        for (int j = 0; j < 13; ++j) lam[j] = nxt[j];
    }
}

// ---- quadratic trajectory cost ---------------------------------------------------------------------
template <bool NODE>
__global__ __launch_bounds__(kBlock) void k_ilqr_cost(const IlqrCost C, const NodeCost N, const float* __restrict__ X,
                                                      const float* __restrict__ U, long B, long H,
                                                      float* __restrict__ cost) {
    const long b = (long)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    float acc = 0.f;
    const long bn = NODE ? b % N.Bn : b;
    for (long k = 0; k <= H; ++k) {
#pragma unroll
        for (int i = 0; i < 13; ++i) {
            float qi, xr, gl;
            N.template row<NODE>(C, k, k == H, i, bn, qi, xr, gl);
            const float x = X[(k * 13 + i) * B + b], d = x - xr;
            acc = fmaf(0.5f * qi * d, d, acc);
            if constexpr (NODE) acc = fmaf(gl, x, acc);
        }
        if (k < H) {
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                const float u = U[(k * 7 + i) * B + b];
                acc = fmaf(0.5f * C.r[i] * u, u, acc);
                acc = fmaf(C.u_lin[i], u, acc);
            }
        }
    }
    cost[b] = acc;
}

// ---- feedback policy evaluated inside the rollout kernels ---------------------------------------------
// Output instance o = a * B + b (a = line-search index): u = clip(U_k[b] + alpha_a kff_k[b] + K_k[b] (x - Xnom_k[b])).
// With Kp (the exact control-rate pass, ac_ilqr_rate.hpp) the law gains  + Kp_k[b] (u_applied_{k-1} - U_{k-1}[b])  for k > 0:
// both `control` overloads read the control the lane applied at the previous node from `u` on entry.
struct Policy {
    const float* __restrict__ Xnom;  // [H+1][13][B]
    const float* __restrict__ U;     // [H][7][B]
    const float* __restrict__ K;     // [H][7][13][B]
    const float* __restrict__ kff;   // [H][7][B]
    long B;                          // nominal batch
    const float* __restrict__ Kp = nullptr;  // [H][7][7][B] or NULL: gains on the previous control
    AlphaSet alphas;
    float u_min[7], u_max[7];
    // Time as a decision variable (the reference's `dt_k` per node, control/base.py:276, 339-385: dt_k = 1 / progress_k^2
    // in 'progress' time, progress_k^2 in 'variable' time, bounded by dt_bounds): control row `dt_row` — a row the force model
    // ignores (a thrust row of the fixed-wing plugin) — carries dt_k itself, clipped to its box like every control; the
    // column of B for it is c = dF/d(dt) of the sensitivity kernels.  dt_row <= 0: the fixed step.
    int dt_row;
    AC_DI float step(const float u[7], float dt) const {
        float r = dt;
#pragma unroll
        for (int i = 1; i < 7; ++i) r = (i == dt_row) ? u[i] : r;
        return r;
    }

    AC_DI void control(long k, long o, const float x[13], float u[7]) const {
        const long b = o % B;
        const float alpha = alphas.a[(int)(o / B)];
        float dx[13];
#pragma unroll
        for (int i = 0; i < 13; ++i) dx[i] = x[i] - Xnom[(k * 13 + i) * B + b];
        const bool fb = Kp != nullptr && k > 0;
        float dp[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) dp[i] = fb ? u[i] - U[((k - 1) * 7 + i) * B + b] : 0.f;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            float s = fmaf(alpha, kff[(k * 7 + i) * B + b], U[(k * 7 + i) * B + b]);
#pragma unroll
            for (int m = 0; m < 13; ++m) s = fmaf(K[((k * 7 + i) * 13 + m) * B + b], dx[m], s);
            if (fb) {
#pragma unroll
                for (int m = 0; m < 7; ++m) s = fmaf(Kp[((k * 7 + i) * 7 + m) * B + b], dp[m], s);
            }
            u[i] = fminf(fmaxf(s, u_min[i]), u_max[i]);
        }
    }

    // The same control law for kernels where the four lane groups g = 0..3 of a wave hold the same instance (MLP
    // rollouts): group g takes the columns m = g, g+4, g+8, g+12 of K_k, so a lane loads a quarter of the gains, and
    // the partial products are summed across the groups with two cross-lane adds.  load() can be issued a node ahead.
    // With Kp, group g also takes the columns m = g, g + 4 (< 7) of Kp_k and the rows of U_{k-1} that go with them.
    struct Quarter {
        float kq[7][4], xn[4], ub[7];
        float kpq[7][2], up[2];
    };
    AC_DI void load(long k, long o, int g, Quarter& q) const {
        const long b = o % B;
        const float alpha = alphas.a[(int)(o / B)];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = g + 4 * c;
            const bool on = m < 13;
            const int mm = on ? m : 12;
            q.xn[c] = Xnom[(k * 13 + mm) * B + b];
#pragma unroll
            for (int i = 0; i < 7; ++i) q.kq[i][c] = on ? K[((k * 7 + i) * 13 + mm) * B + b] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) q.ub[i] = fmaf(alpha, kff[(k * 7 + i) * B + b], U[(k * 7 + i) * B + b]);
        if (Kp != nullptr) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int m = g + 4 * c;
                const bool on = m < 7 && k > 0;
                const int mm = m < 7 ? m : 6;
                q.up[c] = on ? U[((k - 1) * 7 + mm) * B + b] : 0.f;
#pragma unroll
                for (int i = 0; i < 7; ++i) q.kpq[i][c] = on ? Kp[((k * 7 + i) * 7 + mm) * B + b] : 0.f;
            }
        }
    }
    AC_DI void control(const Quarter& q, int g, const float x[13], float u[7]) const {
        float dp[2] = {0.f, 0.f};
        if (Kp != nullptr) {  // u[g], u[g + 4] (applied at the previous node; zero at node 0) without dynamic register indexing
            const float a0 = g == 0 ? u[0] : (g == 1 ? u[1] : (g == 2 ? u[2] : u[3]));
            const float a1 = g == 0 ? u[4] : (g == 1 ? u[5] : (g == 2 ? u[6] : 0.f));
            dp[0] = a0 - q.up[0];
            dp[1] = a1 - q.up[1];
        }
        float dx[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            // x[g + 4 c] without dynamic register indexing (c == 3 only exists for g == 0)
            const float x0 = x[4 * c], x1 = (4 * c + 1 < 13) ? x[(4 * c + 1 < 13) ? 4 * c + 1 : 0] : 0.f;
            const float x2 = (4 * c + 2 < 13) ? x[(4 * c + 2 < 13) ? 4 * c + 2 : 0] : 0.f;
            const float x3 = (4 * c + 3 < 13) ? x[(4 * c + 3 < 13) ? 4 * c + 3 : 0] : 0.f;
            const float xs = g == 0 ? x0 : (g == 1 ? x1 : (g == 2 ? x2 : x3));
            dx[c] = xs - q.xn[c];
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) s = fmaf(q.kq[i][c], dx[c], s);
            if (Kp != nullptr) s = fmaf(q.kpq[i][1], dp[1], fmaf(q.kpq[i][0], dp[0], s));
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            u[i] = fminf(fmaxf(q.ub[i] + s, u_min[i]), u_max[i]);
        }
    }
};

// closed-loop rollout, analytic models: one lane per output instance
template <int MODEL>
__global__ __launch_bounds__(64) void k_rollout_policy(const DevParams P, const Policy pol, const float* __restrict__ X0,
                                                       float dt, long Bout, long H, float* __restrict__ Xout,
                                                       float* __restrict__ Uout) {
    const long o = (long)blockIdx.x * 64 + threadIdx.x;
    if (o >= Bout) return;
    float x[13], u[7];
    load_rows<13>(X0, pol.B, o % pol.B, x);
    double xa[13];
#pragma unroll
    for (int r = 0; r < 13; ++r) { Xout[(long)r * Bout + o] = x[r]; xa[r] = (double)x[r]; }
    AnalyticCoeffs<MODEL> coeffs;
    for (long k = 0; k < H; ++k) {
#pragma unroll
        for (int r = 0; r < 13; ++r) x[r] = (float)xa[r];
        pol.control(k, o, x, u);
#pragma unroll
        for (int r = 0; r < 7; ++r) Uout[(k * 7 + r) * Bout + o] = u[r];
        state_update_carry(P, coeffs, xa, u, pol.step(u, dt));
        float* out = Xout + (k + 1) * 13 * Bout;
#pragma unroll
        for (int r = 0; r < 13; ++r) out[(long)r * Bout + o] = (float)xa[r];
    }
}

}  // namespace ac
