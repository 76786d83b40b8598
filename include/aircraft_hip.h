/*
 * aircraft_hip.h — C ABI of libaircraft_hip.so: the MI355X (gfx950) implementation of the
 * AIrcraft MPC-rollout hot path (6-DoF RK4 step through an aerodynamic-coefficient model,
 * plus first-order step sensitivities).
 *
 * Boundary: these entry points replace the CasADi `ca.Function` objects that the reference's
 * control layer consumes — `system.state_update` / `system.state_derivative`
 * (reference: src/aircraft/control/base.py:187-190) — and the `ca.jacobian` of them
 * (control/aircraft.py:85-95, control/base.py:279-280, 314-315).  A reference-side binding is a
 * ctypes stub; see INTEGRATION.md.
 *
 * Conventions
 *   - state  x = [p_ned(3), v_ned(3), q_frd_ned(4, xyzw), omega_frd(3)]   (dynamics/base.py:84-106)
 *   - control u = [aileron, elevator, rudder (deg), thrust(3), flaps]       (dynamics/aircraft.py:143-166)
 *   - batched arrays are component-major float32 DEVICE buffers: X is [13][n], U is [7][n] — the
 *     reference's own column-mapped call convention (`(13,N)` matrices, main/control/control.py:63),
 *     which is also the coalesced layout on the GPU.  A "unit" is one (x_k, u_k) pair: one MPC
 *     instance at one shooting node.
 *   - the caller owns every buffer; the library never allocates outputs.  The handle owns device
 *     copies of the coefficient-model data.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream),
 *     does no allocation and no synchronisation, and is therefore hipGraph-capturable.
 *   - return value: AC_OK (0) or a negative ac_status; nothing is thrown across the ABI.  NaNs in the
 *     inputs propagate to the outputs unchanged (the reference's callers test np.isnan,
 *     main/dynamics/dynamics.py:108).
 *   - thread-compatible per handle: no global mutable state.  A handle does own mutable DEVICE state that its
 *     launches share, so launches of ONE handle must be ordered on ONE stream (or otherwise serialised) where they use it:
 *       * the ticket counter of the persistent vector-ALU kernels of an MLP set with use_mfma = 0 (ac_step_sens_f32,
 *         ac_shoot_sens_f32, ac_*_derivative_sens_f32 on hidden widths <= 64): 0 between launches, drawn from by every
 *         wave of a launch and reset by the wave that draws the last ticket.  Two launches of one handle running
 *         concurrently on two streams would skip or duplicate unit groups; use one handle per stream;
 *       * the second-order workspace (ac_reserve_hess_workspace; see ac_step_hess_f32).
 *     ac_destroy / ac_set_* free or replace device memory: never while a stream of the process is capturing.
 */
#ifndef AIRCRAFT_HIP_H
#define AIRCRAFT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AC_NUM_STATES 13   /* SixDOF.num_states,   dynamics/base.py:101 */
#define AC_NUM_CONTROLS 7  /* Aircraft.num_controls, dynamics/aircraft.py:162 */
#define AC_AERO_ROWS 22
#define AC_MAX_LAYERS 8
#define AC_MAX_WIDTH 128   /* widest MLP layer the register-resident MFMA engine supports */

typedef enum ac_status {
    AC_OK = 0,
    AC_ERR_BAD_ARG = -1,       /* NULL pointer, negative size, unknown enum */
    AC_ERR_HIP = -2,           /* a HIP runtime call failed; see ac_last_error() */
    AC_ERR_UNSUPPORTED = -3,   /* e.g. MLP wider than AC_MAX_WIDTH */
    AC_ERR_NO_MODEL = -4,      /* model_kind needs data that was never set */
    AC_ERR_NO_DEVICE = -5,     /* no gfx950 device visible */
    AC_ERR_WORKSPACE = -6      /* a handle-owned workspace is too small: call the matching ac_reserve_* first; or a
                                  caller-provided one is (ac_vjp_workspace_floats) */
} ac_status;

/* Registry keys of COEFF_MODEL_REGISTRY, dynamics/coefficient_models.py:32-37 */
typedef enum ac_model_kind { AC_MODEL_DEFAULT = 0, AC_MODEL_LINEAR = 1, AC_MODEL_NN = 2, AC_MODEL_POLY = 3,
                             /* not a coefficient model: the Quadrotor plugin (dynamics/quadrotor.py:8-54) — body force
                              * (0, 0, sum T) and rotor moments straight from control rows 0-3 (the four thrusts);
                              * control rows 4-6 are ignored and their Jacobian columns are zero. */
                             AC_MODEL_QUAD = 4 } ac_model_kind;

/* Constants of one airframe + integration options.
 * Mirrors AircraftOpts / SixDOFOpts / AircraftConfiguration
 * (dynamics/aircraft.py:22-38, dynamics/base.py:9-14, utils.py:201-215).
 * inertia / inertia_inv are computed by the host in float64 from Ixx..Ixz, mass and com
 * (dynamics/aircraft.py:168-187, dynamics/base.py:139-144) and rounded once. */
typedef struct ac_params {
    float mass, S, b, c;
    float inertia[9];
    float inertia_inv[9];
    float com[3];
    float rudder_moment_arm;
    float epsilon;
    float gravity[3];
    int substeps;       /* physical_integration_substeps (>=1) */
    int normalise;      /* SixDOF.normalise: q <- q/|q| once after the last sub-step */
    int stall_scaling;  /* AircraftOpts.stall_scaling */
    int model_kind;     /* ac_model_kind */
} ac_params;

typedef struct ac_handle ac_handle;

/* Lifetime.  ac_create binds the handle to the CURRENT HIP device. */
int ac_create(const ac_params* params, ac_handle** out);
int ac_destroy(ac_handle* h);
/* Replace the scalar parameters (e.g. after the driver overrides aircraft.com, control.py:172). */
int ac_set_params(ac_handle* h, const ac_params* params);

/* Coefficient-model data (HOST pointers; copied).
 * linear: W[6][6] row-major, columns [qbar, alpha, beta, aileron, elevator, 1]   (coefficient_models.py:80-89)
 * poly:   coef[6][34], intercept[6]; sklearn PolynomialFeatures(3) order over (alpha, beta, aileron, elevator)
 *                                                                                 (coefficient_models.py:106-133)
 * mlp:    n_layers Linear layers; W[l] is [widths[l+1]][widths[l]] row-major (torch layout); act[l] = 0 identity,
 *         1 tanh after layer l; widths[0] must be 5, widths[n_layers] must be 6; input/output scalers as in
 *         ScaledModel (surrogates/models.py:101-155).  use_mfma = 1: the v_mfma_f32_16x16x4_f32 engines.  use_mfma = 0
 *         ("MFMA off", BASELINE configs[1]): the register-tiled v_pk_fma_f32 engine on the vector ALUs for hidden widths
 *         <= 64 and at least two layers after the fold (step, derivative, getters, rollout, policy rollout, step +
 *         sensitivities, df/dx); wider nets, single-layer nets and the second-order path of this flavour use the
 *         cross-lane validation form or are refused (see the entry points).
 *         An activation-free layer that is not the last is folded into its successor on the host, in float64
 *         (W2 (W1 x + b1) + b2 = (W2 W1) x + W2 b1 + b2): the reference checkpoint's Linear-Linear-Tanh-Linear net
 *         (surrogates/models.py:114-123) runs as 5-32-6.  Same function, fewer layers; results differ from a
 *         layer-by-layer fp32 evaluation only by rounding. */
int ac_set_linear(ac_handle* h, const float* W);
int ac_set_poly(ac_handle* h, const float* coef, const float* intercept);
int ac_set_mlp(ac_handle* h, int n_layers, const int* widths, const int* act, const float* const* W,
               const float* const* b, const float* in_mean, const float* in_std, const float* out_mean,
               const float* out_std, int use_mfma);

/* x_dot = f(x,u)                                   — SixDOF.state_derivative, dynamics/base.py:385-406 */
int ac_state_derivative_f32(ac_handle* h, const float* X, const float* U, long n, float* Xdot, void* stream);

/* x+ = F(x,u,dt): `substeps` RK4 steps of dt/substeps — SixDOF.state_update, dynamics/base.py:450-480.
 * dt_per_unit: NULL -> every unit uses dt; else [n] per-unit step (dt_k = 1/progress_k^2, control/base.py:276). */
int ac_step_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n,
                float* Xn, void* stream);

/* Rollout X[k+1] = F(X[k], U[k], dt), k = 0..H-1    — Controller.initialise, main/control/control.py:72-93;
 * MHTT.initialise, control/moving_horizon.py:203-213.
 * X0 [13][B]; U [H][7][B]; Xout [H+1][13][B] with Xout[0] = X0. */
int ac_rollout_f32(ac_handle* h, const float* X0, const float* U, float dt, long B, long H, float* Xout,
                   void* stream);

/* Step + first-order sensitivities (the multiple-shooting defect Jacobian blocks):
 *   Xn [13][n], A = dF/dx [13][13][n], Bm = dF/du [13][7][n], c = dF/d(dt) [13][n] (c may be NULL)
 *                                                   — ca.jacobian(state_update, .), control/aircraft.py:85-95 */
int ac_step_sens_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n,
                     float* Xn, float* A, float* Bm, float* c, void* stream);

/* Multiple-shooting forms: every (instance b, node k) pair of a trajectory is an independent unit
 * (x_{k+1} - F(x_k, u_k, dt_k) = 0, control/base.py:275-286, built for k = 0..N-1 by setup(), :423-443).
 * Buffers are rollout-shaped and used IN PLACE (no transpose): X [>=H][13][B] (nodes 0..H-1 are read),
 * U [H][7][B], dt_per_unit NULL or [H][B]; outputs Xn [H][13][B] (= F(x_k,u_k): subtract from X[k+1] for the
 * defect), A [H][13][13][B], Bm [H][13][7][B], c [H][13][B] (c may be NULL). */
int ac_shoot_step_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                      long H, float* Xn, void* stream);
int ac_shoot_sens_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                      long H, float* Xn, float* A, float* Bm, float* c, void* stream);

/* x_dot = f(x, u) with its Jacobians Fx = df/dx [13][13][n], Fu = df/du [13][7][n] — ca.jacobian(state_derivative, .):
 * the implicit defect row  x_{k+1} - x_k - dt_k f(x_{k+1}, u_k)  (control/base.py:282-284), the Baumgarte row (:288-304)
 * and the LQR wrapper (dynamics/base.py:51-52) differentiate f, not the step.  df/dp = 0 and df/d(thrust) = 0 exactly.
 * ac_shoot_derivative_sens_f32 reads H nodes of rollout-shaped X [>=H][13][B], U [H][7][B] in place (pass X + 13 B to
 * evaluate at the NEXT nodes x_1..x_H with the controls u_0..u_{H-1}) and writes Xdot [H][13][B], Fx [H][13][13][B],
 * Fu [H][13][7][B]. */
int ac_state_derivative_sens_f32(ac_handle* h, const float* X, const float* U, long n, float* Xdot, float* Fx, float* Fu,
                                 void* stream);
/* x_dot alone on H nodes of rollout-shaped X [>=H][13][B], U [H][7][B] in place -> Xdot [H][13][B]: the residual of the
 * implicit defect row (control/base.py:282-284) needs f(x_{k+1}, u_k) but no Jacobian. */
int ac_shoot_derivative_f32(ac_handle* h, const float* X, const float* U, long B, long H, float* Xdot, void* stream);
int ac_shoot_derivative_sens_f32(ac_handle* h, const float* X, const float* U, long B, long H, float* Xdot, float* Fx,
                                 float* Fu, void* stream);

/* Envelope rows of AircraftControl.state_constraint (control/aircraft.py:44-59) and their state Jacobian:
 *   rows[0] = v_rel . v_rel   (bounded 20^2 .. 100^2)        rows[1] = beta   (|.| <= 10 deg)
 *   rows[2] = alpha           (|.| <= 20 deg)                rows[3] = z = x[2]   (< 0)
 * rows [4][n]; Jx = d rows / dx [4][13][n] (may be NULL).  The rows do not depend on the control.  Shooting form:
 * X [>=H][13][B] in place -> rows [H][4][B], Jx [H][4][13][B].  Fixed-wing plugin only (AC_ERR_UNSUPPORTED for the quadrotor). */
int ac_envelope_f32(ac_handle* h, const float* X, long n, float* rows, float* Jx, void* stream);
int ac_shoot_envelope_f32(ac_handle* h, const float* X, long B, long H, float* rows, float* Jx, void* stream);

/* The envelope as a SOFT constraint of the batched solver sweep (build-side, SURVEY §8 f1: the state_constraint role of
 * control/aircraft.py:44-59 — IPOPT enforces the rows, the iLQR sweep penalises their violation):
 *   penalty(x) = weight * sum_r max(0, g_r(x) - hi_r)^2 + max(0, lo_r - g_r(x))^2,   g = (|v_rel|^2, beta, alpha, z)
 * ac_envelope_cost_f32:   cost[b] += sum_{k=0..H} penalty(x_k)            X [H+1][13][B], cost [B]
 * ac_envelope_model_f32:  its quadratic model around X for the backward pass: node_glin [H+1][13][B] += 2 w sum_r viol_r grad g_r,
 *                         Hz [H][21][21][B] (x,x block) += 2 w sum_{r violated} grad g_r grad g_r'  (either of node_glin, Hz may be NULL). */
typedef struct ac_envelope_penalty { float lo[4], hi[4], weight; } ac_envelope_penalty;
int ac_envelope_cost_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* cost,
                         void* stream);
int ac_envelope_model_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* node_glin,
                          float* Hz, void* stream);
/* The envelope as a HARD constraint of the sweep, augmented-Lagrangian form: multipliers lam [H+1][8][B] (device; rows 0-3
 * the upper, 4-7 the lower bounds of the four envelope rows; all >= 0; start at zero) per node, row and instance —
 *   L_A = w sum_r max(0, g_r - hi_r + lam_hi / 2w)^2 - (lam_hi / 2w)^2 + max(0, lo_r - g_r + lam_lo / 2w)^2 - (lam_lo / 2w)^2
 * i.e. the penalty above on bounds shifted inwards by lam / 2w.  ac_envelope_al_cost_f32 / _model_f32 are the two calls above
 * with that shift (lam NULL = the plain penalty; a cost batch wider than Bl — the line-search candidates — reads the
 * multipliers of instance b % Bl); ac_envelope_al_update_f32 is the first-order multiplier update at the iterate X,
 *   lam_hi <- max(0, lam_hi + 2 w (g - hi)),   lam_lo <- max(0, lam_lo + 2 w (lo - g)),
 * and (viol_max [B] non-NULL, zeroed by the caller) reports each instance's largest bound excess over all nodes and rows,
 * relative to the row's range where it has one.  The weight must be > 0. */
int ac_envelope_al_cost_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* lam, long Bl, const float* X, long B,
                            long H, float* cost, void* stream);
int ac_envelope_al_model_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* lam, const float* X, long B, long H,
                             float* node_glin, float* Hz, void* stream);
int ac_envelope_al_update_f32(ac_handle* h, const ac_envelope_penalty* pen, const float* X, long B, long H, float* lam,
                              float* viol_max, void* stream);

/* Quaternion rows of ControlProblem.state_constraint on H nodes of X [>=H][13][B] (control/base.py:285-304):
 *   mode 0 ('constraint'):  row = q . q - 1                                                        (:285-286)
 *   mode 1 ('baumgarte'):   row = 2 a phi_dot + b^2 phi,  phi = q . q - 1,  phi_dot = 2 q . q_dot,  a = b = 2   (:288-304)
 * row [H][B], Jx = d row / dx [H][13][B], Ju = d row / du [H][7][B].  Mode 1 needs Xdot, Fx, Fu of the same (x, u) from
 * ac_shoot_derivative_sens_f32 (NULL allowed in mode 0). */
int ac_quat_rows_f32(ac_handle* h, int mode, const float* X, const float* Xdot, const float* Fx, const float* Fu, long B,
                     long H, float* row, float* Jx, float* Ju, void* stream);

/* Second-order step sensitivities: Hout [21][21][n] = sum_i lambda_i d2F_i / dz dz over z = (x[13], u[7], dt) — the
 * block the defect rows x_{k+1} - F(x_k, u_k, dt_k) (control/base.py:279-280) contribute to IPOPT's `nlp_hess_l`
 * (the reference's largest time sink, todo.md:102).  lambda [13][n] (device) are the multipliers of the 13 rows of F.
 * Exact second-order forward mode of the same fp32 arithmetic as ac_step_f32.  Rows/columns of p (0-2) and of controls
 * without effect are zero.  All force models.  The MLP surrogate evaluates its second-derivative tensor with the MFMA
 * engine (hidden width 128 with one to three hidden 128 x 128 products: forward tangents + a reverse sweep through the
 * transposed blocks, csrc/ac_hess_rev.hpp, which also keeps per-wave layer states in a handle-owned scratch of
 * CUs x 4 x (1 + 6 hidden products) x 8 KiB; otherwise one slab per derivative, csrc/ac_hess_nn.hpp)
 * into a handle-owned workspace of n*504 floats: size it once with ac_reserve_hess_workspace(h, n_max) — a
 * host-side call that may allocate — BEFORE the first compute call (and before capturing a hipGraph); the compute calls
 * themselves never allocate, free or synchronise and return AC_ERR_WORKSPACE when the workspace is too small.  The
 * workspace is one buffer per handle: second-order calls of one handle must be ordered on one stream (or use one handle
 * per stream).  physical_integration_substeps > 1 (the reference's default is 10, dynamics/base.py:12, 463-474) composes the
 * per-sub-step blocks: d2/dz2 = sum_s T_s' H_s T_s with T_s = d(x_{s-1}, u, dt/ns)/dz carried by the first-order chain and the
 * multipliers pulled back through the later sub-steps (mu_{s-1} = A_s' mu_s); it needs (559 ns + 481) n floats more of the
 * same reserved workspace, sized for the handle's sub-step count at the time of ac_reserve_hess_workspace.
 * AC_ERR_UNSUPPORTED for an MLP wider than 64 with use_mfma = 0 unless it has one to three hidden 128 x 128 products (the
 * reverse-sweep kernel has a cross-lane flavour, the slab-per-derivative kernel at that width has not).  Hout is zero-filled by the call (hipMemsetAsync on `stream`) before the active block is
 * written.  ac_shoot_hess_f32 reads rollout-shaped X [H(+1)][13][B], U [H][7][B], lambda [H][13][B] in place and writes
 * Hout [H][21][21][B]. */
int ac_step_hess_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit,
                     const float* lambda, long n, float* Hout, void* stream);
/* Size the second-order workspaces for n units: the MLP path's stage tensors (and the reverse sweep's scratch) and, when the
 * handle integrates with more than one RK4 sub-step, the composition buffers (hipFree + hipMalloc when one must grow: implicit device synchronisation,
 * not capturable); a no-op when both are already large enough.  Call again after changing `substeps`. */
int ac_reserve_hess_workspace(ac_handle* h, long n);
int ac_shoot_hess_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit,
                      const float* lambda, long B, long H, float* Hout, void* stream);

/* The defect rows of multiple shooting, written by the step / derivative kernels themselves
 *                                                  — ControlProblem.state_constraint, control/base.py:275-286.
 * X [H+1][13][B] (every node), U [H][7][B]; dt / dt_per_unit [H][B] as in ac_shoot_step_f32.  R [H][13][B]:
 *   ac_shoot_defect_f32             R_k = x_{k+1} - F(x_k, u_k, dt_k)                   ('explicit', :279-280)
 *   ac_shoot_implicit_defect_f32    R_k = x_{k+1} - x_k - dt_k f(x_{k+1}, u_k)          ('implicit', :282-284)
 *   ac_shoot_implicit_rows_f32      the same R with its Jacobian blocks: Jnext [H][13][13][B] = d R_k / d x_{k+1} =
 *                                   I - dt_k Fx, Ju [H][13][7][B] = d R_k / d u_k = -dt_k Fu, Jdt [H][13][B] =
 *                                   d R_k / d dt_k = -f  (d R_k / d x_k = -I is not stored). */
int ac_shoot_defect_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B, long H,
                        float* R, void* stream);
int ac_shoot_implicit_defect_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                                 long H, float* R, void* stream);
int ac_shoot_implicit_rows_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long B,
                               long H, float* R, float* Jnext, float* Ju, float* Jdt, void* stream);

/* Getters, out [22][n]: v_frd_rel(3), airspeed, alpha, beta, qbar, coefficients(6), forces_frd(3), moments_frd(3),
 * phi, theta, psi (Euler angles of q)        — dynamics/base.py:147-278, dynamics/aircraft.py:255-330, base.py:179-195 */
int ac_aero_f32(ac_handle* h, const float* X, const float* U, long n, float* out, void* stream);

/* Trajectory cost + best-K selection used by the sharded random-restart driver (build-side).
 * cost[b] = sum_k |p_k - goal|^2 * w_track  +  w_goal * |p_H - goal|^2 ; X is a rollout [H+1][13][B] (device),
 * goal3 is a HOST pointer to 3 floats, cost [B] (device). */
int ac_traj_cost_f32(ac_handle* h, const float* X, long B, long H, const float* goal3, float w_track, float w_goal,
                     float* cost, void* stream);

/* Second half of K6: the per-rank best-K select and the record pack in ONE launch.  cost [B] (device; NaN counts as
 * +inf, equal costs are ordered by instance index), X [H+1][13][B], U [H][7][B] rollout-shaped, 1 <= K <= min(8, B);
 * rec [K][1 + (H+1)*13 + H*7] = rows [cost, X(H+1,13) node-major, U(H,7) node-major] in ascending cost — the block each
 * rank hands to the path's one all-gather (8 056 B per row at H = 100). */
int ac_best_records_f32(ac_handle* h, const float* cost, const float* X, const float* U, long B, long H, int K,
                        float* rec, void* stream);
/* The gathered rows of all ranks sorted by cost: rec_in [n][R] -> rec_out [n][R] (n <= 1024 = K * world, column 0 is
 * the key; NaN -> +inf; stable).  rec_out must not alias rec_in. */
int ac_merge_records_f32(ac_handle* h, const float* rec_in, long n, long R, float* rec_out, void* stream);

/* ---- batched iLQR / Gauss-Newton sweep on (F, A, B)  (build-side) ---------------------------
 * Plays the `loss` and control-limit roles of ControlProblem (control/base.py:323-337, control/aircraft.py:29-41,
 * main/control/control.py:35-70) for B independent instances; the reference itself hands the NLP to IPOPT.
 *   J = sum_k 1/2 (x_k - x_ref)' diag(q) (x_k - x_ref) + 1/2 u_k' diag(r) u_k + 1/2 (x_N - x_goal)' diag(qf) (x_N - x_goal) */
typedef struct ac_ilqr_cost {
    float q[13], qf[13], r[7];
    float x_ref[13], x_goal[13];
    float u_min[7], u_max[7];  /* control box (aileron/elevator/rudder limits, control/aircraft.py:29-41) */
    float reg;                 /* Levenberg term on Quu */
    float u_lin[7];            /* + sum_k u_lin . u_k: linear control cost (w_time on the time row: the reference's time loss,
                                  main/control/control.py:44, 66-67) */
    int dt_row;                /* <= 0: fixed time.  r > 0: time is a decision variable per node (control/base.py:276, 339-385:
                                  dt_k = 1/progress_k^2 or progress_k^2, bounded by dt_bounds): control row dt_row — one the force
                                  model ignores (aircraft 3-5, quadrotor 4-6) — carries dt_k; u_min/u_max[dt_row] are dt_bounds
                                  (lower > 0).  The policy rollout integrates node k with the clipped u_k[dt_row]; the caller
                                  linearises with dt_per_unit = that row and puts c = dF/d(dt) into column dt_row of Bm. */
} ac_ilqr_cost;

/* Backward (Riccati) pass along X [H+1][13][B], U [H][7][B] with A [H][13][13][B], Bm [H][13][7][B] from
 * ac_shoot_sens_f32.  Outputs K [H][7][13][B], kff [H][7][B], dV [2][B] (expected-improvement terms). */
int ac_ilqr_backward_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* X, const float* U, const float* A,
                         const float* Bm, long B, long H, float* K, float* kff, float* dV, void* stream);
/* cost[b] of a trajectory batch X [H+1][13][B], U [H][7][B] */
int ac_ilqr_cost_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* X, const float* U, long B, long H,
                     float* out, void* stream);
/* Closed-loop rollout with a parallel line search: output instance o = a*B + b uses step alphas[a] (HOST array,
 * n_alpha <= 8):  u = clip(U_k[b] + alpha kff_k[b] + K_k[b] (x - Xnom_k[b])),  x+ = F(x, u, dt).
 * X0 [13][B]; Xout [H+1][13][n_alpha*B]; Uout [H][7][n_alpha*B].  MLP with use_mfma = 0: hidden widths 32 and 64
 * (AC_ERR_UNSUPPORTED otherwise). */
int ac_rollout_policy_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X0, const float* Xnom,
                          const float* U, const float* K, const float* kff, const float* alphas, int n_alpha, float dt,
                          long B, long H, float* Xout, float* Uout, void* stream);

/* Line-search acceptance, one launch: candidate a of instance b is column a*B + b of Xc [H+1][13][n_alpha*B],
 * Uc [H][7][n_alpha*B] (the layout ac_rollout_policy_f32 writes) with cost Jc [n_alpha*B]; J0 [B] is the cost of the
 * current iterate X [H+1][13][B], U [H][7][B].  Per instance: best = min_a Jc (non-finite costs never win, ties -> the
 * lowest a); if best < J0 the candidate's columns replace the iterate's IN PLACE.  Jout [B] = the accepted cost,
 * improved [B] = 0/1 bytes (may be NULL).  Jout must not alias J0 or Jc (AC_ERR_BAD_ARG): the workgroups that copy the
 * rows re-read both while Jout is being written. */
int ac_ilqr_accept_f32(ac_handle* h, const float* Jc, const float* J0, const float* Xc, const float* Uc, int n_alpha,
                       long B, long H, float* X, float* U, float* Jout, unsigned char* improved, void* stream);

/* Per-node, per-instance state cost for the two calls above (device arrays [H+1][13][Bn], node H = terminal):
 *   l_k(x) = 1/2 sum_j node_q[k][j] (x_j - node_xref[k][j])^2 + node_glin[k] . x
 * replacing the q, qf, x_ref, x_goal fields of the cost struct; r, limits and reg still come from it.  A batch wider than Bn
 * (the line-search candidates) reads instance b % Bn.  Produced by ac_track_progress_f32 for the MHTT loss. */
int ac_ilqr_backward_node_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* X, const float* U, const float* A, const float* Bm,
                              long B, long H, float* K, float* kff, float* dV, void* stream);
int ac_ilqr_cost_node_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                          const float* node_glin, long Bn, const float* X, const float* U, long B, long H, float* out,
                          void* stream);

/* The goal-acquisition loss of the reference's MPC driver — Controller.loss, main/control/control.py:44-68:
 *   J = w_goal |p_xy(N) - goal|^2 + w_rate sum_k sum_i l0(u_{k+1,i} - u_{k,i}; eps_rate) + w_height (z_N - z_0)^2
 *       - (w_speed / N) sum_{k<N} v_rel(x_k).v_rel(x_k) + w_vx v_x(N) + w_vyz (v_y(N)^2 + v_z(N)^2),   l0(d) = 1 - exp(-d^2/eps),
 *   subject to v_x(N) < vx_max (augmented Lagrangian, weight w_al, one multiplier per instance; w_al = 0: not enforced).
 * Reference values: w_goal 1000, w_rate 100, eps_rate 1e-2, w_height 1, w_speed 1/100, w_vx = vel_param * 1000, w_vyz 1000,
 * vx_max -2; the time term 10000 T is the linear control cost of the time row (ac_ilqr_cost::u_lin).
 *   ac_goal_cost_f32        cost_inout [B] += J of every column of X [H+1][13][B], U [H][7][B] (EXACT value); column o
 *                           belongs to instance o % Bn: goal [2][Bn], lam [Bn] (NULL = zeros)
 *   ac_goal_model_f32       the convex quadratic model around the iterate for the backward pass: WRITES node_q / node_xref /
 *                           node_glin [H+1][13][B] and node_uglin [H][7][B] (control gradient of the rate term, neighbours
 *                           held at the iterate), ADDS the rate term's Gauss-Newton curvature to the (u, u) diagonal of
 *                           Hz [H][21][21][B] (zero it or fill it with ac_shoot_hess_f32 / ac_envelope_al_model_f32 first)
 *   ac_goal_multiplier_f32  lam <- max(0, lam + 2 w_al (v_x(N) - vx_max)); viol [B] (may be NULL) = the excess before it
 *   ac_ilqr_backward_goal_f32  ac_ilqr_backward_newton_f32 with node_uglin added to Q_u */
typedef struct ac_goal_loss {
    float w_goal, w_rate, eps_rate, w_height, w_speed, w_vx, w_vyz;
    float vx_max, w_al;
    int time_row;   /* control row carrying dt_k, excluded from the rate term; <= 0: none */
} ac_goal_loss;
int ac_goal_cost_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, long Bn, const float* X,
                     const float* U, long B, long H, float* cost_inout, void* stream);
int ac_goal_model_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, const float* X,
                      const float* U, long B, long H, float* node_q, float* node_xref, float* node_glin, float* node_uglin,
                      float* Hz, void* stream);
int ac_goal_multiplier_f32(ac_handle* h, const ac_goal_loss* loss, const float* X, long B, long H, float* lam, float* viol,
                           void* stream);
int ac_ilqr_backward_goal_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* node_uglin, const float* Hz, const float* X,
                              const float* U, const float* A, const float* Bm, long B, long H, float* K, float* kff,
                              float* dV, void* stream);

/* The control-RATE term  sum_k rho_k(u_k - u_{k-1})  modelled exactly: the Riccati pass carries p_k = u_{k-1} as seven more
 * states (csrc/ac_ilqr_rate.hpp states the recursion).  rate_g, rate_h [H][7][B]: gradient and non-negative diagonal
 * curvature of rho_k with respect to the difference d_k = u_k - u_{k-1}; row 0 is the term against the control applied before
 * the window (all zeros: none).
 *   ac_ilqr_backward_rate_f32   ac_ilqr_backward_newton_f32 (node arrays and Hz optional, as there) with the rate model;
 *                               also returns Kp [H][7][7][B], the gains on the previous control
 *   ac_rollout_policy_rate_f32  ac_rollout_policy_f32 with the law
 *                               u_k = clip(U_k + alpha kff_k + K_k (x - Xnom_k) + Kp_k (u_applied_{k-1} - U_{k-1})),  k > 0
 *   ac_goal_model_rate_f32      ac_goal_model_f32's node arrays, and the l0 term per difference: rate_g = w_rate l0'(d_k),
 *                               rate_h = w_rate l0'^2 / (2 l0) (row 0 and the time row zero); nothing goes to Hz or uglin
 *   ac_ilqr_rate_model_f32      the quadratic rate cost  1/2 sum_k sum_i w_i (u_k,i - u_{k-1},i)^2  (rate_weight: HOST float[7],
 *                               finite, >= 0; u_prev [7][B] or NULL = no k = 0 term): rate_g = w d, rate_h = w
 *   ac_ilqr_rate_cost_f32       cost_inout[o] += that cost of column o of a candidate batch U [H][7][B] (B % Bn == 0); column o
 *                               reads the previous control of instance o % Bn (u_prev [7][Bn] or NULL) */
int ac_ilqr_backward_rate_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                              const float* node_glin, const float* Hz, const float* rate_g, const float* rate_h, const float* X,
                              const float* U, const float* A, const float* Bm, long B, long H, float* K, float* Kp, float* kff,
                              float* dV, void* stream);
int ac_rollout_policy_rate_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X0, const float* Xnom, const float* U,
                               const float* K, const float* Kp, const float* kff, const float* alphas, int n_alpha, float dt,
                               long B, long H, float* Xout, float* Uout, void* stream);
int ac_goal_model_rate_f32(ac_handle* h, const ac_goal_loss* loss, const float* goal, const float* lam, const float* X,
                           const float* U, long B, long H, float* node_q, float* node_xref, float* node_glin, float* rate_g,
                           float* rate_h, void* stream);
int ac_ilqr_rate_model_f32(ac_handle* h, const float* rate_weight, const float* U, const float* u_prev, long B, long H,
                           float* rate_g, float* rate_h, void* stream);
int ac_ilqr_rate_cost_f32(ac_handle* h, const float* rate_weight, const float* u_prev, long Bn, const float* U, long B, long H,
                          float* cost_inout, void* stream);

/* The control box IN the backward pass (control-limited DDP; Tassa, Mansard, Todorov, ICRA 2014).  The passes above solve the
 * unconstrained  kff = -Quu^-1 Qu, K = -Quu^-1 Qux  and leave the box to the clip of the closed-loop rollout.  These two solve,
 * per node,
 *     min_d  1/2 d'Quu d + Qu'd     subject to   u_min - U_k <= d <= u_max - U_k        (fp32, projected Newton: csrc/ac_boxqp.hpp)
 * and return  kff_k = d*,  rows of K_k (and Kp_k) at clamped controls exactly 0.0f, the other rows from the free block of Quu;
 * V and dV follow from the general formulas with these gains.  A row with u_min >= u_max is pinned: always clamped.  With a
 * feasible U, U + alpha kff is inside the box for every alpha in [0, 1].
 *   ac_ilqr_backward_box_f32       ac_ilqr_backward_newton_f32 / _goal_f32: node arrays and Hz optional, node_uglin optional and
 *                                  only with node arrays and Hz
 *   ac_ilqr_backward_rate_box_f32  ac_ilqr_backward_rate_f32
 * act  [H][7][B] int8 or NULL: 0 free, -1 clamped at the lower bound, +1 at the upper bound, 2 pinned.
 * stat [2][B] int32 or NULL: the largest Newton-iteration count over the instance's nodes; the number of nodes whose QP ended at
 *      a cap (16 iterations, 12 halvings) — the last iterate is kept there, feasible and no worse than the start.
 * AC_ERR_BAD_ARG for u_min[i] > u_max[i] or a non-finite bound.  Asynchronous on the stream, no allocation, capturable. */
int ac_ilqr_backward_box_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                             const float* node_glin, const float* node_uglin, const float* Hz, const float* X, const float* U,
                             const float* A, const float* Bm, long B, long H, float* K, float* kff, float* dV, signed char* act,
                             int* stat, void* stream);
int ac_ilqr_backward_rate_box_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                                  const float* node_glin, const float* Hz, const float* rate_g, const float* rate_h,
                                  const float* X, const float* U, const float* A, const float* Bm, long B, long H, float* K,
                                  float* Kp, float* kff, float* dV, signed char* act, int* stat, void* stream);

/* Gauss-Newton multiple shooting (Giftthaler et al. 2018): the iterate is (X, U) with X[0] = x0, every state a decision variable;
 * node k has the gap  d_k = F(x_k, u_k) - x_{k+1}  (ac_shoot_defect_f32 returns R_k = -d_k) and the linearised dynamics read
 * dx_{k+1} = A_k dx_k + B_k du_k + d_k.
 *   ac_ilqr_backward_shoot_f32  the backward pass of ac_ilqr_backward_newton_f32 / _goal_f32 (box == 0) or ac_ilqr_backward_box_f32
 *                               (box != 0; act / stat are used only then) in which node k reads  v = V'_x + V'_xx d_k  in place of
 *                               V'_x.  F [H][13][B] = F(x_k, u_k) (ac_shoot_sens_f32).  Vx [H][13][B], Vxx [H][13][13][B]: both or
 *                               neither (NULL); Vx[k], Vxx[k] = the value expansion of node k + 1, which node k starts from.
 *   ac_shoot_direction_f32      one forward sweep: dX [H+1][13][B] (dX[0] = 0), dU [H][7][B] = kff + K dx, the solution of the
 *                               equality-constrained QP, and Lam [H][13][B] (NULL, or with Vx and Vxx) = Vx[k] + Vxx[k] dx_{k+1}, the
 *                               multipliers of its defect rows.  limits (NULL, or with U [H][7][B]): the step of the controls
 *                               is clipped as it is formed, du_k = clip(U_k + kff_k + K_k dx_k, u_min, u_max) - U_k, and dX follows
 *                               the clipped step: for a feasible U every candidate U + alpha dU is then inside the box to a rounding.
 *   ac_shoot_merit_weight_f32   mu[b] = max(mu[b], factor max_{k,i} |Lam[k][i][b]|): the L1 penalty weight, never decreasing.
 *   ac_shoot_candidates_f32     column a B + b of Xc [H+1][13][n_alpha B], Uc [H][7][n_alpha B]:  Xc = X + alpha_a dX (row block 0:
 *                               X[0] bit for bit),  Uc = clip(U + alpha_a dU, limits->u_min, limits->u_max).
 *   ac_shoot_merit_f32          per column c of B:  phi[c] = J[c] + mu[c % Bn] sum_k sum_i |R[k][i][c]|  (rows in their order, no
 *                               atomics),  defect_inf[c] = max |R|.  R [H][13][B] (ac_shoot_defect_f32), or R == NULL and the
 *                               iterate's F [H][13][B], X [H+1][13][B] (then Bn == B): R = X[k+1] - F[k].  phi may be J.
 * AC_ERR_BAD_ARG for a NULL required pointer or Vx without Vxx; B == 0 is AC_OK.  Asynchronous on the stream, no allocation,
 * capturable. */
int ac_ilqr_backward_shoot_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                               const float* node_glin, const float* node_uglin, const float* Hz, const float* X, const float* U,
                               const float* A, const float* Bm, const float* F, long B, long H, float* K, float* kff, float* dV,
                               float* Vx, float* Vxx, int box, signed char* act, int* stat, void* stream);
int ac_shoot_direction_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X, const float* U, const float* F, const float* A,
                           const float* Bm, const float* K, const float* kff, const float* Vx, const float* Vxx, long B, long H,
                           float* dX, float* dU, float* Lam, void* stream);
int ac_shoot_merit_weight_f32(ac_handle* h, const float* Lam, float factor, long B, long H, float* mu, void* stream);
int ac_shoot_candidates_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* X, const float* U, const float* dX,
                            const float* dU, const float* alphas, int n_alpha, long B, long H, float* Xc, float* Uc, void* stream);
int ac_shoot_merit_f32(ac_handle* h, const float* J, const float* mu, long Bn, const float* R, const float* F, const float* X,
                       long B, long H, float* phi, float* defect_inf, void* stream);

/* Exact-Hessian (Newton / SQP) variant of the sweep, for the force models ac_shoot_hess_f32 supports:
 *   ac_ilqr_costate_f32        Lam [H][13][B]: multipliers of the defect rows at the current iterate,
 *                              Lam[H-1] = grad l_N(x_N), Lam[k-1] = grad l_k(x_k) + A_k' Lam[k]
 *   ac_shoot_hess_f32          Hz [H][21][21][B] = sum_i Lam[k][i] d2F_i/dz dz      (the nlp_hess_l blocks)
 *   ac_ilqr_backward_newton_f32  the backward pass with Hz's (x,x), (u,x), (u,u) blocks added to Qxx, Qux, Quu
 * node_q/node_xref/node_glin and Hz may be NULL (then this is ac_ilqr_backward_f32). */
int ac_ilqr_costate_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                        const float* node_glin, const float* X, const float* A, long B, long H, float* Lam,
                        void* stream);
int ac_ilqr_backward_newton_f32(ac_handle* h, const ac_ilqr_cost* cost, const float* node_q, const float* node_xref,
                                const float* node_glin, const float* Hz, const float* X, const float* U, const float* A,
                                const float* Bm, long B, long H, float* K, float* kff, float* dV, void* stream);

/* ---- track + progress terms of the moving-horizon track tracker   ---------------------------
 * Track: piecewise cubic Hermite curve over s in [0,1] through the sampled Dubins path
 * (control/initialisation.py:782-851).  `coef` is a HOST array [n_segments][3][4]: per segment and axis the cubic
 * c0 + c1 t + c2 t^2 + c3 t^3 in the local parameter t = s*n_segments - segment (the host layer computes the
 * Hermite slopes in float64, aircraft_amd/control/track.py); `length` is DubinsInitialiser.length()
 * (initialisation.py:738-758).  The handle keeps a device copy. */
int ac_set_track(ac_handle* h, int n_segments, const float* coef, float length);
/* pos [3][n], tangent [3][n] = track.eval(s), track.eval_tangent(s) for s [n] (device) */
int ac_track_eval_f32(ac_handle* h, const float* s, long n, float* pos, float* tangent, void* stream);

typedef struct ac_mhtt_weights { /* control/moving_horizon.py:47-55 */
    float w_tracking, w_progress, w_progress_rate, w_backward, w_terminal_align, w_low_velocity, w_control;
} ac_mhtt_weights;

/* Progress along the track for all nodes of all instances: X [H+1][13][B], s0 [B] -> S [H+1][B],
 * s_dot [H][B] (may be NULL), track_err [H][B] = |p_k - track(s_k)|^2 (may be NULL).
 *   mode 0: s_{k+1} = clip(s_k + s_dot dt, 0, 1)                    the initial guess, moving_horizon.py:216-233
 *   mode 1: s_{k+1} = clip(s_k + s_dot dt + 0.05 delta_s, 0, 1)     the constraint row at its bound, :161-168
 * If node_q/node_xref/node_glin [H+1][13][B] are non-NULL (all three), the diagonal-quadratic model of the MHTT
 * loss around this progress sequence is written for ac_ilqr_*_node_f32 (weights may be NULL otherwise). */
int ac_track_progress_f32(ac_handle* h, const ac_mhtt_weights* weights, const float* X, const float* s0, float dt,
                          long B, long H, int mode, float* S, float* s_dot, float* track_err, float* node_q,
                          float* node_xref, float* node_glin, void* stream);
/* J [B] = MHTT.loss (moving_horizon.py:44-105) of X [H+1][13][B], U [H][7][B] with progress S [H+1][B] */
int ac_mhtt_loss_f32(ac_handle* h, const ac_mhtt_weights* weights, const float* X, const float* U, const float* S,
                     long B, long H, float* J, void* stream);

/* ---- Reverse mode: vector-Jacobian products (autograd) ----------------------------------------------------------------------
 * One cotangent per unit instead of 21 tangents: the gradient of a scalar loss through the step, a rollout or f.
 *   ac_step_vjp_f32              Lam [13][n] (dLoss/dx+)  ->  Xbar = A' Lam [13][n], Ubar = B' Lam [7][n], dtbar = c . Lam [n]
 *                                (dtbar may be NULL).  A, B, c are the blocks of ac_step_sens_f32: every sub-step, the final
 *                                normalisation and dt_per_unit (NULL or [n]) exactly as ac_step_f32 applies them.  p never
 *                                enters f, so Xbar[0..2] of a step equals Lam[0..2].
 *   ac_rollout_vjp_f32           Xtraj [H+1][13][B] the saved forward trajectory (ac_rollout_f32's output), U [H][7][B],
 *                                G [H+1][13][B] = dLoss/dX[k] (the cotangent of every node, node 0 included)
 *                                ->  X0bar [13][B], Ubar [H][7][B], dtbar [B] (nullable: sum over nodes of c_k . lambda_{k+1})
 *                                by  lambda_H = G_H,  lambda_k = G_k + A_k' lambda_{k+1},  Ubar_k = B_k' lambda_{k+1},
 *                                X0bar = lambda_0.  The Jacobians are taken at the saved nodes.
 *   ac_state_derivative_vjp_f32  W [13][n] (dLoss/dx_dot)  ->  Xbar = (df/dx)' W [13][n], Ubar = (df/du)' W [7][n];
 *                                Xbar[0..2] = 0.
 * Routes (ac_set_vjp_route; AC_VJP_AUTO picks the first that applies):
 *   fused     default / linear / cubic-fit models with substeps <= 40: k_step_vjp, k_rollout_vjp, k_deriv_vjp — one lane per
 *             unit (instance), the RK4 stages recomputed and pulled back in registers and LDS; no workspace
 *   composed  the MLP surrogate and the quadrotor (any model on request): ac_step_sens_f32 / ac_shoot_sens_f32 /
 *             ac_state_derivative_sens_f32 write A, B (, c) into the WORKSPACE, then k_vjp_contract applies the cotangent
 *             (k_vjp_recur runs the rollout's reverse recurrence)
 * ws / ws_floats: caller-owned device scratch of at least ac_vjp_workspace_floats(h, which, n or B, H) floats (0 for the
 * fused route: ws may then be NULL); smaller returns AC_ERR_WORKSPACE.  The composed route's buffers are therefore the
 * caller's: the handle reserves nothing, and a caller that captures a hipGraph allocates the workspace before capture.
 * Like every compute call: asynchronous on `stream`, no allocation, no synchronisation, hipGraph-capturable. */
typedef enum ac_vjp_which { AC_VJP_STEP = 0, AC_VJP_ROLLOUT = 1, AC_VJP_DERIVATIVE = 2 } ac_vjp_which;
typedef enum ac_vjp_route { AC_VJP_AUTO = 0, AC_VJP_FUSED = 1, AC_VJP_COMPOSED = 2 } ac_vjp_route;
int ac_set_vjp_route(ac_handle* h, int route);  /* AC_VJP_FUSED on a model without fused kernels: the calls return AC_ERR_UNSUPPORTED */
int ac_vjp_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats);
int ac_step_vjp_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                    float* Xbar, float* Ubar, float* dtbar, float* ws, size_t ws_floats, void* stream);
int ac_rollout_vjp_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                       float* Ubar, float* dtbar, float* ws, size_t ws_floats, void* stream);
int ac_state_derivative_vjp_f32(ac_handle* h, const float* X, const float* U, long n, const float* W, float* Xbar, float* Ubar,
                                float* ws, size_t ws_floats, void* stream);

/* ---- Reverse mode to the WEIGHTS of the MLP surrogate --------------------------------------------------------
 * The gradient of  sum over units of Lam . F(x, u, dt; theta)  over the weights and biases of the net AS THE HANDLE HOLDS IT:
 * ac_set_mlp folds every activation-free layer that is not the last into its successor, so the folded net has tanh on every
 * layer but the last.
 *   ac_mlp_folded_shape     n_layers and widths [n_layers + 1] (5 ... 6; room for AC_MAX_LAYERS + 1) of the folded net
 *   ac_mlp_grad_floats      length of the gradient vector: per folded layer W[l] ([nout][nin] row-major, logical sizes, no
 *                           padding) followed by b[l]
 *   ac_step_wgrad_seeds_f32 Lam [13][n] -> per RK4 stage s the normalised network input Z [4][5][n] and the cotangent of the
 *                           raw network output Ybar [4][6][n] (output scale and stall factors applied): the weight gradient of
 *                           ANY differentiable surrogate evaluated at Z is its ordinary backward pass with Ybar
 *   ac_step_wgrad_f32       Wbar [ac_mlp_grad_floats] (overwritten): the seeds, then the net's backward pass over the 4 n
 *                           samples on the matrix cores (k_mlp_wgrad), one partial per workgroup in the workspace, added in a
 *                           fixed order: the same inputs give the same bits
 *   ac_rollout_wgrad_f32    Xtraj, U, G as ac_rollout_vjp_f32: the reverse recurrence lambda_k = G_k + A_k' lambda_{k+1} (the
 *                           composed route, lambda kept in the workspace), then the step gradient over the B H units
 *                           (X_k, U_k, lambda_{k+1})
 * One RK4 sub-step only: physical_integration_substeps > 1 returns AC_ERR_UNSUPPORTED, as do a net with tanh on its last layer
 * and a width-128 net with more than three hidden-to-hidden layers.  A model other than the MLP: AC_ERR_UNSUPPORTED.
 * ws / ws_floats: caller-owned device scratch of at least ac_wgrad_workspace_floats(h, which, n or B, H) floats, else
 * AC_ERR_WORKSPACE.  Asynchronous on `stream`, no allocation, no synchronisation, hipGraph-capturable. */
typedef enum ac_wgrad_which { AC_WGRAD_SEEDS = 0, AC_WGRAD_STEP = 1, AC_WGRAD_ROLLOUT = 2 } ac_wgrad_which;
int ac_mlp_folded_shape(const ac_handle* h, int* n_layers, int* widths);
int ac_mlp_grad_floats(const ac_handle* h, size_t* floats);
int ac_wgrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats);
int ac_step_wgrad_seeds_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n,
                            const float* Lam, float* Z, float* Ybar, float* ws, size_t ws_floats, void* stream);
int ac_step_wgrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Wbar, float* ws, size_t ws_floats, void* stream);
int ac_rollout_wgrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* Wbar,
                         float* ws, size_t ws_floats, void* stream);

/* ---- Reverse mode to the COEFFICIENTS of the cubic-fit and the linear model ----------------------------------
 * The gradient of  sum over units of Lam . F(x, u, dt; theta)  (step) or  sum over nodes of G_k . X_k  (rollout) over the model's
 * own parameters, in the order they were installed:
 *   poly    theta = coef [6][34] then intercept [6] (ac_set_poly): 210 floats
 *   linear  theta = W [6][6] (ac_set_linear; the last column is the bias): 36 floats
 * One fused reverse sweep per call (k_step_cgrad: one lane per unit; k_rollout_cgrad: one lane per instance, as
 * ac_rollout_vjp_f32): it also writes Xbar / Ubar / dtbar (X0bar / Ubar / dtbar) where those pointers are not NULL — the
 * values of ac_step_vjp_f32 / ac_rollout_vjp_f32 on the fused route — so a backward pass that needs the state, control, dt
 * and coefficient gradients is one launch.  Thetabar [ac_coef_grad_floats] is overwritten.  Sub-steps: supported up to 30
 * (above: AC_ERR_UNSUPPORTED); per-unit dt: accepted by the step.  The default model, the quadrotor and the MLP surrogate
 * (see ac_step_wgrad_f32 for its weights) return AC_ERR_UNSUPPORTED.
 * Accumulation without atomics, in a fixed order: per-lane accumulators in LDS, one partial per workgroup in the workspace,
 * the partials added in workgroup order.  The number of workgroups follows from the handle (CU count read by ac_create) and
 * the problem size alone; ac_set_cgrad_grid caps it (0 = auto; for tests and A/B runs).  The same inputs on the same handle and
 * grid give the same bits, eager or under graph replay.
 * ws / ws_floats: caller-owned device scratch of at least ac_cgrad_workspace_floats(h, which, n or B, H) floats (for the grid
 * in force at the call), else AC_ERR_WORKSPACE.  Asynchronous on `stream`, no allocation, no synchronisation,
 * hipGraph-capturable. */
typedef enum ac_cgrad_which { AC_CGRAD_STEP = 0, AC_CGRAD_ROLLOUT = 1 } ac_cgrad_which;
int ac_coef_grad_floats(const ac_handle* h, size_t* floats);
int ac_cgrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats);
int ac_set_cgrad_grid(ac_handle* h, int max_workgroups);
int ac_step_cgrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Xbar, float* Ubar, float* dtbar, float* Thetabar, float* ws, size_t ws_floats, void* stream);
int ac_rollout_cgrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                         float* Ubar, float* dtbar, float* Thetabar, float* ws, size_t ws_floats, void* stream);

/* ---- Reverse mode to the AIRFRAME CONSTANTS: mass, inertia, centre of mass ----------------------------------
 * The gradient of  sum over units of Lam . F(x, u, dt; phi)  (step) or  sum over nodes of G_k . X_k  (rollout) over the 22
 * floats of ac_params that enter f, in this order:
 *   Phibar [0]       mass
 *   Phibar [1..9]    inertia [9], row-major
 *   Phibar [10..18]  inertia_inv [9], row-major
 *   Phibar [19..21]  com [3]
 * The entries of inertia and inertia_inv are differentiated as INDEPENDENT numbers, exactly as the kernels read them: that
 * inertia is built from mass and com, that it is symmetric and that inertia_inv is its inverse is the caller's chain rule
 * (aircraft_amd.autodiff.AirframeParameters.derived()).  com enters through M = Ma + com x F only.  S, b, c and
 * rudder_moment_arm have no gradient here.
 * One fused reverse sweep per call (k_step_agrad, k_rollout_agrad), the default, linear and cubic-fit models; like
 * ac_*_cgrad_f32 it also writes Xbar / Ubar / dtbar (X0bar / Ubar / dtbar) where those pointers are not NULL, accumulates
 * without atomics in a fixed order and takes its grid from the handle and the problem size (ac_set_cgrad_grid caps it).
 * Phibar [AC_AIRFRAME_GRAD_FLOATS] is overwritten.  Sub-steps: up to 40, the limit of the fused VJP route (above:
 * AC_ERR_UNSUPPORTED); per-unit dt: accepted by the step.  The MLP surrogate and the quadrotor return AC_ERR_UNSUPPORTED.
 * ws / ws_floats: caller-owned device scratch of at least ac_agrad_workspace_floats(h, which, n or B, H) floats (which: an
 * ac_cgrad_which), else AC_ERR_WORKSPACE.  Asynchronous on `stream`, no allocation, no synchronisation, hipGraph-capturable. */
#define AC_AIRFRAME_GRAD_FLOATS 22
int ac_agrad_workspace_floats(const ac_handle* h, int which, long n_or_B, long H, size_t* floats);
int ac_step_agrad_f32(ac_handle* h, const float* X, const float* U, float dt, const float* dt_per_unit, long n, const float* Lam,
                      float* Xbar, float* Ubar, float* dtbar, float* Phibar, float* ws, size_t ws_floats, void* stream);
int ac_rollout_agrad_f32(ac_handle* h, const float* Xtraj, const float* U, float dt, long B, long H, const float* G, float* X0bar,
                         float* Ubar, float* dtbar, float* Phibar, float* ws, size_t ws_floats, void* stream);

/* ---- steady-flight trim (fixed-wing models) ------------------------------------------------------------------
 * Per instance, find z = (alpha, theta, phi [rad], aileron, elevator [deg], rudder [deg] | beta [rad]) such that the flight
 * given by target (p, V, psi, turn rate psid about NED down, and beta or rudder) is steady:
 *     q = Euler-to-quaternion(phi, theta, psi) (xyzw, body -> NED; the convention ac_aero_f32's phi/theta/psi rows invert)
 *     v_b = V (cos a cos b, sin b, sin a cos b),  v_ned = q v_b q^-1,  omega_b = q^-1 (0, 0, psid) q
 *     u = (aileron, elevator, rudder, Uhold rows 3-6)
 *     r_v = q^-1 f[3:6] q - omega_b x v_b   (m/s^2),   r_w = f[10:13]   (rad/s^2),   f = ac_state_derivative_f32(x, u)
 * r = 0 exactly when body velocity and body rates are constant; with psid = 0 it is the reference's trim objective
 * |v_dot_ned|^2 + |omega_dot|^2 = 0 at omega = 0 (a steady glide sinks with v_dot_ned = 0).
 * lateral 0: beta = target row 6 is held and the rudder is z[5]; lateral 1: the rudder = target row 6 is held and beta is z[5]
 * (the linear model has no rudder column: trim its turns in mode 1).
 * Solver: `iters` Levenberg-Marquardt iterations with projection onto [lo, hi], each three launches on `stream`:
 * k_trim_assemble (z -> x, u), the handle's ac_state_derivative_sens_f32 launch (f, df/dx, df/du), k_trim_update (r and
 * dr/dz, accept / reject, the next candidate by a 6x6 Cholesky solve).  An instance whose max|r_v| <= tol_v and
 * max|r_w| <= tol_w is frozen: later iterations leave its results bit-identical.  Z0 [6][n] is the initial guess (projected
 * onto the bounds).  Outputs: X [13][n], U [7][n], Z [6][n] at the best z found, R [6][n] = (r_v, r_w) there, and status [n]:
 *   0 converged, 1 not converged within iters, 2 stopped on a bound with the residual above tolerance,
 *   3 non-finite (V <= 0, a NaN or Inf input, or a model that returns no finite residual at the guess).
 * ws / ws_floats: caller-owned device scratch of at least ac_trim_workspace_floats(h, n) floats, else AC_ERR_WORKSPACE.
 * AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for iters < 1, n < 0, !(lo <= hi), tol <= 0, NULL pointers or an
 * unknown lateral mode.  Like every compute call: asynchronous, no allocation, no synchronisation, hipGraph-capturable. */
typedef struct ac_trim_opts {
    int lateral;         /* 0: beta held, rudder solved; 1: rudder held, beta solved */
    float tol_v, tol_w;  /* convergence: max |r_v| (m/s^2), max |r_w| (rad/s^2) */
    float lo[6], hi[6];  /* bounds of z = (alpha, theta, phi [rad], aileron, elevator [deg], rudder [deg] | beta [rad]) */
} ac_trim_opts;
int ac_trim_workspace_floats(const ac_handle* h, long n, size_t* floats);
int ac_trim_f32(ac_handle* h, const ac_trim_opts* o,
                const float* target /* [7][n]: p(3), V, psi, turn_rate, beta (mode 0) | rudder (mode 1) */,
                const float* Uhold /* [7][n]: rows 3-6 held, rows 0-2 ignored */, const float* Z0 /* [6][n] */, int iters, long n,
                float* X /* [13][n] */, float* U /* [7][n] */, float* Z /* [6][n] */, float* R /* [6][n] */, int* status /* [n] */,
                float* ws, size_t ws_floats, void* stream);

/* ---- LQR stabiliser about steady-flight trims (fixed-wing models) -------------------------------------------------
 * The steady-flight chart: for a state x and a nominal xb, with Z = R_z(yaw of q_b),
 *     xi = ( Z' (p - p_b),  R(q)' v - R(q_b)' v_b,  Z' 2 vec(q (x) q_b^-1),  omega - omega_b )
 * (R(q): body -> NED, quaternions normalised, the sign of q (x) q_b^-1 such that its scalar part is >= 0).  Coordinates:
 * 0 along-track, 1 cross-track, 2 down (heading frame), 3-5 body velocity, 6-7 tilt about the heading frame's forward and right
 * axes, 8 heading, 9-11 body rates.  Steady flight (an ac_trim_f32 result) is a fixed point of the chart.
 * ac_lqr_f32, per instance, at the nominal (X, U):
 *   1. the handle's own ac_step_sens_f32 launch writes x+ = F(x, u, dt), A, B into the workspace (every model and engine);
 *   2. k_lqr_project: A_xi = E(x+) A T(x) [12][12], B_xi = E(x+) B [12][7]  (T = dx/dxi, E = dxi/dx, analytic);
 *   3. k_lqr_dare: P = Q + A'PA - A'PB (R + B'PB)^-1 B'PA with Q = diag(q), R = diag(r) by `iters` steps of the structured
 *      doubling algorithm (an instance whose iterate moved by less than tol, relative in the max norm, is frozen: later
 *      steps leave it bit-identical), then K = (R + B'PB)^-1 B'PA [7][12] (u = u_b - K xi) and
 *      resid = max|Q + A'PA - A'PB K - P| / max|P|.
 * q[i] >= 0; q[i] == 0 for i in {0, 1, 2, 8} DROPS that coordinate (it feeds no other one: its rows and columns of P and its
 * column of K are exactly 0); r[j] > 0.  The thrust columns of B are exactly zero, so rows 3-5 of K are exactly 0.
 * status [n]: 0 converged, 1 not converged within iters, 2 breakdown (a pivot <= 0 or a non-finite intermediate: P, K, resid
 * are NaN), 3 non-finite input (NaN outputs).  used_iters [n]: doubling steps taken.  No instance affects another.
 * ws / ws_floats: caller-owned device scratch of at least ac_lqr_workspace_floats(h, n) floats, else AC_ERR_WORKSPACE; after
 * the call it holds x+ [13][n], A [13][13][n], B [13][7][n], each on a 256-byte boundary, in this order.
 * AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for iters < 1, n < 0, dt <= 0, a negative or non-finite q, r <= 0,
 * tol < 0 or NULL pointers.  Asynchronous, no allocation, no synchronisation, hipGraph-capturable.
 * ac_lqr_gains_f32: K_x,k = -K E(x_k) for the nodes k < H of Xnom [H+1][13][n] -> Kx [H][7][13][n], the gains
 * ac_rollout_policy_f32 reads (with kff = 0: u = clip(U_k + K_x,k (x - Xnom_k))).
 * ac_steady_error_f32: xi [12][n] of X about Xnom (both [13][n]); exactly 0 for X = Xnom. */
typedef struct ac_lqr_opts { float q[12]; float r[7]; float tol; } ac_lqr_opts;
int ac_lqr_workspace_floats(const ac_handle* h, long n, size_t* floats);
int ac_lqr_f32(ac_handle* h, const ac_lqr_opts* o, const float* X /* [13][n] */, const float* U /* [7][n] */, float dt, int iters,
               long n, float* Axi /* [12][12][n] */, float* Bxi /* [12][7][n] */, float* P /* [12][12][n] */,
               float* K /* [7][12][n] */, float* resid /* [n] */, int* status /* [n] */, int* used_iters /* [n] */, float* ws,
               size_t ws_floats, void* stream);
int ac_lqr_gains_f32(ac_handle* h, const float* Xnom, const float* K, long n, long H, float* Kx, void* stream);
int ac_steady_error_f32(ac_handle* h, const float* X, const float* Xnom, long n, float* xi, void* stream);

/* ---- extended Kalman filter over the step sensitivities (fixed-wing models) ---------------------------------------
 * Error state about an estimate x: d = (dp NED, dv NED, dtheta body-frame rotation vector, dw) [12], with
 *     x [+] d = ( p + dp, v + dv, (q (x) (dtheta/2, 1)) / |.|, w + dw )      (Hamilton, xyzw; no heading singularity).
 * One step, per instance:
 *   1. the handle's own ac_step_sens_f32 launch writes x- = F(x, u, dt), A, B into the workspace (every model and engine);
 *   2. k_ekf_step: Abar = E(x-) A G(x) [12][12] (G = d(x [+] d)/dd, E = dd/dx, analytic), P- = Abar P Abar' + diag(Qd), symmetrised;
 *      nu = z - h(x-) and H [15][12] (analytic) once, at x-; fifteen scalar updates in row order over the USED rows (mask bit
 *      set, NULL mask: all; and z finite):  s = h P h' + r,  rho = nu_i - h d,  d += P h' rho / s,  P -= (P h')(P h')' / s;
 *      x+ = x- [+] d (x- itself, bit for bit, when no row was applied).  No reset Jacobian is applied to P.
 * Measurement rows h(x): 0-2 GPS position p, 3-5 GPS velocity v (NED), 6-8 gyro w, 9-11 air data (V, alpha, beta [rad]) = rows
 * 3-5 of ac_aero_f32 bit for bit, 12-14 magnetometer R(q/|q|)' mag_ned.  R = diag(Rd).
 * Outputs: Xo [13][n], Po [12][12][n] (bitwise symmetric); nu, S [15][n]: rho and s of every used row in the order they were
 * applied (the innovation of row i given the rows before it; nu = z - h(x-) for the first), 0 for unused rows; nis [n] =
 * sum rho^2 / s (= nu' S^-1 nu of the batch update); ll [n] = -1/2 sum (log 2 pi s + rho^2 / s); used [n]: bits of the used rows;
 * status [n]: 0, or bit 1 (value 1): a used row had s <= 0 or a non-finite s and was skipped; bit 2 (value 2): the prediction
 * (x-, P-) is not finite: Xo, Po are the prediction, no row is applied, nu = S = nis = ll = used = 0.  No instance affects
 * another; no atomics, every sum in a fixed order: an instance's bits depend neither on n nor on its place in the batch.
 * Xpred [13][n], Ppred, Abar [12][12][n]: optional (NULL), the prediction and the projected Jacobian (what ac_ekf_smooth_f32 reads).
 * predict == 0: the measurement update alone (Abar = I, U, dt, Qd ignored and may be NULL / 0, no sensitivity launch).
 * ws / ws_floats: caller-owned device scratch of at least ac_ekf_workspace_floats floats, else AC_ERR_WORKSPACE; after a
 * predicting step it holds x- [13][n], A [13][13][n], B [13][7][n], each on a 256-byte boundary, in this order.
 * ac_ekf_filter_f32: T steps as a host loop over the step (U [T][7][n], Z [T][15][n], mask [T][n] or NULL), the estimate
 * ping-ponging through the workspace; Xo, Po: the final estimate; ll [n]: summed over the steps in step order; the per-step
 * outputs Xs [T][13][n], Ps [T][12][12][n], nu, S [T][15][n], nis, used, status [T][n] may each be NULL.
 * ac_ekf_filter_rec_f32: ac_ekf_filter_f32 with three more per-step outputs after status, the records a smoother reads:
 * Xpreds [T][13][n], Ppreds, Abars [T][12][12][n] (each may be NULL), bit for bit what T calls of ac_ekf_step_f32 write to
 * Xpred, Ppred, Abar; every other output is ac_ekf_filter_f32's bit for bit.
 * ac_ekf_measure_f32: Z [15][n] = h(X) (predict is ignored).
 * AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for n < 0, T < 0, a NULL required pointer, or (predict set) a dt that
 * is not finite and > 0; n == 0 or T == 0 is AC_OK.  Asynchronous, no allocation, no synchronisation, hipGraph-capturable. */
typedef struct ac_ekf_opts { float mag_ned[3]; int predict; } ac_ekf_opts;
int ac_ekf_workspace_floats(const ac_handle* h, long n, size_t* floats);
int ac_ekf_measure_f32(ac_handle* h, const ac_ekf_opts* o, const float* X /* [13][n] */, long n, float* Z /* [15][n] */, void* stream);
int ac_ekf_step_f32(ac_handle* h, const ac_ekf_opts* o, const float* X /* [13][n] */, const float* P /* [12][12][n] */,
                    const float* U /* [7][n] */, float dt, const float* Z /* [15][n] */, const int* mask /* [n] bits 0-14 | NULL */,
                    const float* Qd /* [12][n] */, const float* Rd /* [15][n] */, long n, float* Xo, float* Po,
                    float* nu /* [15][n] */, float* S /* [15][n] */, float* nis, float* ll /* [n] */, int* used /* [n] */,
                    int* status /* [n] */, float* Xpred, float* Ppred, float* Abar /* optional, may be NULL */, float* ws,
                    size_t ws_floats, void* stream);
int ac_ekf_filter_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U /* [T][7][n] */, float dt,
                      const float* Z /* [T][15][n] */, const int* mask /* [T][n] | NULL */, const float* Qd, const float* Rd,
                      long n, long T, float* Xo, float* Po, float* ll /* [n] */, float* Xs, float* Ps, float* nu, float* S,
                      float* nis, int* used, int* status /* per step, each may be NULL */, float* ws, size_t ws_floats,
                      void* stream);
int ac_ekf_filter_rec_f32(ac_handle* h, const ac_ekf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status,
                          float* Xpreds, float* Ppreds, float* Abars /* per step, each may be NULL */, float* ws, size_t ws_floats,
                          void* stream);

/* ---- unscented Kalman filter beside the EKF bank (fixed-wing models) ------------------------------------------------
 * The EKF's error state, chart, measurement rows h(x) [15], diagonal Qd, Rd and mask / NaN rule, with sigma points in place of
 * Jacobians: the second-order terms of f and h that one linearisation per step leaves out are carried.  kappa >= 0 (default 0):
 * gamma = sqrt(12 + kappa), weights w0 = kappa / (12 + kappa) for the centre and 1 / (2 (12 + kappa)) for the 24 other points.
 * One step, per instance:
 *   1. k_ukf_sigma: L L' = P (plain Cholesky), the points x and x [+] (+-gamma L.j) and the replicated U into the workspace;
 *   2. the handle's own ac_step_f32 launch over the 25 n units (every model and engine);
 *   3. k_ukf_update: e_j = F(chi_j) [-] F(chi_0), dbar = sum w_j e_j, x- = F(chi_0) [+] dbar, P- = sum w_j (e_j - dbar)(e_j - dbar)'
 *      + diag(Qd); L- L-' = P-, z_j = h(x- [+] (+-gamma L-.j)), zbar = sum w_j z_j, Pzz = sum w_j (z_j - zbar)(z_j - zbar)' + diag(Rd),
 *      Pxz = L- Y' with Y.j = (z_+j - z_-j) / (2 gamma); a Cholesky of Pzz in row order over the USED rows (an unused row is a
 *      unit row), L_S; w = L_S^-1 (z - zbar), Yx = Pxz L_S^-', d = Yx w, P = P- - Yx Yx', x+ = x- [+] d (x- itself, bit for bit,
 *      when no row was applied).
 * Outputs have ac_ekf_step_f32's shapes and meaning: S_i = (L_S)_ii^2, the innovation variance of row i given the rows before
 * it; nu_i = (L_S)_ii w_i; nis = sum w_i^2; ll = -1/2 sum (log 2 pi S_i + w_i^2); used; unused rows give 0.  Po, Ppred are
 * symmetric bit for bit.  Abar (optional) = D L^-1 with D.j = (e_+j - e_-j) / (2 gamma): the statistical linearisation
 * Cov(d+, d) P^-1, with which ac_ekf_smooth_f32 on these records is the unscented RTS smoother (its gain P Abar' (P-)^-1 is
 * the sigma-point cross covariance times (P-)^-1).
 * status [n]: 0, or bit 1 (value 1): a used row's pivot was <= 0 or not finite, the row is skipped as if unused; bit 2
 * (value 2): the prediction is not finite (ac_ekf_step_f32's rule); bit 3 (value 4): a pivot of the factor of P or of P- was
 * <= 0 or not finite.  For P: the instance's 25 units are all x^, Xo = X and Po = P come back unchanged (Xpred = X, Ppred = P,
 * Abar = I), nu = S = nis = ll = used = 0.  For P-: Xo, Po are the prediction and no row is applied.
 * predict == 0: the measurement update alone at (X, P) (Abar = I; U, dt, Qd ignored; neither k_ukf_sigma nor a step launch).
 * ws / ws_floats: caller-owned device scratch of at least ac_ukf_workspace_floats floats, else AC_ERR_WORKSPACE.  After a
 * predicting step it holds, each on a 256-byte boundary and in this order: the sigma points [13][25 n] (unit j n + i is point j
 * of instance i: 0 the centre, 1 + j and 13 + j the points +-gamma L.j; position rows RELATIVE to the instance's p^), the
 * replicated U [7][25 n], their images [13][25 n] (positions still relative), L [12][12][n], the flag of P's factor [n] (int).
 * ac_ukf_filter_f32, ac_ukf_filter_rec_f32: ac_ekf_filter_f32's and ac_ekf_filter_rec_f32's host loop over the step, bit-equal
 * to T step calls.  AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for n < 0, T < 0, a NULL required pointer, (predict
 * set) a dt that is not finite and > 0, or a kappa that is not finite and >= 0; n == 0 or T == 0 is AC_OK.  Asynchronous, no
 * allocation, no synchronisation, hipGraph-capturable.  No atomics: an instance's bits depend neither on n nor on its place. */
typedef struct ac_ukf_opts { float mag_ned[3]; int predict; float kappa; } ac_ukf_opts;
int ac_ukf_workspace_floats(const ac_handle* h, long n, size_t* floats);
int ac_ukf_step_f32(ac_handle* h, const ac_ukf_opts* o, const float* X /* [13][n] */, const float* P /* [12][12][n] */,
                    const float* U /* [7][n] */, float dt, const float* Z /* [15][n] */, const int* mask /* [n] bits 0-14 | NULL */,
                    const float* Qd /* [12][n] */, const float* Rd /* [15][n] */, long n, float* Xo, float* Po,
                    float* nu /* [15][n] */, float* S /* [15][n] */, float* nis, float* ll /* [n] */, int* used /* [n] */,
                    int* status /* [n] */, float* Xpred, float* Ppred, float* Abar /* optional, may be NULL */, float* ws,
                    size_t ws_floats, void* stream);
int ac_ukf_filter_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U /* [T][7][n] */, float dt,
                      const float* Z /* [T][15][n] */, const int* mask /* [T][n] | NULL */, const float* Qd, const float* Rd,
                      long n, long T, float* Xo, float* Po, float* ll /* [n] */, float* Xs, float* Ps, float* nu, float* S,
                      float* nis, int* used, int* status /* per step, each may be NULL */, float* ws, size_t ws_floats,
                      void* stream);
int ac_ukf_filter_rec_f32(ac_handle* h, const ac_ukf_opts* o, const float* X, const float* P, const float* U, float dt,
                          const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T, float* Xo, float* Po,
                          float* ll, float* Xs, float* Ps, float* nu, float* S, float* nis, int* used, int* status,
                          float* Xpreds, float* Ppreds, float* Abars /* per step, each may be NULL */, float* ws, size_t ws_floats,
                          void* stream);

/* ---- the loop closed through the estimator: simulated sensors and the LQG rollout (fixed-wing models) ---------------
 * Noise: Philox4x32-10 with key (seed_lo, seed_hi) and counter (g low word, g high word, step, purpose), g = instance_offset + i
 * the GLOBAL instance; Box-Muller as ac_mppi_sample_f32 forms it.  Purposes 0-3: the four normals of measurement rows 4p .. 4p+3
 * (the sixteenth is dropped); 4: word j is the uniform (x >> 8) 2^-24 of sensor group j = 0 .. 3; 5: word 0 is group 4's; 6-8: the
 * twelve process-noise normals.  A draw depends on (seed, step, g, row) alone.  Sensor groups, three rows each: 0 GPS position,
 * 1 GPS velocity, 2 gyro, 3 air data, 4 magnetometer (ac_ekf_step_f32's rows).
 *   ac_sense_f32     at step s = step + (step_dev ? *step_dev : 0) (step_dev: a DEVICE int the caller increments, so that a captured
 *                    call draws fresh noise on every replay; the sum wraps): group j reports when (s - phase[j]) % period[j] == 0
 *                    (taken in 64-bit, so any int step and phase are allowed) and its uniform
 *                    is not below dropout[j].  A reporting row is Z = fmaf(sigma_r, normal, h(X)), h being ac_ekf_measure_f32's
 *                    values (so Z is that call's output bit for bit where sigma_r = 0); a group that does not report has its three
 *                    mask bits cleared and NaN in its rows.  sigma_r [15][n] must be finite and >= 0 (not checked on the device).
 *   ac_disturb_f32   Xo = X [+] (sigma_q . normals) in the EKF's chart, sigma_q [12][n]; Xo may be X.
 *   ac_policy_f32    U_r = clip(Unom_r + sum_c Kx[r][c] (Fb_c - Xnom_c), u_min_r, u_max_r), the sum as one fmaf per c = 0 .. 12 in
 *                    that order: ac_rollout_policy_f32's law with kff = 0 on whatever state Fb [13][n] it is handed.  Kx [7][13][n]
 *                    (ac_lqr_gains_f32, ILQR), Xnom [13][n], Unom [7][n]; `limits`: only u_min, u_max are read (infinite bounds
 *                    are allowed).
 *   ac_estimate_score_f32   e [12][n] = X [-] Xhat in the chart, nees [n] = e' P^-1 e by a plain Cholesky of P [12][12][n] (its lower
 *                    triangle is read) and one forward solve; status [n]: 1 when a pivot is <= 0 or not finite (nees = NaN), else 0.
 *   ac_lqg_rollout_f32      a host loop of launches; for k = 0 .. T-1:
 *                      1. u_k = policy(fb_k; Xnom_k, Unom_k, Kx_k), fb the estimate (AC_FB_ESTIMATE) or the truth (AC_FB_TRUTH);
 *                      2. x_{k+1} = F(x_k, u_k, dt) (the handle's ac_step_f32 launch, any engine), then, sigma_q given, [+] noise at
 *                         step step0 + k (sigma_q NULL: the step's output bit for bit);
 *                      3. (z, mask) = sense(x_{k+1}) at step step0 + k + 1;
 *                      4. ac_ekf_step_f32 / ac_ukf_step_f32 (predict set) with (x^_k, P_k, u_k, dt, z, mask, Qd, Rd);
 *                      5. the score of x_{k+1} against (x^_{k+1}, P_{k+1}).
 *                    The estimator's magnetometer model is the sensors' (s->mag_ned).
 *                    Every output equals, bit for bit, what these single calls give in that order.  Inputs X0, Xhat0 [13][n], P0
 *                    [12][12][n], Xnom [T+1][13][n] (node T is not read), Unom [T][7][n], Kx [T][7][13][n], Qd [12][n], Rd [15][n],
 *                    sigma_q [12][n] | NULL, sigma_r [15][n].  Outputs: the final estimate Xo, Po (required); per step, each may be
 *                    NULL: Xtrue, Xhat [T+1][13][n] (node 0 the inputs), U [T][7][n], Ps [T][12][12][n], Z [T][15][n], mask, used,
 *                    est_status, score_status [T][n] (int), nis, nees [T][n], err [T][12][n].
 * ws / ws_floats (the rollout only): caller-owned device scratch of at least ac_lqg_workspace_floats floats, else
 * AC_ERR_WORKSPACE: the estimator's own workspace followed by the loop's buffers, every region on a 256-byte boundary.
 * AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG (before any launch) for a NULL required pointer, n < 0, T < 0, a dt that is
 * not finite and > 0, a period < 1, a dropout outside [0, 1), u_min > u_max or a NaN bound, an unknown estimator or feedback, a
 * kappa that is not finite and >= 0, step0 + T > 2^31 - 1; n == 0 or T == 0 is AC_OK.  NaNs propagate (a non-finite truth gives NaN measurements, hence
 * unused rows); nothing is trapped.  Asynchronous, no allocation, no synchronisation, hipGraph-capturable.  No atomics: an
 * instance's bits depend neither on n nor on its place in the batch. */
typedef struct ac_sense_opts {
    float mag_ned[3];
    unsigned seed_lo, seed_hi;
    long instance_offset;
    int period[5], phase[5];   /* group j reports at steps with (step - phase[j]) % period[j] == 0, period >= 1 */
    float dropout[5];          /* probability in [0, 1) that a due group does not report */
} ac_sense_opts;
enum { AC_EST_EKF = 0, AC_EST_UKF = 1 };
enum { AC_FB_ESTIMATE = 0, AC_FB_TRUTH = 1 };
typedef struct ac_lqg_opts {
    int estimator;   /* AC_EST_EKF | AC_EST_UKF */
    int feedback;    /* AC_FB_ESTIMATE | AC_FB_TRUTH */
    float kappa;     /* AC_EST_UKF only (ac_ukf_opts) */
    int step0;       /* the step index of X0: node k + 1 is measured at step step0 + k + 1 */
} ac_lqg_opts;
int ac_sense_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev /* device, may be NULL */,
                 const float* X /* [13][n] */, const float* sigma_r /* [15][n] */, long n, float* Z /* [15][n] */,
                 int* mask /* [n] */, void* stream);
int ac_disturb_f32(ac_handle* h, const ac_sense_opts* o, int step, const int* step_dev, const float* X /* [13][n] */,
                   const float* sigma_q /* [12][n] */, long n, float* Xo /* [13][n], may be X */, void* stream);
int ac_policy_f32(ac_handle* h, const ac_ilqr_cost* limits, const float* Fb /* [13][n] */, const float* Xnom /* [13][n] */,
                  const float* Unom /* [7][n] */, const float* Kx /* [7][13][n] */, long n, float* U /* [7][n] */, void* stream);
int ac_estimate_score_f32(ac_handle* h, const float* X /* [13][n] */, const float* Xhat /* [13][n] */,
                          const float* P /* [12][12][n] */, long n, float* e /* [12][n] */, float* nees /* [n] */,
                          int* status /* [n] */, void* stream);
int ac_lqg_workspace_floats(const ac_handle* h, int estimator, long n, size_t* floats);
int ac_lqg_rollout_f32(ac_handle* h, const ac_lqg_opts* o, const ac_sense_opts* s, const ac_ilqr_cost* limits, const float* X0,
                       const float* Xhat0, const float* P0, const float* Xnom, const float* Unom, const float* Kx, const float* Qd,
                       const float* Rd, const float* sigma_q, const float* sigma_r, float dt, long n, long T, float* Xo, float* Po,
                       float* Xtrue, float* Xhat, float* U, float* Ps, float* Z, int* mask, float* nis, float* nees, int* used,
                       int* est_status, int* score_status, float* err, float* ws, size_t ws_floats, void* stream);

/* ---- RTS smoother over the trace of the extended Kalman filter (fixed-wing models) --------------------------------
 * The fixed-interval Rauch-Tung-Striebel estimate of every node of a recorded filter run, given the whole run: one launch
 * (k_ekf_smooth) sweeps backward in time, one instance per 16-lane group.  Nodes k = 0 .. T-1 are the filter's steps: Xf, Pf
 * the filtered estimate (ac_ekf_filter_rec_f32's Xs, Ps), Xpred, Ppred the prediction, Abar the Jacobian that maps the error
 * state of node k-1 to node k (its Xpreds, Ppreds, Abars).  X0, P0: the estimate the run started from, node "-1"; given (with
 * Xs0, Ps0) it is smoothed too.  Node T-1 is copied bit for bit.  Link k = T-1 .. 1 (and 0 with X0, P0), per instance:
 *     L L' = P-_k (plain Cholesky),   C_k = P_{k-1} Abar_k' (P-_k)^-1,   e = x^s_k [-] x-_k  ([-]: the inverse of [+]),
 *     x^s_{k-1} = x^_{k-1} [+] C_k e,   P^s_{k-1} = 1/2 (X + X'),  X = P_{k-1} + (C_k (P^s_k - P-_k)) C_k'.
 * As in the filter, no reset Jacobian is applied: P_k is taken as the covariance about x^_k.
 * Outputs: Xs [T][13][n], Ps [T][12][12][n] (bitwise symmetric); Xs0 [13][n], Ps0 [12][12][n] with X0, P0, else NULL; Cg
 * [T][12][12][n] or NULL: C_k of link k (entry 0 is zero without X0, P0); the lag-one smoothed covariance is
 * Cov(d_k, d_{k-1} | all data) = P^s_k C_k'.  status [T][n]: entry k describes link k (entry 0 is 0 without X0, P0): 0, or
 * value 2: an operand of the link (x^_{k-1}, P_{k-1}, x-_k, P-_k, Abar_k, the carried x^s_k, P^s_k) was not finite, else
 * value 1: a pivot of the Cholesky was <= 0 or not finite.  In both cases C_k = 0, node k-1 is the filtered (x^_{k-1}, P_{k-1})
 * bit for bit and the recursion goes on from it.  No instance affects another; no atomics, every sum in a fixed order: an
 * instance's bits depend neither on n nor on its place in the batch.
 * No workspace.  AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for n < 0, T < 0, a NULL required pointer, X0, P0, Xs0,
 * Ps0 not given all together, or an output that overlaps an input; n == 0 or T == 0 is AC_OK.  Asynchronous, no allocation,
 * no synchronisation, hipGraph-capturable. */
int ac_ekf_smooth_f32(ac_handle* h, const float* X0 /* [13][n] | NULL */, const float* P0 /* [12][12][n] | NULL */,
                      const float* Xf /* [T][13][n] */, const float* Pf /* [T][12][12][n] */, const float* Xpred, const float* Ppred,
                      const float* Abar, long n, long T, float* Xs /* [T][13][n] */, float* Ps /* [T][12][12][n] */,
                      float* Xs0, float* Ps0 /* with X0, P0; else NULL */, float* Cg /* [T][12][12][n] | NULL: C_k of link k */,
                      int* status /* [T][n] */, void* stream);

/* ---- EM statistics for the noise variances of the extended Kalman filter (fixed-wing models) -----------------------
 * The M-step of an EM estimate of the diagonal Q and R from a recorded filter run (ac_ekf_filter_rec_f32: Xpred, Ppred, used) and
 * its smoothed trace (ac_ekf_smooth_f32: Xs, Ps), per instance over the nodes k = 0 .. T-1.  Qd, Rd must be the variances THE
 * RECORDS WERE MADE WITH; mag_ned the filter's.
 *   Process noise, innovations form: with e = x^s_k [-] x-_k, y = (P-_k)^-1 e, W = (P-_k)^-1 (P-_k - P^s_k) (P-_k)^-1 (plain Cholesky
 *   of P-_k),  t_kj = Q_j + Q_j^2 (y_j^2 - W_jj) = E[w_kj^2 | all data];  Qsum [12][n] = sum_k t_kj over the counted nodes, nq [n] their
 *   number.  Node 0 counts like any other (its P-_0 contains Q); the initial node is not read.
 *   Sensor noise, relinearised at the smoothed state: for every node and row i whose `used` bit is set and whose z is finite,
 *   Rsum_i += (z_i - h_i(x^s_k))^2 + h_i P^s_k h_i',  nr_i += 1;  Rsum, nr [15][n]  (h, H: the filter's, evaluated at x^s_k).
 * status [T][n] per node: 0; value 2: an operand of the node (x-_k, P-_k, x^s_k, P^s_k, Qd) is not finite, the node adds nothing;
 * else value 1: a pivot of the Cholesky was <= 0 or not finite, the node adds nothing to Q and its R terms count.  A link the
 * smoother reported does not exclude a node.
 * Qn [12][n], Rn [15][n] (each may be NULL): the new variances max(sum / count, floor_rel * input); the input bit for bit where
 * the count is 0.  floor_rel must be finite and >= 0; 0 means 1e-4.
 * Two launches: k_ekf_em_nodes over (groups of 16 instances) x (chunks of 32 consecutive nodes), per-node terms in float32,
 * float64 sums in node order into the workspace; k_ekf_em_reduce sums the chunks in chunk order and rounds to float32 once.  No
 * atomics, every sum in a fixed order: an instance's bits depend neither on n nor on its place in the batch (they do depend
 * on the chunk length 32, which is part of the contract).
 * ws / ws_floats: caller-owned device scratch of at least ac_ekf_em_workspace_floats(h, n, T) floats, else AC_ERR_WORKSPACE.
 * AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG for n < 0, T < 0, a NULL required pointer, a floor_rel that is not finite
 * and >= 0, or an output that overlaps an input; n == 0 is AC_OK and launches nothing; T == 0 writes zero sums and counts and
 * Qn, Rn = Qd, Rd.  Asynchronous, no allocation, no synchronisation, hipGraph-capturable. */
typedef struct ac_ekf_em_opts { float mag_ned[3]; float floor_rel; } ac_ekf_em_opts;
int ac_ekf_em_workspace_floats(const ac_handle* h, long n, long T, size_t* floats);
int ac_ekf_em_f32(ac_handle* h, const ac_ekf_em_opts* o, const float* Xpred /* [T][13][n] */, const float* Ppred /* [T][12][12][n] */,
                  const float* Xs /* [T][13][n] */, const float* Ps /* [T][12][12][n] */, const float* Z /* [T][15][n] */,
                  const int* used /* [T][n] */, const float* Qd /* [12][n] */, const float* Rd /* [15][n] */, long n, long T,
                  float* Qsum /* [12][n] */, float* Rsum /* [15][n] */, int* nq /* [n] */, int* nr /* [15][n] */,
                  int* status /* [T][n] */, float* Qn /* [12][n] | NULL */, float* Rn /* [15][n] | NULL */, float* ws,
                  size_t ws_floats, void* stream);

/* ---- iterated extended Kalman smoother: Gauss-Newton on the MAP trajectory of a log (fixed-wing models) ----------
 * Nominal Xbar [T+1][13][n]: Xbar[0] is node -1 (the initial node), Xbar[k+1] is filter node k.  Prior (X0, P0); U, Z, mask, Qd, Rd as
 * in ac_ekf_filter_rec_f32; [+] / [-] the filter's chart and its inverse.  MAP cost per instance J = Jprior + Jproc + Jmeas:
 *     Jprior = 1/2 e0' P0^-1 e0, e0 = Xbar[0] [-] X0 (plain Cholesky of P0, its lower triangle is read, one triangular solve);
 *     Jproc  = 1/2 sum_k sum_j w_kj^2 / Qd_j, w_k = Xbar[k+1] [-] F(Xbar[k], U_k, dt); a row with Qd_j = 0 adds nothing and sets
 *              status bit 4 when w_kj != 0;
 *     Jmeas  = 1/2 sum_k sum_{used i} (z_ki - h_i(Xbar[k+1]))^2 / Rd_i, a row being used when its mask bit is set and z is finite.
 * ac_ieks_pass_f32: one linearised pass about Xbar.  One sensitivity launch over the T n units writes F_k, A_k into the workspace;
 *   k_ieks_filter runs the whole forward recursion in one launch, one instance per 16-lane group, the deviation d (R^12, about
 *   the nominal) and P in registers from step to step, from d = X0 [-] Xbar[0], P = P0.  Step k: Abar_k = E(F_k) A_k G(Xbar[k]) (the
 *   filter's expression and operation order), c_k = F_k [-] Xbar[k+1], d- = c_k + Abar_k d, P- = 1/2 (X + X') + diag(Qd) with
 *   X = Abar P Abar' (ac_ekf_step_f32's bits on equal operands); nu_i = z_i - h_i(Xbar[k+1]) and H AT THE NOMINAL; the fifteen
 *   scalar updates in row order with ac_ekf_step_f32's recursion and rejection rule, from d = d- (rho = nu_i - h_i d).  Records in
 *   ac_ekf_filter_rec_f32's shapes: Xs[k] = Xbar[k+1] [+] d_k, Ps[k], Xpreds[k] = Xbar[k+1] [+] d-_k, Ppreds[k], Abars[k], nu, S, nis,
 *   used, status [T][n] (ac_ekf_step_f32's bits), ll [n] summed in step order; ll, nu, S, nis, used, status may be NULL.  No reset
 *   Jacobian and no chart-change Jacobian is applied: re-basing the deviation from F_k to Xbar[k+1] is the first-order `+ c_k`, so
 *   a fixed point of the iteration is stationary for J to second order in the deviations only.  A step whose Xbar[k], Xbar[k+1],
 *   F_k, A_k, d- or P- is not finite sets status bit 2 (value 2): no row is applied at that node (used 0), and the recursion
 *   restarts there from d = 0, P = P- if all of P- is finite, else P0; Xs[k] = Xbar[k+1] bit for bit, Ps[k] = that P.
 *   ac_ekf_smooth_f32 on these records with (X0, P0) gives the smoothed trajectory; ac_ekf_em_f32 runs on them as on the filter's.
 * ac_ieks_cost_f32: J of reps n trajectories Xtraj [T+1][13][reps n] under Utraj [T][7][reps n]; the data of column c are those of
 *   instance c mod n.  A plain step launch supplies F; k_ieks_cost_nodes runs over (blocks of columns) x (chunks of 32 consecutive
 *   nodes), per-node terms float32, float64 sums in node order; k_ieks_cost_reduce sums the chunks in chunk order, adds Jprior and
 *   rounds to float32 once.  J [reps n]; Jprior, Jproc, Jmeas [reps n] or NULL; status [reps n]: bit 1 (value 1) P0 has no Cholesky
 *   factor, bit 2 (value 2) a node, an F or J is not finite, bit 3 (value 4) a defect in a row with Qd_j = 0.
 * ac_ieks_candidates_f32: Xc [T+1][13][C n], column c n + i = Xbar [+] ladder[c] (X^s [-] Xbar) per node (X^s: Xs0 for node -1, Xs [T][13][n]
 *   for the others), and Uc [T][7][C n], U replicated.  ladder: C host floats, 1 <= C <= 8.
 * ac_ieks_accept_f32: per instance the first c with Jc[c n + i] < Jcur[i] and status bit 2 of stc[c n + i] clear: its columns of Xc
 *   are copied into Xbar, alpha[i] = ladder[c], Jout[i] = Jc[c n + i], status[i] |= stc[c n + i]; none: Xbar is kept, alpha[i] = 0,
 *   Jout[i] = Jcur[i], status[i] |= 8 (no decrease).  status [n] is read and written.  Jout must not overlap Jcur.
 * ac_ieks_solve_f32: `iters` Gauss-Newton iterations as a host loop of the calls above from the caller's Xbar, which is updated in
 *   place: cost[0] = J(Xbar) and status = its bits; per iteration pass, ac_ekf_smooth_f32, candidates, one step launch and one cost
 *   over the C n candidates, accept -> alpha[it], cost[it+1]; then one more pass and smoother at the final Xbar.  Outputs: the final
 *   smoothed Xs [T][13][n], Ps, Xs0, Ps0; that last pass's records Xf, Pf, ll, nu, S, nis, used, fstatus, Xpreds, Ppreds, Abars;
 *   cost [iters+1][n], alpha [iters][n], status [n].  Every output is bit-equal to issuing the single calls in that order.  An
 *   instance without a decrease stays where it is: the same nominal gives the same pass, candidates and decision again.
 * No atomics, every sum in a fixed order: an instance's bits depend neither on n, on reps nor on its place in the batch.
 * ws / ws_floats: caller-owned device scratch of at least ac_ieks_workspace_floats(h, n, T, candidates) floats (the pass ignores
 * `candidates`; the cost needs candidates >= reps), else AC_ERR_WORKSPACE.  AC_ERR_UNSUPPORTED for the quadrotor; AC_ERR_BAD_ARG
 * for n < 0, T < 0, reps < 1, iters < 0, a ladder that is not 1 .. 8 finite values in (0, 1], a NULL required pointer, or dt not
 * finite and > 0; n == 0 or T == 0 is AC_OK and launches nothing.  Asynchronous, no allocation, no synchronisation,
 * hipGraph-capturable. */
int ac_ieks_workspace_floats(const ac_handle* h, long n, long T, int candidates, size_t* floats);
int ac_ieks_pass_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0 /* [13][n] */, const float* P0 /* [12][12][n] */,
                     const float* Xbar /* [T+1][13][n] */, const float* U /* [T][7][n] */, float dt, const float* Z /* [T][15][n] */,
                     const int* mask /* [T][n] | NULL */, const float* Qd, const float* Rd, long n, long T, float* Xs, float* Ps,
                     float* ll, float* nu, float* S, float* nis, int* used, int* status, float* Xpreds, float* Ppreds, float* Abars,
                     float* ws, size_t ws_floats, void* stream);
int ac_ieks_cost_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, const float* Xtraj /* [T+1][13][reps n] */,
                     const float* Utraj /* [T][7][reps n] */, float dt, const float* Z, const int* mask, const float* Qd,
                     const float* Rd, long n, long reps, long T, float* J /* [reps n] */, float* Jprior, float* Jproc, float* Jmeas,
                     int* status /* [reps n] */, float* ws, size_t ws_floats, void* stream);
int ac_ieks_candidates_f32(ac_handle* h, const float* Xbar, const float* Xs0 /* [13][n] */, const float* Xs /* [T][13][n] */,
                           const float* U, const float* ladder /* host, [candidates] */, int candidates, long n, long T,
                           float* Xc /* [T+1][13][C n] */, float* Uc /* [T][7][C n] */, void* stream);
int ac_ieks_accept_f32(ac_handle* h, const float* Jcur /* [n] */, const float* Jc /* [C n] */, const int* stc /* [C n] */,
                       const float* Xc, const float* ladder, int candidates, long n, long T, float* Xbar, float* alpha /* [n] */,
                       float* Jout /* [n] */, int* status /* [n], in and out */, void* stream);
int ac_ieks_solve_f32(ac_handle* h, const ac_ekf_opts* o, const float* X0, const float* P0, float* Xbar /* in and out */,
                      const float* U, float dt, const float* Z, const int* mask, const float* Qd, const float* Rd, long n, long T,
                      int iters, const float* ladder, int candidates, float* Xs, float* Ps, float* Xs0, float* Ps0, float* Xf,
                      float* Pf, float* ll, float* nu, float* S, float* nis, int* used, int* fstatus, float* Xpreds, float* Ppreds,
                      float* Abars, float* cost /* [iters+1][n] */, float* alpha /* [iters][n] */, int* status /* [n] */, float* ws,
                      size_t ws_floats, void* stream);

/* ---- flight modes: eigenvalues of the trim linearisation ---------------------------------------------------------
 * ac_eig_f32 (any handle): the eigenvalues of n real m x m matrices M [m][m][n], 1 <= m <= 13, float32 in and out with float64
 * arithmetic between (the eigenvalues carry the rounding of the output, 6e-8, not the matrix's conditioning), one instance per
 * lane (k_eig): balancing as LAPACK gebal does it (the permutation search that isolates every row or column whose off-diagonal
 * part is exactly zero, then scaling by powers of two), Householder reduction to Hessenberg form, Francis double-shift QR
 * (EISPACK hqr: deflation at 2^-52, exceptional shifts at the 10th and 20th iteration of an eigenvalue, at most max_iters
 * iterations per eigenvalue, 0: 30).  wr, wi [m][n] in the CANONICAL ORDER: descending wr^2 + wi^2, then descending imaginary
 * part (the + member of a pair first), then descending real part; a conjugate pair has the same real part bit for bit and
 * imaginary parts +z, -z.  status [n]: 0 all m eigenvalues found; 1 the cap was reached: the instance's outputs are NaN; 3 a
 * non-finite entry: outputs NaN, no iteration.  iters [n] or NULL: QR iterations used.  No workspace.
 * ac_modes_f32 (fixed-wing models), per instance at (X, U), which need not be a trim:
 *   1. the handle's own ac_step_sens_f32 launch writes x+ = F(x, u, dt), A, B into the workspace (every model and engine);
 *   2. k_lqr_project: A_xi, B_xi in the steady-flight chart, bit for bit what ac_lqr_f32 exports (Axi, Bxi: optional outputs);
 *   3. k_modes_eig: a copy of A_xi with the entries [rows 3-7, 9-11][columns 0, 1, 2, 8] set to exactly 0 (they are 0 by the
 *      translation and yaw invariance of the dynamics; the projection leaves float32 noise there), minus B_xi K when K
 *      [7][12][n] is given (u = u_b - K xi), restricted to the rows and columns of `coords` (m of them, 8 .. 12), its
 *      eigenvalues as above, and s = log(lambda) / dt as sigma = log1p((wr - 1)(wr + 1) + wi^2) / (2 dt) [1/s] and
 *      omega = atan2(wi, wr) / dt [rad/s].  wr, wi, sigma, omega [12][n]: rows >= m are 0.
 * No instance affects another, and an instance's bits depend neither on n nor on its place in the batch.
 * ws / ws_floats: caller-owned device scratch of at least ac_modes_workspace_floats(h, n) floats, else AC_ERR_WORKSPACE; after
 * the call it holds x+ [13][n], A [13][13][n], B [13][7][n], A_xi [12][12][n], B_xi [12][7][n], each on a 256-byte boundary, in
 * this order (A_xi, B_xi only when the outputs Axi, Bxi are NULL).
 * AC_ERR_BAD_ARG for m outside 1 .. 13, max_iters < 0, n < 0, a NULL required pointer, a `coords` that lacks one of the bits
 * 3-7, 9-11 or sets a bit >= 12, a dt that is not finite and > 0, or an output that overlaps an input; AC_ERR_UNSUPPORTED from
 * ac_modes_f32 for the quadrotor; n == 0 is AC_OK.  Asynchronous, no allocation, no synchronisation, hipGraph-capturable. */
int ac_eig_f32(ac_handle* h, const float* M /* [m][m][n] */, int m, int max_iters /* 0: 30 */, long n, float* wr, float* wi /* [m][n] */,
               int* status /* [n] */, int* iters /* [n] | NULL */, void* stream);
typedef struct ac_modes_opts {
    unsigned coords; /* bit i: chart coordinate i is kept; bits 3-7 and 9-11 are required; 0 = the eight flight coordinates (0xEF8) */
    int max_iters;   /* 0: 30 */
} ac_modes_opts;
int ac_modes_workspace_floats(const ac_handle* h, long n, size_t* floats);
int ac_modes_f32(ac_handle* h, const ac_modes_opts* o, const float* X /* [13][n] */, const float* U /* [7][n] */, float dt,
                 const float* K /* [7][12][n] | NULL: open loop */, long n, float* Axi /* [12][12][n] | NULL */,
                 float* Bxi /* [12][7][n] | NULL */, float* wr, float* wi, float* sigma, float* omega /* each [12][n] */,
                 int* status /* [n] */, int* iters /* [n] | NULL */, float* ws, size_t ws_floats, void* stream);

/* ---- sampling-based MPC: MPPI (every model kind) ---------------------------------------------------------------
 * One MPPI iteration draws K perturbed control sequences per instance (ac_mppi_sample_f32), rolls them out and costs them with
 * the calls above (candidate k of instance b is column o = k*B + b, the layout ac_rollout_policy_f32 writes), and blends them by
 * exp(-cost / lambda) (ac_mppi_update_f32).  Neither call looks at the force model.
 * Noise: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) with
 *     key = (seed & 0xffffffff, seed >> 32),  counter = (k, g, t, 2*it + j),  g = instance_offset + b,  t the node, j in {0, 1};
 * each word pair (xa, xb) gives two normals: u1 = ((xa >> 8) + 1) 2^-24, u2 = (xb >> 8) 2^-24, r = sqrt(-2 ln u1),
 * na = r cos(2 pi u2), nb = r sin(2 pi u2).  Call j = 0 feeds control rows 0-3 ((x0, x1) -> rows 0, 1; (x2, x3) -> rows 2, 3),
 * call j = 1 rows 4, 5, 6 (its fourth normal is dropped).  The draw of (seed, it, k, g, t, row) does not depend on B, K, H or on
 * how a batch is sharded.
 * it_dev: the iteration counter `it`, one unsigned int in DEVICE memory (NULL: it = 0).  The sampler reads it, the update
 * increments it as its last action — a captured sample -> ... -> update sequence draws fresh noise at every replay.
 * ac_mppi_sample_f32:  Uc[t][r][o] = min(max(Unom[t][r][b] + sigma[r] n, u_min[r]), u_max[r]); rows with sigma[r] == 0 get the
 *   clipped nominal without a draw; keep_nominal: column k = 0 is the clipped nominal in every row.  X0 [13][B] given: X0c [13][K*B]
 *   is its K-fold tiling, written by the same launch (X0 and X0c both or neither).
 * ac_mppi_update_f32:  per instance b, F = {k : J[k*B + b] finite}, Jmin = min over F, w_k = exp(-(J_k - Jmin) / lambda) on F (else 0),
 *   eta = sum w_k:  Unew[t][r][b] = clip(sum_k w_k Uc[t][r][k*B + b] / eta).  stats [4][B]: Jmin, the effective sample size
 *   eta^2 / sum w_k^2, |F|, the index of the cheapest sample (the lowest k on ties).  F empty: Unew = Unom bit for bit and
 *   stats = (+inf, 0, 0, -1).  Non-finite costs never win (as in ac_ilqr_accept_f32).  No atomics, every sum in a fixed order: the
 *   same inputs give the same bits.  Unew may be Unom itself (exact aliasing only).  ws: caller-owned device scratch of at least
 *   ac_mppi_workspace_floats floats (the normalised weights), else AC_ERR_WORKSPACE.
 * AC_ERR_BAD_ARG: K, B or H < 1, K*B > 2^31 - 1, lambda not finite or <= 0, a negative or non-finite sigma, u_min > u_max, a NULL
 * required pointer, X0 / X0c given one without the other.  Like every compute call: asynchronous on `stream`, no allocation, no
 * synchronisation, hipGraph-capturable. */
typedef struct ac_mppi_opts {
    float sigma[7];               /* std of the control noise per row (units of the row); 0 = row not sampled */
    float u_min[7], u_max[7];     /* control box */
    float lambda;                 /* temperature, > 0 */
    unsigned long long seed;
    unsigned int instance_offset; /* global index of local instance 0 (sharded batches) */
    int keep_nominal;             /* 1: sample k = 0 is the unperturbed nominal */
} ac_mppi_opts;
int ac_mppi_workspace_floats(const ac_handle* h, int K, long B, long H, size_t* floats);
int ac_mppi_sample_f32(ac_handle* h, const ac_mppi_opts* o, const unsigned int* it_dev,
                       const float* Unom /* [H][7][B] */, const float* X0 /* [13][B] or NULL */,
                       int K, long B, long H, float* Uc /* [H][7][K*B] */,
                       float* X0c /* [13][K*B] or NULL */, void* stream);
int ac_mppi_update_f32(ac_handle* h, const ac_mppi_opts* o, unsigned int* it_dev,
                       const float* J /* [K*B] */, const float* Uc, const float* Unom,
                       int K, long B, long H, float* Unew /* [H][7][B] */, float* stats /* [4][B] */,
                       float* ws, size_t ws_floats, void* stream);

/* Diagnostics */
const char* ac_last_error(void);    /* thread-local text of the last failing HIP call */
const char* ac_version(void);
int ac_device_arch(char* buf, size_t len);  /* gcnArchName of the current device */
/* Device pointer and size (floats) of the handle's second-order workspace (tests poison it with NaNs to prove that every
 * element a second-order call reads was written by that call). */
int ac_hess_workspace(const ac_handle* h, float** ptr, size_t* floats);
/* Hidden layers of the width-128 matrix-core sensitivity kernels (k_nn_step_sens<8>, k_nn_step_sens_pair<8>):
 *   AC_HIDDEN_F16   two-plane f16 MFMA, three products per fp32 product — for nets that pass the range gate of ac_set_mlp
 *                   (every operand of the hidden layers provably under 2^15, tangents not uniformly under 2^-14)
 *   AC_HIDDEN_BF16  three-plane bf16 MFMA, six products: any finite net; the fall-back of the gate
 *   AC_HIDDEN_AUTO  f16 where the gate passes, else bf16 (the default)
 * AC_HIDDEN_F16 on a net the gate rejects is AC_ERR_UNSUPPORTED — from this call if the net is already set, else from the
 * compute calls — never a silent fall-back.  Other kernels and other nets are not affected by the setting.
 * ac_hidden_route_of: the route the handle's net takes now (AC_HIDDEN_AUTO: it has no such kernels) and the gate's verdict
 * (0 passes; 1 a weight >= 2^15, 2 tangent bound >= 2^15, 3 tangents under 2^-14, 4 non-finite; -1 no such kernels). */
typedef enum ac_hidden_route { AC_HIDDEN_AUTO = 0, AC_HIDDEN_BF16 = 1, AC_HIDDEN_F16 = 2 } ac_hidden_route;
int ac_set_hidden_route(ac_handle* h, int route);
int ac_hidden_route_of(const ac_handle* h, int* route, int* gate);
/* Name + launch geometry of the kernel the last call on this handle dispatched (for profiling). */
int ac_last_launch(const ac_handle* h, char* name, size_t len, int* grid, int* block, int* lds_bytes);
/* Test aid (csrc/f16_split_check.hip): the multiply form and the fused form of the f16 activation split over every finite
 * fp32 pattern with |x| < 2^15.  out[0] / out[1]: patterns whose residual plane differs in the low / high half of the pair,
 * out[2]: patterns visited (2 * 0x47000000), out[3]: one differing pattern + 1, or 0.  Allocates and synchronises. */
int ac_f16_split_check(unsigned long long out[4]);

#ifdef __cplusplus
}
#endif
#endif
