"""ctypes binding of libaircraft_hip.so (include/aircraft_hip.h).

There is NO CPU fallback: if the shared library is missing or no gfx950 device is visible, every
compute call raises.  (`tests -m "not gpu"` only check that the library loads and exports the ABI.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# AIRCRAFT_HIP_LIB selects another build flavor of the same ABI (the diagnostic libaircraft_hip_diag.so)
LIB_PATH = os.environ.get("AIRCRAFT_HIP_LIB") or os.path.join(_HERE, "libaircraft_hip.so")

AC_OK = 0
STATUS_NAMES = {0: "AC_OK", -1: "AC_ERR_BAD_ARG", -2: "AC_ERR_HIP", -3: "AC_ERR_UNSUPPORTED",
                -4: "AC_ERR_NO_MODEL", -5: "AC_ERR_NO_DEVICE", -6: "AC_ERR_WORKSPACE"}
MODEL_KINDS = {"default": 0, "linear": 1, "nn": 2, "poly": 3, "quad": 4}
VJP_ROUTES = {"auto": 0, "fused": 1, "composed": 2}   # ac_vjp_route
HIDDEN_ROUTES = {"auto": 0, "bf16": 1, "f16": 2}      # ac_hidden_route
VJP_STEP, VJP_ROLLOUT, VJP_DERIVATIVE = 0, 1, 2       # ac_vjp_which
WGRAD_SEEDS, WGRAD_STEP, WGRAD_ROLLOUT = 0, 1, 2      # ac_wgrad_which
CGRAD_STEP, CGRAD_ROLLOUT = 0, 1                      # ac_cgrad_which
AIRFRAME_GRAD_FLOATS = 22                             # AC_AIRFRAME_GRAD_FLOATS: mass, inertia[9], inertia_inv[9], com[3]
TRIM_STATUS = {0: "converged", 1: "max_iter", 2: "bound", 3: "non_finite"}  # ac_trim_f32 status per instance
LQR_STATUS = {0: "converged", 1: "max_iter", 2: "breakdown", 3: "non_finite"}  # ac_lqr_f32 status per instance
EKF_ROWS = 15                                         # ac_ekf_*: GPS p, GPS v, gyro, air data, magnetometer (3 rows each)
EKF_REJECTED, EKF_NONFINITE = 1, 2                    # ac_ekf_step_f32 status bits per instance
LQG_ESTIMATORS = {"ekf": 0, "ukf": 1}                 # ac_lqg_opts.estimator (AC_EST_*)
LQG_FEEDBACK = {"estimate": 0, "truth": 1}            # ac_lqg_opts.feedback (AC_FB_*)
LQG_GROUPS = 5                                        # ac_sense_opts: GPS p, GPS v, gyro, air data, magnetometer
RTS_NOT_PD, RTS_NONFINITE = 1, 2                      # ac_ekf_smooth_f32 status bits per link and instance
EM_NOT_PD, EM_NONFINITE = 1, 2                        # ac_ekf_em_f32 status values per node and instance
EM_CHUNK = 32                                         # ac_ekf_em_f32: nodes per float64 partial sum (kEmChunk)
IEKS_P0_NOT_PD, IEKS_NONFINITE, IEKS_QZERO_DEFECT, IEKS_NO_DECREASE = 1, 2, 4, 8  # ac_ieks_cost_f32 / ac_ieks_solve_f32 status bits
IEKS_CHUNK = 32                                       # ac_ieks_cost_f32: nodes per float64 partial sum (kIeksChunk)
IEKS_MAX_CANDIDATES = 8                               # longest ladder of ac_ieks_*
EIG_STATUS = {0: "converged", 1: "max_iter", 3: "non_finite"}  # ac_eig_f32 / ac_modes_f32 status per instance
EIG_MAX_M = 13                                        # ac_eig_f32: 1 <= m <= 13
MODES_FLIGHT = 0xEF8                                  # ac_modes_opts.coords: chart coordinates 3-7 and 9-11
NUM_STATES = 13
NUM_CONTROLS = 7
AERO_ROWS = 22
MAX_LAYERS = 8
MAX_WIDTH = 128


class AcParams(C.Structure):
    """struct ac_params (include/aircraft_hip.h)."""
    _fields_ = [
        ("mass", C.c_float), ("S", C.c_float), ("b", C.c_float), ("c", C.c_float),
        ("inertia", C.c_float * 9),
        ("inertia_inv", C.c_float * 9),
        ("com", C.c_float * 3),
        ("rudder_moment_arm", C.c_float),
        ("epsilon", C.c_float),
        ("gravity", C.c_float * 3),
        ("substeps", C.c_int), ("normalise", C.c_int), ("stall_scaling", C.c_int), ("model_kind", C.c_int),
    ]


class IlqrCost(C.Structure):
    """struct ac_ilqr_cost (include/aircraft_hip.h)."""
    _fields_ = [("q", C.c_float * 13), ("qf", C.c_float * 13), ("r", C.c_float * 7), ("x_ref", C.c_float * 13),
                ("x_goal", C.c_float * 13), ("u_min", C.c_float * 7), ("u_max", C.c_float * 7), ("reg", C.c_float),
                ("u_lin", C.c_float * 7), ("dt_row", C.c_int)]


class GoalLoss(C.Structure):
    """struct ac_goal_loss (include/aircraft_hip.h); defaults are Controller.loss, main/control/control.py:44-68."""
    _fields_ = [("w_goal", C.c_float), ("w_rate", C.c_float), ("eps_rate", C.c_float), ("w_height", C.c_float),
                ("w_speed", C.c_float), ("w_vx", C.c_float), ("w_vyz", C.c_float), ("vx_max", C.c_float), ("w_al", C.c_float),
                ("time_row", C.c_int)]


class TrimOpts(C.Structure):
    """struct ac_trim_opts (include/aircraft_hip.h)."""
    _fields_ = [("lateral", C.c_int), ("tol_v", C.c_float), ("tol_w", C.c_float), ("lo", C.c_float * 6), ("hi", C.c_float * 6)]


class LqrOpts(C.Structure):
    """struct ac_lqr_opts (include/aircraft_hip.h)."""
    _fields_ = [("q", C.c_float * 12), ("r", C.c_float * 7), ("tol", C.c_float)]


class ModesOpts(C.Structure):
    """struct ac_modes_opts (include/aircraft_hip.h)."""
    _fields_ = [("coords", C.c_uint), ("max_iters", C.c_int)]


class EkfOpts(C.Structure):
    """struct ac_ekf_opts (include/aircraft_hip.h)."""
    _fields_ = [("mag_ned", C.c_float * 3), ("predict", C.c_int)]


class UkfOpts(C.Structure):
    """struct ac_ukf_opts (include/aircraft_hip.h)."""
    _fields_ = [("mag_ned", C.c_float * 3), ("predict", C.c_int), ("kappa", C.c_float)]


class SenseOpts(C.Structure):
    """struct ac_sense_opts (include/aircraft_hip.h)."""
    _fields_ = [("mag_ned", C.c_float * 3), ("seed_lo", C.c_uint), ("seed_hi", C.c_uint), ("instance_offset", C.c_long),
                ("period", C.c_int * 5), ("phase", C.c_int * 5), ("dropout", C.c_float * 5)]


class LqgOpts(C.Structure):
    """struct ac_lqg_opts (include/aircraft_hip.h)."""
    _fields_ = [("estimator", C.c_int), ("feedback", C.c_int), ("kappa", C.c_float), ("step0", C.c_int)]


class EkfEmOpts(C.Structure):
    """struct ac_ekf_em_opts (include/aircraft_hip.h)."""
    _fields_ = [("mag_ned", C.c_float * 3), ("floor_rel", C.c_float)]


class MppiOpts(C.Structure):
    """struct ac_mppi_opts (include/aircraft_hip.h)."""
    _fields_ = [("sigma", C.c_float * 7), ("u_min", C.c_float * 7), ("u_max", C.c_float * 7), ("lambda_", C.c_float),
                ("seed", C.c_ulonglong), ("instance_offset", C.c_uint), ("keep_nominal", C.c_int)]


class EnvelopePenalty(C.Structure):
    """struct ac_envelope_penalty (include/aircraft_hip.h)."""
    _fields_ = [("lo", C.c_float * 4), ("hi", C.c_float * 4), ("weight", C.c_float)]


class MhttWeights(C.Structure):
    """struct ac_mhtt_weights (include/aircraft_hip.h); defaults are moving_horizon.py:47-55."""
    _fields_ = [("w_tracking", C.c_float), ("w_progress", C.c_float), ("w_progress_rate", C.c_float),
                ("w_backward", C.c_float), ("w_terminal_align", C.c_float), ("w_low_velocity", C.c_float),
                ("w_control", C.c_float)]


# every symbol include/aircraft_hip.h declares, with its prototype
_FP = C.POINTER(C.c_float)
_VP = C.c_void_p
PROTOTYPES = {
    "ac_create": (C.c_int, [C.POINTER(AcParams), C.POINTER(_VP)]),
    "ac_destroy": (C.c_int, [_VP]),
    "ac_set_params": (C.c_int, [_VP, C.POINTER(AcParams)]),
    "ac_set_linear": (C.c_int, [_VP, _FP]),
    "ac_set_poly": (C.c_int, [_VP, _FP, _FP]),
    "ac_set_mlp": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_FP), C.POINTER(_FP),
                             _FP, _FP, _FP, _FP, C.c_int]),
    "ac_state_derivative_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_step_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP]),
    "ac_rollout_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP]),
    "ac_step_sens_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP]),
    "ac_shoot_step_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_shoot_sens_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP]),
    "ac_state_derivative_sens_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP]),
    "ac_shoot_derivative_sens_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP]),
    "ac_shoot_derivative_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_shoot_defect_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_shoot_implicit_defect_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_shoot_implicit_rows_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP]),
    "ac_envelope_f32": (C.c_int, [_VP, _VP, C.c_long, _VP, _VP, _VP]),
    "ac_shoot_envelope_f32": (C.c_int, [_VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_envelope_cost_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_envelope_model_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_envelope_al_cost_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_envelope_al_model_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_envelope_al_update_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_quat_rows_f32": (C.c_int, [_VP, C.c_int, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP]),
    "ac_step_hess_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_reserve_hess_workspace": (C.c_int, [_VP, C.c_long]),
    "ac_shoot_hess_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_aero_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_traj_cost_f32": (C.c_int, [_VP, _VP, C.c_long, C.c_long, _FP, C.c_float, C.c_float, _VP, _VP]),
    "ac_best_records_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_long, C.c_long, C.c_int, _VP, _VP]),
    "ac_merge_records_f32": (C.c_int, [_VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_ilqr_accept_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_int, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP]),
    "ac_ilqr_backward_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP]),
    "ac_ilqr_cost_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_ilqr_backward_node_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP,
                                            _VP]),
    "ac_ilqr_costate_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_ilqr_backward_newton_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                              _VP, _VP, _VP]),
    "ac_ilqr_cost_node_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_long, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_goal_cost_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_long, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_goal_model_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ac_goal_multiplier_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_ilqr_backward_goal_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP,
                                            _VP, _VP]),
    "ac_ilqr_backward_rate_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                            _VP, _VP, _VP, _VP]),
    "ac_ilqr_backward_box_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP,
                                           _VP, _VP, _VP, _VP]),
    "ac_ilqr_backward_rate_box_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long,
                                                _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ac_ilqr_backward_shoot_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP,
                                             _VP, _VP, _VP, C.c_int, _VP, _VP, _VP]),
    "ac_shoot_direction_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP,
                                         _VP]),
    "ac_shoot_merit_weight_f32": (C.c_int, [_VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP]),
    "ac_shoot_candidates_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _FP, C.c_int, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_shoot_merit_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_rollout_policy_rate_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _FP, C.c_int, C.c_float, C.c_long, C.c_long,
                                             _VP, _VP, _VP]),
    "ac_goal_model_rate_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ac_ilqr_rate_model_f32": (C.c_int, [_VP, _FP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_ilqr_rate_cost_f32": (C.c_int, [_VP, _FP, _VP, C.c_long, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_set_track": (C.c_int, [_VP, C.c_int, _FP, C.c_float]),
    "ac_track_eval_f32": (C.c_int, [_VP, _VP, C.c_long, _VP, _VP, _VP]),
    "ac_track_progress_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_float, C.c_long, C.c_long, C.c_int, _VP, _VP, _VP, _VP,
                                        _VP, _VP, _VP]),
    "ac_mhtt_loss_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_rollout_policy_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _FP, C.c_int, C.c_float, C.c_long, C.c_long,
                                        _VP, _VP, _VP]),
    "ac_set_vjp_route": (C.c_int, [_VP, C.c_int]),
    "ac_set_hidden_route": (C.c_int, [_VP, C.c_int]),
    "ac_hidden_route_of": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ac_vjp_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_step_vjp_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_rollout_vjp_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_state_derivative_vjp_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_mlp_folded_shape": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ac_mlp_grad_floats": (C.c_int, [_VP, C.POINTER(C.c_size_t)]),
    "ac_wgrad_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_step_wgrad_seeds_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_step_wgrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_rollout_wgrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_coef_grad_floats": (C.c_int, [_VP, C.POINTER(C.c_size_t)]),
    "ac_cgrad_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_set_cgrad_grid": (C.c_int, [_VP, C.c_int]),
    "ac_step_cgrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_rollout_cgrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t,
                                       _VP]),
    "ac_agrad_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_step_agrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_rollout_agrad_f32": (C.c_int, [_VP, _VP, _VP, C.c_float, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t,
                                       _VP]),
    "ac_trim_workspace_floats": (C.c_int, [_VP, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_trim_f32": (C.c_int, [_VP, C.POINTER(TrimOpts), _VP, _VP, _VP, C.c_int, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t,
                              _VP]),
    "ac_lqr_workspace_floats": (C.c_int, [_VP, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_lqr_f32": (C.c_int, [_VP, C.POINTER(LqrOpts), _VP, _VP, C.c_float, C.c_int, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                             C.c_size_t, _VP]),
    "ac_lqr_gains_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP]),
    "ac_steady_error_f32": (C.c_int, [_VP, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_ekf_workspace_floats": (C.c_int, [_VP, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_ekf_measure_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, C.c_long, _VP, _VP]),
    "ac_ekf_step_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP,
                                  _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ekf_filter_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                    _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ekf_filter_rec_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                        _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ukf_workspace_floats": (C.c_int, [_VP, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_ukf_step_f32": (C.c_int, [_VP, C.POINTER(UkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP,
                                  _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ukf_filter_f32": (C.c_int, [_VP, C.POINTER(UkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                    _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ukf_filter_rec_f32": (C.c_int, [_VP, C.POINTER(UkfOpts), _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP,
                                        _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_sense_f32": (C.c_int, [_VP, C.POINTER(SenseOpts), C.c_int, _VP, _VP, _VP, C.c_long, _VP, _VP, _VP]),
    "ac_disturb_f32": (C.c_int, [_VP, C.POINTER(SenseOpts), C.c_int, _VP, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_policy_f32": (C.c_int, [_VP, C.POINTER(IlqrCost), _VP, _VP, _VP, _VP, C.c_long, _VP, _VP]),
    "ac_estimate_score_f32": (C.c_int, [_VP, _VP, _VP, _VP, C.c_long, _VP, _VP, _VP, _VP]),
    "ac_lqg_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_lqg_rollout_f32": (C.c_int, [_VP, C.POINTER(LqgOpts), C.POINTER(SenseOpts), C.POINTER(IlqrCost)] + [_VP] * 10
                           + [C.c_float, C.c_long, C.c_long] + [_VP] * 15 + [C.c_size_t, _VP]),
    "ac_ekf_smooth_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ac_ekf_em_workspace_floats": (C.c_int, [_VP, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_ekf_em_f32": (C.c_int, [_VP, C.POINTER(EkfEmOpts), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, C.c_long, C.c_long, _VP, _VP, _VP, _VP,
                                _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "ac_ieks_workspace_floats": (C.c_int, [_VP, C.c_long, C.c_long, C.c_int, C.POINTER(C.c_size_t)]),
    "ac_ieks_pass_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long]
                         + [_VP] * 12 + [C.c_size_t, _VP]),
    "ac_ieks_cost_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long,
                                   C.c_long] + [_VP] * 6 + [C.c_size_t, _VP]),
    "ac_ieks_candidates_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float), C.c_int, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_ieks_accept_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_float), C.c_int, C.c_long, C.c_long, _VP, _VP, _VP, _VP,
                                     _VP]),
    "ac_ieks_solve_f32": (C.c_int, [_VP, C.POINTER(EkfOpts), _VP, _VP, _VP, _VP, C.c_float, _VP, _VP, _VP, _VP, C.c_long, C.c_long,
                                    C.c_int, C.POINTER(C.c_float), C.c_int] + [_VP] * 19 + [C.c_size_t, _VP]),
    "ac_eig_f32": (C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_long, _VP, _VP, _VP, _VP, _VP]),
    "ac_modes_workspace_floats": (C.c_int, [_VP, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_modes_f32": (C.c_int, [_VP, C.POINTER(ModesOpts), _VP, _VP, C.c_float, _VP, C.c_long, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                               _VP, C.c_size_t, _VP]),
    "ac_mppi_workspace_floats": (C.c_int, [_VP, C.c_int, C.c_long, C.c_long, C.POINTER(C.c_size_t)]),
    "ac_mppi_sample_f32": (C.c_int, [_VP, C.POINTER(MppiOpts), _VP, _VP, _VP, C.c_int, C.c_long, C.c_long, _VP, _VP, _VP]),
    "ac_mppi_update_f32": (C.c_int, [_VP, C.POINTER(MppiOpts), _VP, _VP, _VP, _VP, C.c_int, C.c_long, C.c_long, _VP, _VP, _VP,
                                     C.c_size_t, _VP]),
    "ac_last_error": (C.c_char_p, []),
    "ac_version": (C.c_char_p, []),
    "ac_device_arch": (C.c_int, [C.c_char_p, C.c_size_t]),
    "ac_hess_workspace": (C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_size_t)]),
    "ac_last_launch": (C.c_int, [_VP, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                 C.POINTER(C.c_int)]),
    "ac_f16_split_check": (C.c_int, [C.POINTER(C.c_ulonglong)]),
}

_lib = None


class AircraftHipError(RuntimeError):
    """Raised for any non-zero ac_status — the reference's failures surface as RuntimeError too
    (control/base.py:471-474)."""


def load():
    """Load libaircraft_hip.so; raise (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AircraftHipError(
                f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). aircraft_amd has no CPU fallback."
            )
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != AC_OK:
        msg = load().ac_last_error().decode()  # cleared at the top of every entry point: never a stale text
        raise AircraftHipError(f"{what or 'aircraft_hip call'} failed: {STATUS_NAMES.get(rc, rc)} {msg}".strip())
