"""Batched iLQR / Gauss-Newton sweep on top of the multiple-shooting linearisation.

The reference formulates its MPC as an NLP and hands it to IPOPT, one instance at a time
(src/aircraft/control/base.py:455-477).  This module is the build-side solver that turns the hot-path kernels
(rollout, step sensitivities) into B simultaneous MPC solves — random restarts / independent instances — playing the
`loss` and control-limit roles of the reference's controllers (control/base.py:323-337, control/aircraft.py:29-41,
main/control/control.py:35-70: goal term on the final position, actuation penalty, surface limits).

One iteration = linearise (ac_shoot_sens_f32) -> backward Riccati pass (ac_ilqr_backward_f32) -> closed-loop rollouts for
every line-search step alpha in ONE launch (ac_rollout_policy_f32) -> cost (ac_ilqr_cost_f32) -> per-instance argmin.
Everything stays on the device; torch supplies the buffers only (the acceptance is a HIP kernel too: ac_ilqr_accept_f32).

A control-RATE cost (`ILQR(rate_weight=)`, `GoalAcquisition(rate="exact")`) is modelled exactly: the Riccati pass carries the
previous control as seven more states (ac_ilqr_backward_rate_f32, csrc/ac_ilqr_rate.hpp) and the closed loop feeds the control
it applied at the previous node back through the gains Kp (ac_rollout_policy_rate_f32).

The control box enters the backward pass with `ILQR(box="qp")` (control-limited DDP: a 7-variable QP per node,
ac_ilqr_backward_box_f32 / ac_ilqr_backward_rate_box_f32, csrc/ac_boxqp.hpp); the default `box="clip"` leaves it to the clip of the
closed-loop rollout.

`ILQR(shooting="multiple")` is Gauss-Newton multiple shooting (Giftthaler et al. 2018): the states of the iterate are decision
variables, the gaps d_k = F(x_k, u_k) - x_{k+1} enter the Riccati pass (ac_ilqr_backward_shoot_f32), one forward sweep gives the
direction (dX, dU) and the multipliers of the defect rows (ac_shoot_direction_f32), every line-search candidate X + alpha dX,
clip(U + alpha dU) is evaluated as independent nodes in ONE step launch (ac_shoot_defect_f32), and the acceptance runs on the exact
L1 merit  J + mu_b sum |defect|  (ac_shoot_merit_f32).  The default `shooting="single"` is the sweep described above, unchanged.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

from .. import _lib
from .base import MultipleShooting


def _torch():
    import torch

    return torch


@dataclass
class QuadraticCost:
    """J = sum_k 1/2 (x_k - x_ref)' diag(q) (x_k - x_ref) + 1/2 u_k' diag(r) u_k + 1/2 (x_N - x_goal)' diag(qf) (x_N - x_goal)."""
    q: Sequence[float] = field(default_factory=lambda: [0.0] * 13)
    qf: Sequence[float] = field(default_factory=lambda: [0.0] * 13)
    r: Sequence[float] = field(default_factory=lambda: [1e-2] * 7)
    x_ref: Sequence[float] = field(default_factory=lambda: [0.0] * 13)
    x_goal: Sequence[float] = field(default_factory=lambda: [0.0] * 13)
    # control box: aileron/elevator/rudder +-5 deg (control/aircraft.py:26), thrust disabled, flaps in [0, 1]
    u_min: Sequence[float] = field(default_factory=lambda: [-5, -5, -5, 0, 0, 0, 0])
    u_max: Sequence[float] = field(default_factory=lambda: [5, 5, 5, 0, 0, 0, 1])
    reg: float = 1e-3
    u_lin: Sequence[float] = field(default_factory=lambda: [0.0] * 7)   # linear control cost (the time term)
    dt_row: int = 0                                                      # > 0: control row carrying dt_k (ILQR(time="variable"))

    @staticmethod
    def goal(goal_xy, w_goal=1000.0, w_height=1.0, height=None, w_lateral_speed=1000.0, r=1e-2, reg=1e-3):
        """The shape of Controller.loss (main/control/control.py:35-70): reach goal (x, y) at the final node, keep the
        final height, damp final lateral/vertical speed, penalise actuation."""
        c = QuadraticCost(r=[r] * 7, reg=reg)
        qf = [0.0] * 13; xg = [0.0] * 13
        qf[0] = qf[1] = 2.0 * w_goal; xg[0], xg[1] = float(goal_xy[0]), float(goal_xy[1])
        if height is not None:
            qf[2] = 2.0 * w_height; xg[2] = float(height)
        qf[4] = qf[5] = 2.0 * w_lateral_speed
        c.qf, c.x_goal = qf, xg
        return c

    @staticmethod
    def cruise(w_lateral_speed=0.5, w_attitude=5.0, w_rate=0.2, r=0.5, reg=1.0):
        """A regulator without a goal point, for closed loops that run for minutes: hold the heading north (v_east -> 0,
        q -> identity, i.e. wings level, nose on the horizon, yaw 0), damp the body rates, penalise actuation; height and
        along-track position are free (a glider sinks)."""
        c = QuadraticCost(r=[r] * 7, reg=reg)
        q = [0.0] * 13
        q[4] = w_lateral_speed
        q[6] = q[7] = q[8] = w_attitude   # vector part of q (xyzw) -> 0
        q[10] = q[11] = q[12] = w_rate
        xr = [0.0] * 13
        xr[9] = 1.0
        c.q, c.qf, c.x_ref, c.x_goal = q, list(q), xr, list(xr)
        return c

    def struct(self) -> "_lib.IlqrCost":
        s = _lib.IlqrCost()
        for name, n in (("q", 13), ("qf", 13), ("r", 7), ("x_ref", 13), ("x_goal", 13), ("u_min", 7), ("u_max", 7), ("u_lin", 7)):
            v = [float(x) for x in getattr(self, name)]
            assert len(v) == n, name
            getattr(s, name)[:] = v
        s.reg = float(self.reg)
        s.dt_row = int(self.dt_row)
        return s


class ILQR(MultipleShooting):
    def __init__(self, *, system, dt: float = 0.01, num_nodes: int, cost: QuadraticCost, opts: Optional[dict] = None,
                 alphas: Sequence[float] = (1.0, 0.5, 0.25, 0.1, 0.03), hessian: str = "gauss-newton",
                 envelope_weight: float = 0.0, envelope_bounds=None, envelope: str = "penalty",
                 time: str = "fixed", dt_bounds=(0.005, 0.02), w_time: float = 0.0, r_time: float = 0.0, rate_weight=None,
                 box: str = "clip", shooting: str = "single", defect_weight: float = 1.0, merit_factor: float = 2.0):
        """shooting: 'single' (the iterate is a rollout; line search by closed-loop rollouts) or 'multiple' (the states are decision
        variables too: `solve(X0=)` takes a state guess, the defects x_{k+1} - F(x_k, u_k) are closed by the iteration; the line
        search runs on the merit  J + mu_b sum |defect|  with  mu_b <- max(mu_b, merit_factor max |lambda|), mu_b = defect_weight
        at the start of every solve; `last_multipliers`, `last_defect`, `merit_weight`, `defect_history`).
        box: 'clip' (the backward pass is unconstrained, the closed-loop rollout clips into [u_min, u_max]) or 'qp' (the box
        in the backward pass too: per node  min 1/2 d'Quu d + Qu'd,  u_min - U_k <= d <= u_max - U_k;  kff is its solution, the
        gains of clamped controls are zero; `last_active` / `qp_stat` report the active set and the QP's iteration counts).
        rate_weight (a scalar or 7 values, >= 0): adds the actuator-slew cost  1/2 sum_k sum_i w_i (u_k,i - u_{k-1},i)^2  —
        plus the k = 0 term against `solve(u_prev=)` — to the objective (`trajectory_cost`), modelled exactly in the backward
        pass; the time row of time='variable' is excluded.
        hessian: 'gauss-newton' (first-order dynamics in the backward pass: iLQR) or 'exact' (adds the second-order
        terms  sum_i lambda_i d2F_i/dz dz  of every node — what IPOPT gets from `nlp_hess_l`).
        envelope_weight > 0: the flight envelope of AircraftControl.state_constraint (control/aircraft.py:44-59:
        20^2 <= |v_rel|^2 <= 100^2, |beta| <= 10 deg, |alpha| <= 20 deg, z < 0) as a soft constraint — the squared violation
        of its four rows, times the weight, at every node, with its Gauss-Newton model in the backward pass (IPOPT
        enforces the rows as hard constraints; the control box stays a hard clip).  envelope_bounds: ((lo, hi),) * 4,
        default `system.ENVELOPE_BOUNDS`.
        envelope: 'penalty' (the soft form above) or 'al' — the HARD treatment: augmented-Lagrangian multipliers per node, row
        and instance (ac_envelope_al_*), updated by `update_multipliers()` between sweeps (`solve(al_every=)`); the penalty
        alone leaves a violation of about multiplier / (2 weight) at an active bound, the multipliers remove it."""
        super().__init__(system=system, dt=dt, num_nodes=num_nodes, opts=opts or {"quaternion": "integration"})
        assert 1 <= len(alphas) <= 8 and hessian in ("gauss-newton", "exact") and envelope in ("penalty", "al")
        self.envelope_mode = envelope
        # time as a decision variable per node (the reference's opts['time'] in ('progress', 'variable'),
        # control/base.py:276, 339-385; its loss adds the total time, main/control/control.py:44, 66-67): a control row the
        # force model ignores carries dt_k, boxed by dt_bounds, costed by w_time * dt_k (+ 1/2 r_time dt_k^2); the column of B
        # for it is c = dF/d(dt) from the sensitivity kernels.
        assert time in ("fixed", "variable")
        assert box in ("clip", "qp"), "box: 'clip' or 'qp'"
        self.box = box
        assert shooting in ("single", "multiple"), "shooting: 'single' or 'multiple'"
        self.shooting = shooting
        self.defect_weight, self.merit_factor = float(defect_weight), float(merit_factor)
        assert 0.0 < self.defect_weight < float("inf") and 0.0 <= self.merit_factor < float("inf"), "defect_weight > 0, merit_factor >= 0"
        if shooting == "multiple":  # (each of these is a follow-up)
            assert rate_weight is None, "shooting='multiple' does not take rate_weight yet (the rate kernels have no defect switch)"
            assert time == "fixed", "shooting='multiple' keeps the fixed step (time='variable' is not supported yet)"
            assert hessian == "gauss-newton", "shooting='multiple' is Gauss-Newton (hessian='exact' is not supported yet)"
        self.defect_history = None
        self.time_row = 0
        if time == "variable":
            assert hessian == "gauss-newton", "the exact-Hessian sweep keeps the fixed step"
            import copy

            self.time_row = 4 if getattr(system, "num_controls", 7) == 4 else 3
            cost = copy.deepcopy(cost)
            r = self.time_row
            cost.u_min, cost.u_max, cost.u_lin, cost.r = list(cost.u_min), list(cost.u_max), list(cost.u_lin), list(cost.r)
            cost.u_min[r], cost.u_max[r] = float(dt_bounds[0]), float(dt_bounds[1])
            cost.u_lin[r], cost.r[r], cost.dt_row = float(w_time), float(r_time), r
            self.cost = cost
        self.cost = cost
        self.alphas = [float(a) for a in alphas]
        self.hessian_mode = hessian
        self.envelope_weight = float(envelope_weight)
        self.envelope_bounds = envelope_bounds
        self.rate_weight = None
        if rate_weight is not None:
            w = [float(rate_weight)] * 7 if not hasattr(rate_weight, "__len__") else [float(v) for v in rate_weight]
            assert len(w) == 7 and all(0.0 <= v < float("inf") for v in w), "rate_weight: a scalar or 7 finite values >= 0"
            if self.time_row > 0:
                w[self.time_row] = 0.0
            self.rate_weight = w
        self._u_prev = None        # (7, B) control applied before the window (solve(u_prev=)), or None
        self._rate_exact = self.rate_weight is not None   # the backward pass carries u_{k-1} (GoalAcquisition(rate="exact") too)
        self._ws = None

    # ---- device workspace (allocated once per (B, H)) ------------------------------------------------
    def _workspace(self, B, dev):
        torch = _torch()
        H, na = self.num_nodes, len(self.alphas)
        key = (B, H, na, str(dev))
        if self._ws is None or self._ws["key"] != key:
            f = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
            self._ws = dict(key=key, F=f(H, 13, B), A=f(H, 13, 13, B), Bm=f(H, 13, 7, B), K=f(H, 7, 13, B), kff=f(H, 7, B),
                            dV=f(2, B), Xc=f(H + 1, 13, na * B), Uc=f(H, 7, na * B), Jc=f(na * B), J0=f(B), Ja=f(B),
                            improved=torch.empty((B,), device=dev, dtype=torch.bool))
            if self.time_row > 0:
                self._ws.update(dt=f(H, B), c=f(H, 13, B))
            if self._rate_exact:
                self._ws.update(Kp=f(H, 7, 7, B), rate_g=f(H, 7, B), rate_h=f(H, 7, B))
            if self.box == "qp":
                self._ws.update(act=torch.zeros((H, 7, B), device=dev, dtype=torch.int8),
                                stat=torch.zeros((2, B), device=dev, dtype=torch.int32))
            if self.shooting == "multiple":
                self._ws.update(Vx=f(H, 13, B), Vxx=f(H, 13, 13, B), dX=f(H + 1, 13, B), dU=f(H, 7, B), Lam=f(H, 13, B),
                                Rc=f(H, 13, na * B), phic=f(na * B), phi0=f(B), dinfc=f(na * B), dinf0=f(B),
                                mu=torch.full((B,), self.defect_weight, device=dev, dtype=torch.float32))
            if self.hessian_mode == "exact":
                self._ws.update(Lam=f(H, 13, B), Hz=f(H, 21, 21, B))
                self.system._sync()
                self.system._reserve_hess(H * B)  # host-side, once: the solve itself stays allocation-free (capturable)
            if self.envelope_weight > 0:
                # constant-cost rows as per-node arrays (the penalty gradient is added to glin every iteration)
                c = self.cost
                nq = torch.tensor([list(c.q)] * H + [list(c.qf)], device=dev, dtype=torch.float32)        # (H+1, 13)
                nx = torch.tensor([list(c.x_ref)] * H + [list(c.x_goal)], device=dev, dtype=torch.float32)
                self._ws.update(env_q=nq[:, :, None].expand(H + 1, 13, B).contiguous(),
                                env_xref=nx[:, :, None].expand(H + 1, 13, B).contiguous(), env_glin=f(H + 1, 13, B))
                if "Hz" not in self._ws:
                    self._ws["Hz"] = f(H, 21, 21, B)
                if self.envelope_mode == "al":
                    self._ws.update(lam=torch.zeros((H + 1, 8, B), device=dev, dtype=torch.float32), viol=f(B))
        return self._ws

    def _envelope_struct(self):
        b = self.envelope_bounds or self.system.ENVELOPE_BOUNDS
        big = 3.0e38
        clamp = lambda v: max(-big, min(big, float(v)))  # noqa: E731  (inf does not survive some float paths: use +-FLT_MAX)
        p = _lib.EnvelopePenalty()
        p.lo[:] = [clamp(r[0]) for r in b]
        p.hi[:] = [clamp(r[1]) for r in b]
        p.weight = self.envelope_weight
        return p

    def _lam(self):
        """The multipliers of the augmented-Lagrangian envelope (H+1, 8, B), or None for the plain penalty."""
        return self._ws.get("lam") if (self._ws is not None and self.envelope_mode == "al") else None

    def envelope_cost(self, X, cost_inout):
        """cost_inout[b] += the envelope term of every node of X (in place, on the device): the squared violation times the
        weight, or its augmented-Lagrangian form with the current multipliers."""
        lib = self.system._sync()
        H, B = X.shape[0] - 1, X.shape[2]
        p = self._envelope_struct()
        lam = self._lam()
        _lib.check(lib.ac_envelope_al_cost_f32(self.system._handle, C.byref(p), lam.data_ptr() if lam is not None else None,
                                               lam.shape[2] if lam is not None else 1, X.data_ptr(), B, H,
                                               cost_inout.data_ptr(), self.system._stream()), "ac_envelope_al_cost_f32")
        return cost_inout

    def update_multipliers(self, X):
        """First-order multiplier update of the augmented-Lagrangian envelope at the iterate X (in place).  Returns each
        instance's largest bound excess before the update (B,), relative to the row's range."""
        lib = self.system._sync()
        assert self.envelope_mode == "al" and self.envelope_weight > 0
        H, B = X.shape[0] - 1, X.shape[2]
        ws = self._workspace(B, X.device)
        p = self._envelope_struct()
        ws["viol"].zero_()
        _lib.check(lib.ac_envelope_al_update_f32(self.system._handle, C.byref(p), X.data_ptr(), B, H, ws["lam"].data_ptr(),
                                                 ws["viol"].data_ptr(), self.system._stream()), "ac_envelope_al_update_f32")
        return ws["viol"]

    def _envelope_model(self, X, glin=None, Hz=None):
        """Adds the penalty's gradient to glin (N+1, 13, B) and / or its Gauss-Newton curvature to the (x, x) block of
        Hz (N, 21, 21, B), in place."""
        lib = self.system._sync()
        H, B = X.shape[0] - 1, X.shape[2]
        p = self._envelope_struct()
        lam = self._lam()
        _lib.check(lib.ac_envelope_al_model_f32(self.system._handle, C.byref(p), lam.data_ptr() if lam is not None else None,
                                                X.data_ptr(), B, H, glin.data_ptr() if glin is not None else None,
                                                Hz.data_ptr() if Hz is not None else None, self.system._stream()),
                   "ac_envelope_al_model_f32")

    def _cstruct(self):
        return C.byref(self.cost.struct())

    def trajectory_cost(self, X, U, out=None):
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        if out is None:
            out = torch.empty((B,), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_ilqr_cost_f32(self.system._handle, self._cstruct(), X.data_ptr(), U.data_ptr(), B, H,
                                        out.data_ptr(), self.system._stream()), "ac_ilqr_cost_f32")
        if self.rate_weight is not None:  # (a candidate batch reads instance o % Bn's previous control)
            up = self._u_prev
            _lib.check(lib.ac_ilqr_rate_cost_f32(self.system._handle, self._rate_arr(), up.data_ptr() if up is not None else None,
                                                 up.shape[1] if up is not None else B, U.data_ptr(), B, H, out.data_ptr(),
                                                 self.system._stream()), "ac_ilqr_rate_cost_f32")
        return out

    def _rate_arr(self):
        return (C.c_float * 7)(*self.rate_weight)

    def rate_model(self, U, out=None):
        """The model of the quadratic rate cost for the backward pass: (rate_g, rate_h), each (N, 7, B) — gradient and
        curvature with respect to the difference u_k - u_{k-1}; row 0 is the term against `u_prev` (zeros without one)."""
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        if out is None:
            out = (torch.empty((H, 7, B), device=U.device), torch.empty((H, 7, B), device=U.device))
        up = self._u_prev
        assert up is None or tuple(up.shape) == (7, B), "u_prev: (7, B)"
        _lib.check(lib.ac_ilqr_rate_model_f32(self.system._handle, self._rate_arr(), U.data_ptr(),
                                              up.data_ptr() if up is not None else None, B, H, out[0].data_ptr(),
                                              out[1].data_ptr(), self.system._stream()), "ac_ilqr_rate_model_f32")
        return out

    def _node_cost(self, X, U):
        """Hook: per-node state-cost arrays (node_q, node_xref, node_glin), each (N+1, 13, B), or None for the constant
        quadratic cost of `self.cost` (MHTT overrides this)."""
        return None

    @staticmethod
    def _ptrs(node):
        return [C.c_void_p(t.data_ptr()) for t in node] if node is not None else [C.c_void_p(0)] * 3

    def costate(self, X, A, node=None, out=None):
        """Multipliers of the defect rows at the current iterate, (N, 13, B): Lam[N-1] = grad l_N(x_N),
        Lam[k-1] = grad l_k(x_k) + A_k' Lam[k]."""
        torch = _torch()
        lib = self.system._sync()
        H, B = A.shape[0], A.shape[3]
        if out is None:
            out = torch.empty((H, 13, B), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_ilqr_costate_f32(self.system._handle, self._cstruct(), *self._ptrs(node), X.data_ptr(),
                                           A.data_ptr(), B, H, out.data_ptr(), self.system._stream()),
                   "ac_ilqr_costate_f32")
        return out

    _goal_model = None  # GoalAcquisition sets it (see iterate)

    @property
    def last_active(self):
        """box='qp': the active set of the last backward pass, (N, 7, B) int8 — 0 free, -1 / +1 clamped at the lower / upper
        bound, 2 pinned (u_min == u_max); None before the first iteration or with box='clip'."""
        return self._ws.get("act") if self._ws is not None else None

    @property
    def qp_stat(self):
        """box='qp': (2, B) int32 of the last backward pass — the largest Newton-iteration count over the instance's nodes, and
        the number of nodes whose QP ended at an iteration cap."""
        return self._ws.get("stat") if self._ws is not None else None

    def _backward_box(self, X, U, A, Bm, out, Hz, node, uglin, rate):
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        n = 4 if rate is not None else 3
        if out is None:
            out = (torch.empty((H, 7, 13, B), device=X.device), torch.empty((H, 7, B), device=X.device),
                   torch.empty((2, B), device=X.device))
            if rate is not None:
                out += (torch.empty((H, 7, 7, B), device=X.device),)
        out = tuple(out)
        if len(out) == n:
            out += (torch.empty((H, 7, B), device=X.device, dtype=torch.int8),
                    torch.empty((2, B), device=X.device, dtype=torch.int32))
        assert len(out) == n + 2, "out: the outputs of the unboxed pass, then act (N, 7, B) int8 and stat (2, B) int32"
        act, stat = out[n], out[n + 1]
        assert act.dtype == torch.int8 and stat.dtype == torch.int32 and act.is_contiguous() and stat.is_contiguous()
        hz = C.c_void_p(Hz.data_ptr() if Hz is not None else 0)
        if rate is not None:
            K, kff, dV, Kp = out[:4]
            _lib.check(lib.ac_ilqr_backward_rate_box_f32(self.system._handle, self._cstruct(), *self._ptrs(node), hz,
                                                         rate[0].data_ptr(), rate[1].data_ptr(), X.data_ptr(), U.data_ptr(),
                                                         A.data_ptr(), Bm.data_ptr(), B, H, K.data_ptr(), Kp.data_ptr(),
                                                         kff.data_ptr(), dV.data_ptr(), act.data_ptr(), stat.data_ptr(),
                                                         self.system._stream()), "ac_ilqr_backward_rate_box_f32")
            return out
        K, kff, dV = out[:3]
        if uglin is not None:
            assert node is not None and Hz is not None
        _lib.check(lib.ac_ilqr_backward_box_f32(self.system._handle, self._cstruct(), *self._ptrs(node),
                                                C.c_void_p(uglin.data_ptr() if uglin is not None else 0), hz, X.data_ptr(),
                                                U.data_ptr(), A.data_ptr(), Bm.data_ptr(), B, H, K.data_ptr(), kff.data_ptr(),
                                                dV.data_ptr(), act.data_ptr(), stat.data_ptr(), self.system._stream()),
                   "ac_ilqr_backward_box_f32")
        return out

    # ---- multiple shooting ---------------------------------------------------------------------------------------------------
    @property
    def last_multipliers(self):
        """shooting='multiple': the multipliers of the defect rows of the last iteration's QP, (N, 13, B); None before it.
        They are those of the sweep `iterate` runs, lam_k = V_x^{k+1} + V_xx^{k+1} dx_{k+1} with the control step CLIPPED into the
        box: where no clip binds they are the multipliers of the equality-constrained QP exactly, where one binds they belong to the
        clipped direction, not to the QP's solution."""
        return self._ws.get("Lam") if self._shoot_done() else None

    @property
    def last_defect(self):
        """shooting='multiple': (B,) the largest |x_{k+1} - F(x_k, u_k)| of the iterate the last iteration STARTED from (the end
        of `solve` measures the final iterate); None before the first iteration."""
        return self._ws.get("dinf0") if self._shoot_done() else None

    @property
    def merit_weight(self):
        """shooting='multiple': (B,) the weight mu_b of the L1 defect term in the merit function.  Every `solve` starts it at
        `defect_weight` and it never decreases within one; `GoalAcquisition.solve(al_every=)` is a sequence of solves (one per
        block of sweeps between multiplier updates: the objective changes there), so it starts again with every block."""
        return self._ws.get("mu") if (self._ws is not None and self.shooting == "multiple") else None

    def _shoot_done(self):
        """an iteration of this mode has filled the workspace (the buffers are uninitialised before)"""
        return self._ws is not None and self.shooting == "multiple" and self._ws.get("shoot_done", False)

    def _backward_shoot(self, X, U, A, Bm, F, out, Hz, node, uglin, box):
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        if out is None:
            out = (torch.empty((H, 7, 13, B), device=X.device), torch.empty((H, 7, B), device=X.device),
                   torch.empty((2, B), device=X.device), torch.empty((H, 13, B), device=X.device),
                   torch.empty((H, 13, 13, B), device=X.device))
        out = tuple(out)
        if box and len(out) == 5:
            out += (torch.empty((H, 7, B), device=X.device, dtype=torch.int8), torch.empty((2, B), device=X.device, dtype=torch.int32))
        assert len(out) == (7 if box else 5), "out: K, kff, dV, Vx (N, 13, B), Vxx (N, 13, 13, B), then act and stat with box=True"
        K, kff, dV, Vx, Vxx = out[:5]
        assert (Vx is None) == (Vxx is None), "Vx and Vxx go together"
        act, stat = (out[5], out[6]) if box else (None, None)
        if box:
            assert act.dtype == torch.int8 and stat.dtype == torch.int32 and act.is_contiguous() and stat.is_contiguous()
        if uglin is not None:
            assert node is not None and Hz is not None
        vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        _lib.check(lib.ac_ilqr_backward_shoot_f32(self.system._handle, self._cstruct(), *self._ptrs(node), vp(uglin), vp(Hz),
                                                  X.data_ptr(), U.data_ptr(), A.data_ptr(), Bm.data_ptr(), F.data_ptr(), B, H,
                                                  K.data_ptr(), kff.data_ptr(), dV.data_ptr(), vp(Vx), vp(Vxx), 1 if box else 0,
                                                  vp(act), vp(stat), self.system._stream()), "ac_ilqr_backward_shoot_f32")
        return out

    def direction(self, X, F, A, Bm, K, kff, Vx=None, Vxx=None, out=None, U=None):
        """shooting='multiple': the forward sweep  dx_0 = 0, du_k = kff_k + K_k dx_k, dx_{k+1} = A_k dx_k + B_k du_k + F_k - x_{k+1}
        -> dX (N+1, 13, B), dU (N, 7, B), Lam (N, 13, B) = Vx[k] + Vxx[k] dx_{k+1} (None without Vx / Vxx): the solution of the
        equality-constrained QP of the iteration and the multipliers of its defect rows (ac_shoot_direction_f32).
        U (N, 7, B): clip the control step as it is formed, du_k = clip(U_k + kff_k + K_k dx_k, u_min, u_max) - U_k, dX following
        the clipped step — what `iterate` does, so that the candidates stay consistent where the box binds."""
        torch = _torch()
        lib = self.system._sync()
        H, B = kff.shape[0], kff.shape[2]
        assert (Vx is None) == (Vxx is None), "Vx and Vxx go together"
        if out is None:
            out = (torch.empty((H + 1, 13, B), device=X.device), torch.empty((H, 7, B), device=X.device),
                   torch.empty((H, 13, B), device=X.device) if Vx is not None else None)
        dX, dU, Lam = out
        vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        _lib.check(lib.ac_shoot_direction_f32(self.system._handle, self._cstruct() if U is not None else None, X.data_ptr(), vp(U),
                                              F.data_ptr(), A.data_ptr(), Bm.data_ptr(),
                                              K.data_ptr(), kff.data_ptr(), vp(Vx), vp(Vxx), B, H, dX.data_ptr(), dU.data_ptr(),
                                              vp(Lam if Vx is not None else None), self.system._stream()), "ac_shoot_direction_f32")
        return dX, dU, (Lam if Vx is not None else None)

    def _merit(self, J, mu, phi, dinf, R=None, F=None, X=None):
        lib = self.system._sync()
        src = R if R is not None else F
        H, Bc = src.shape[0], src.shape[2]
        vp = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        _lib.check(lib.ac_shoot_merit_f32(self.system._handle, J.data_ptr(), mu.data_ptr(), mu.shape[0], vp(R), vp(F), vp(X), Bc, H,
                                          phi.data_ptr(), dinf.data_ptr(), self.system._stream()), "ac_shoot_merit_f32")
        return phi, dinf

    def _shoot_search(self, X, U, ws, env):
        """Direction, merit weight, the candidates of every alpha as independent nodes, their merit, the acceptance."""
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        na = len(self.alphas)
        self.direction(X, ws["F"], ws["A"], ws["Bm"], ws["K"], ws["kff"], ws["Vx"], ws["Vxx"], out=(ws["dX"], ws["dU"], ws["Lam"]),
                       U=U)
        _lib.check(lib.ac_shoot_merit_weight_f32(self.system._handle, ws["Lam"].data_ptr(), C.c_float(self.merit_factor), B, H,
                                                 ws["mu"].data_ptr(), self.system._stream()), "ac_shoot_merit_weight_f32")
        arr = (C.c_float * na)(*self.alphas)
        _lib.check(lib.ac_shoot_candidates_f32(self.system._handle, self._cstruct(), X.data_ptr(), U.data_ptr(), ws["dX"].data_ptr(),
                                               ws["dU"].data_ptr(), arr, na, B, H, ws["Xc"].data_ptr(), ws["Uc"].data_ptr(),
                                               self.system._stream()), "ac_shoot_candidates_f32")
        _lib.check(lib.ac_shoot_defect_f32(self.system._handle, ws["Xc"].data_ptr(), ws["Uc"].data_ptr(), C.c_float(self.dt),
                                           C.c_void_p(0), na * B, H, ws["Rc"].data_ptr(), self.system._stream()),
                   "ac_shoot_defect_f32")
        self.trajectory_cost(ws["Xc"], ws["Uc"], out=ws["Jc"])
        self.trajectory_cost(X, U, out=ws["J0"])
        if env:
            self.envelope_cost(ws["Xc"], ws["Jc"])
            self.envelope_cost(X, ws["J0"])
        self._merit(ws["Jc"], ws["mu"], ws["phic"], ws["dinfc"], R=ws["Rc"])
        self._merit(ws["J0"], ws["mu"], ws["phi0"], ws["dinf0"], F=ws["F"], X=X)   # the iterate's own F: no second step evaluation
        ws["shoot_done"] = True
        return self.accept(ws["phic"], ws["phi0"], ws["Xc"], ws["Uc"], X, U)

    def measure(self, X, U):
        """shooting='multiple': (cost J (B,), largest |defect| (B,)) of an iterate — one step launch; fresh tensors."""
        torch = _torch()
        B = U.shape[2]
        ws = self._workspace(B, U.device)
        R = self.defects(X, U)
        J = self.trajectory_cost(X, U).clone()
        if self.envelope_weight > 0:
            self.envelope_cost(X, J)
        phi, dinf = torch.empty_like(J), torch.empty_like(J)
        self._merit(J, ws["mu"], phi, dinf, R=R)
        return J, dinf

    def backward(self, X, U, A, Bm, out=None, Hz=None, node="auto", uglin=None, rate=None, box=False, shoot=None):
        """Riccati pass -> K (N, 7, 13, B), kff (N, 7, B), dV (2, B).  Hz (N, 21, 21, B): optional second-order
        dynamics blocks from `hessian()` (exact-Hessian / Newton step).  uglin (N, 7, B): optional per-node control
        gradient (needs node arrays and Hz: ac_ilqr_backward_goal_f32).
        rate = (rate_g, rate_h), each (N, 7, B): the control-rate term per difference u_k - u_{k-1}, carried exactly
        (ac_ilqr_backward_rate_f32) -> K, kff, dV, Kp (N, 7, 7, B); `out` then takes the four.
        box=True: the control box as a QP per node (ac_ilqr_backward_box_f32 / ac_ilqr_backward_rate_box_f32); the result — and
        `out` — then carries act (N, 7, B) int8 and stat (2, B) int32 after the outputs above.
        shoot = F (N, 13, B), the step results F(x_k, u_k) of `linearise`: the pass over a multiple-shooting iterate, whose node k
        reads V'_x + V'_xx (F_k - x_{k+1}) in place of V'_x (ac_ilqr_backward_shoot_f32) -> K, kff, dV, Vx (N, 13, B),
        Vxx (N, 13, 13, B) — the value expansion node k starts from, what `direction` needs for the multipliers — then act, stat
        with box=True; in `out`, Vx and Vxx may both be None."""
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        if isinstance(node, str):
            node = self._node_cost(X, U)
        if shoot is not None:
            assert rate is None, "the rate kernels have no defect switch"
            return self._backward_shoot(X, U, A, Bm, shoot, out, Hz, node, uglin, box)
        if rate is not None:
            assert uglin is None, "the rate gradient arrives in `rate`"
        if box:
            return self._backward_box(X, U, A, Bm, out, Hz, node, uglin, rate)
        if rate is not None:
            if out is None:
                out = (torch.empty((H, 7, 13, B), device=X.device), torch.empty((H, 7, B), device=X.device),
                       torch.empty((2, B), device=X.device), torch.empty((H, 7, 7, B), device=X.device))
            K, kff, dV, Kp = out
            _lib.check(lib.ac_ilqr_backward_rate_f32(self.system._handle, self._cstruct(), *self._ptrs(node),
                                                     C.c_void_p(Hz.data_ptr() if Hz is not None else 0), rate[0].data_ptr(),
                                                     rate[1].data_ptr(), X.data_ptr(), U.data_ptr(), A.data_ptr(),
                                                     Bm.data_ptr(), B, H, K.data_ptr(), Kp.data_ptr(), kff.data_ptr(),
                                                     dV.data_ptr(), self.system._stream()), "ac_ilqr_backward_rate_f32")
            return K, kff, dV, Kp
        if out is None:
            out = (torch.empty((H, 7, 13, B), device=X.device), torch.empty((H, 7, B), device=X.device),
                   torch.empty((2, B), device=X.device))
        K, kff, dV = out
        if uglin is not None:
            assert node is not None and Hz is not None
            _lib.check(lib.ac_ilqr_backward_goal_f32(self.system._handle, self._cstruct(), *self._ptrs(node),
                                                     C.c_void_p(uglin.data_ptr()), C.c_void_p(Hz.data_ptr()), X.data_ptr(),
                                                     U.data_ptr(), A.data_ptr(), Bm.data_ptr(), B, H, K.data_ptr(),
                                                     kff.data_ptr(), dV.data_ptr(), self.system._stream()),
                       "ac_ilqr_backward_goal_f32")
            return K, kff, dV
        _lib.check(lib.ac_ilqr_backward_newton_f32(self.system._handle, self._cstruct(), *self._ptrs(node),
                                                   C.c_void_p(Hz.data_ptr() if Hz is not None else 0), X.data_ptr(),
                                                   U.data_ptr(), A.data_ptr(), Bm.data_ptr(), B, H, K.data_ptr(),
                                                   kff.data_ptr(), dV.data_ptr(), self.system._stream()),
                   "ac_ilqr_backward_newton_f32")
        return K, kff, dV

    def forward(self, x0, Xnom, U, K, kff, alphas=None, out=None, Kp=None):
        """Closed-loop rollouts for every alpha: Xc (H+1, 13, n_alpha*B), Uc (H, 7, n_alpha*B); column a*B + b.
        Kp (N, 7, 7, B): the gains on the previous control of `backward(rate=)` (ac_rollout_policy_rate_f32)."""
        torch = _torch()
        lib = self.system._sync()
        alphas = self.alphas if alphas is None else [float(a) for a in alphas]
        na = len(alphas)
        H, B = U.shape[0], U.shape[2]
        if out is None:
            out = (torch.empty((H + 1, 13, na * B), device=U.device), torch.empty((H, 7, na * B), device=U.device))
        Xc, Uc = out
        arr = (C.c_float * na)(*alphas)
        if Kp is not None:
            _lib.check(lib.ac_rollout_policy_rate_f32(self.system._handle, self._cstruct(), x0.data_ptr(), Xnom.data_ptr(),
                                                      U.data_ptr(), K.data_ptr(), Kp.data_ptr(), kff.data_ptr(), arr, na,
                                                      C.c_float(self.dt), B, H, Xc.data_ptr(), Uc.data_ptr(),
                                                      self.system._stream()), "ac_rollout_policy_rate_f32")
            return Xc, Uc
        _lib.check(lib.ac_rollout_policy_f32(self.system._handle, self._cstruct(), x0.data_ptr(), Xnom.data_ptr(),
                                             U.data_ptr(), K.data_ptr(), kff.data_ptr(), arr, na, C.c_float(self.dt),
                                             B, H, Xc.data_ptr(), Uc.data_ptr(), self.system._stream()),
                   "ac_rollout_policy_f32")
        return Xc, Uc

    def iterate(self, x0, X, U):
        """One iLQR iteration in place on (X, U).  Returns (cost (B,), improved (B,) bool).
        shooting='multiple': X need not be the rollout of U; the first result is the accepted MERIT J + mu sum |defect|
        (the cost and the defect of the iterate the iteration started from are left in the workspace: `last_defect`)."""
        torch = _torch()
        B = U.shape[2]
        ws = self._workspace(B, U.device)
        na = len(self.alphas)
        if self.time_row > 0:
            # linearise at the nodes' own steps dt_k = U[k, time_row]; its derivative c = dF/d(dt) IS the column of B for that row
            ws["dt"].copy_(U[:, self.time_row, :])
            self.linearise(X, U, dt=ws["dt"], want_c=True, out=(ws["F"], ws["A"], ws["Bm"], ws["c"]))
            ws["Bm"][:, :, self.time_row, :].copy_(ws["c"])
        else:
            self.linearise(X, U, want_c=False, out=(ws["F"], ws["A"], ws["Bm"], None))
        node = self._node_cost(X, U)  # None, or a subclass's per-node arrays (rewritten by it every iteration)
        Hz = None
        env = self.envelope_weight > 0
        goal = self._goal_model is not None  # GoalAcquisition: node arrays + control gradient + (u, u) curvature
        exact_rate = self._rate_exact       # the rate term per difference, u_{k-1} carried through the backward pass
        if self.hessian_mode != "exact" and (env or (goal and not exact_rate)):
            Hz = ws["Hz"].zero_()
        # (first: it WRITES the node arrays the envelope below adds to; adds the rate curvature to Hz, returns the control gradient)
        uglin = self._goal_model(X, U, Hz) if (goal and not exact_rate) else None
        rate = None
        if exact_rate:
            rate = (ws["rate_g"], ws["rate_h"])
            if goal:
                self._goal_model_rate(X, U, rate)  # the node arrays too
            else:
                self.rate_model(U, out=rate)
        if env:
            if node is None:  # the constant cost as per-node arrays, so that the penalty gradient has a place to go
                ws["env_glin"].zero_()
                node = (ws["env_q"], ws["env_xref"], ws["env_glin"])
            self._envelope_model(X, glin=node[2])  # before the costate: the multipliers see the penalty too
        if self.hessian_mode == "exact":
            self.costate(X, ws["A"], node, out=ws["Lam"])
            Hz = self.hessian(X, U, ws["Lam"], out=ws["Hz"])
        if env:
            self._envelope_model(X, Hz=Hz)
        qp = self.box == "qp"
        extra = (ws["act"], ws["stat"]) if qp else ()
        if self.shooting == "multiple":
            assert rate is None, "shooting='multiple' does not combine with rate='exact' yet"
            self.backward(X, U, ws["A"], ws["Bm"], out=(ws["K"], ws["kff"], ws["dV"], ws["Vx"], ws["Vxx"]) + extra, Hz=Hz, node=node,
                          uglin=uglin, box=qp, shoot=ws["F"])
            return self._shoot_search(X, U, ws, env)
        if rate is not None:
            self.backward(X, U, ws["A"], ws["Bm"], out=(ws["K"], ws["kff"], ws["dV"], ws["Kp"]) + extra, Hz=Hz, node=node, rate=rate,
                          box=qp)
            self.forward(x0, X, U, ws["K"], ws["kff"], out=(ws["Xc"], ws["Uc"]), Kp=ws["Kp"])
        else:
            self.backward(X, U, ws["A"], ws["Bm"], out=(ws["K"], ws["kff"], ws["dV"]) + extra, Hz=Hz, node=node, uglin=uglin,
                          box=qp)
            self.forward(x0, X, U, ws["K"], ws["kff"], out=(ws["Xc"], ws["Uc"]))
        self.trajectory_cost(ws["Xc"], ws["Uc"], out=ws["Jc"])
        self.trajectory_cost(X, U, out=ws["J0"])
        if env:
            self.envelope_cost(ws["Xc"], ws["Jc"])
            self.envelope_cost(X, ws["J0"])
        return self.accept(ws["Jc"], ws["J0"], ws["Xc"], ws["Uc"], X, U)

    def accept(self, Jc, J0, Xc, Uc, X, U):
        """Line-search acceptance in ONE launch (`ac_ilqr_accept_f32`): per instance the cheapest finite candidate replaces
        the iterate (X, U) in place if it beats J0.  Returns (accepted cost (B,), improved (B,) bool)."""
        torch = _torch()
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        na = Jc.numel() // B
        ws = self._workspace(B, U.device)
        Ja, imp = ws["Ja"], ws["improved"]
        _lib.check(lib.ac_ilqr_accept_f32(self.system._handle, Jc.data_ptr(), J0.data_ptr(), Xc.data_ptr(), Uc.data_ptr(),
                                          na, B, H, X.data_ptr(), U.data_ptr(), Ja.data_ptr(), imp.data_ptr(),
                                          self.system._stream()), "ac_ilqr_accept_f32")
        return Ja, imp

    def _solve_shoot(self, x0, U, X0, iters, save_to, save_instance, al_every):
        torch = _torch()
        H, B = U.shape[0], U.shape[2]
        if X0 is None:
            X = self.rollout(x0, U)
        else:
            assert tuple(X0.shape) == (H + 1, 13, B), "X0: (N + 1, 13, B)"
            X = X0.to(device=U.device, dtype=torch.float32).clone().contiguous()
            X[0].copy_(x0)
        ws = self._workspace(B, U.device)
        ws["mu"].fill_(self.defect_weight)
        hist, dhist = [], []
        if save_to:
            self.save_progress(save_to, 0, X, U, save_instance, mode="w")
        for it in range(iters):
            self.iterate(x0, X, U)   # (J and the defect of the iterate it started from are by-products of its line search)
            hist.append(ws["J0"].clone()); dhist.append(ws["dinf0"].clone())
            if al_every and self.envelope_mode == "al" and (it + 1) % al_every == 0 and it + 1 < iters:
                self.update_multipliers(X)
            if save_to:
                self.save_progress(save_to, it + 1, X, U, save_instance)
        J, dinf = self.measure(X, U)
        hist.append(J); dhist.append(dinf)
        self.defect_history = torch.stack(dhist)
        return X, U, torch.stack(hist)

    def solve(self, x0, U0, iters: int = 10, save_to: Optional[str] = None, save_instance: int = 0, al_every: int = 0,
              u_prev=None, X0=None):
        """Rollout from x0 with U0, then `iters` iLQR iterations.  Returns (X, U, cost history (iters+1, B)).
        shooting='multiple': X0 (N+1, 13, B) is the state guess (its row block 0 is overwritten with x0; None: the rollout, whose
        gaps are rounding only); the history holds the COST J of every iterate, `defect_history` (iters+1, B) its largest |defect|.
        u_prev (7, B), with `rate_weight`: the control applied before the window; the rate cost then has a k = 0 term.
        `save_to` writes instance `save_instance` after every iteration in the reference's trajectory format
        (iteration_0 = the initial rollout), the role of the IPOPT callback in control/base.py:60-86.
        al_every > 0 (envelope = 'al'): a multiplier update after every al_every-th sweep."""
        torch = _torch()
        U = U0.clone()
        if u_prev is not None:
            assert self.rate_weight is not None, "u_prev needs ILQR(rate_weight=)"
            assert tuple(u_prev.shape) == (7, U0.shape[2]), "u_prev: (7, B)"
            u_prev = u_prev.to(device=U0.device, dtype=torch.float32).contiguous()
        self._u_prev = u_prev
        assert X0 is None or self.shooting == "multiple", "a state guess X0 needs ILQR(shooting='multiple')"
        if self.shooting == "multiple":
            return self._solve_shoot(x0, U, X0, iters, save_to, save_instance, al_every)
        if self.time_row > 0:
            U[:, self.time_row, :] = self.dt  # every node starts at the nominal step (the rollout below uses it)
        X = self.rollout(x0, U)
        J = self.trajectory_cost(X, U).clone()
        if self.envelope_weight > 0:  # the same objective as every later entry (iterate() adds the penalty)
            self.envelope_cost(X, J)
        hist = [J]
        if save_to:
            self.save_progress(save_to, 0, X, U, save_instance, mode="w")
        for it in range(iters):
            J, _ = self.iterate(x0, X, U)
            hist.append(J.clone())
            if al_every and self.envelope_mode == "al" and (it + 1) % al_every == 0 and it + 1 < iters:
                self.update_multipliers(X)  # (the objective changes with the multipliers: the history is monotone between updates)
            if save_to:
                self.save_progress(save_to, it + 1, X, U, save_instance)
        return X, U, torch.stack(hist)


class GoalAcquisition(ILQR):
    """The reference's goal-acquisition problem (Controller, main/control/control.py:25-70) on the batched sweep: reach
    goal (x, y) at the final node while the loss of Controller.loss is minimised —

        1000 |p_xy(N) - goal|^2 + 100 sum l0_smooth(u_{k+1} - u_k, 1e-2) + (z_N - z_0)^2 - sum v_rel.v_rel / 100 / N
        + vel_param 1000 v_x(N) + 1000 (v_y(N)^2 + v_z(N)^2) [+ 10000 T],     subject to  v_x(N) < -2

    — for B instances at once (independent goals / initial states / random restarts).  The EXACT loss drives the line
    search and the history (ac_goal_cost_f32); the backward pass sees its convex quadratic model (ac_goal_model_f32:
    csrc/ac_goal.hpp states what is modelled how); the terminal inequality is an augmented-Lagrangian term with one
    multiplier per instance, updated by `update_goal_multiplier()` (`solve(al_every=)`).  time='variable' adds the
    reference's time term 10000 T through w_time (opts['time'] = 'progress' in the reference's driver, control.py:182).
    rate: how the backward pass models the control-rate term — 'frozen' (neighbours u_{k-1}, u_{k+1} held at the iterate, the
    diagonal curvature only) or 'exact' (ac_goal_model_rate_f32: the term per difference, u_{k-1} carried through the pass).
    The exact loss is the same either way."""

    def __init__(self, *, system, goal, dt: float = 0.01, num_nodes: int = 400, vel_param: float = 1.0, w_goal: float = 1000.0,
                 w_rate: float = 100.0, eps_rate: float = 1e-2, w_height: float = 1.0, w_speed: float = 0.01,
                 w_final_velocity: float = 1000.0, vx_max: float = -2.0, w_al: float = 10.0, r: float = 0.0, reg: float = 1e-2,
                 time: str = "fixed", w_time: float = 10000.0, rate: str = "frozen", **kw):
        assert rate in ("frozen", "exact")
        assert not (rate == "exact" and kw.get("rate_weight") is not None), "rate='exact' and rate_weight do not combine"
        cost = QuadraticCost(q=[0.0] * 13, qf=[0.0] * 13, r=[float(r)] * 7, reg=float(reg))  # every state term lives in the node arrays
        super().__init__(system=system, dt=dt, num_nodes=num_nodes, cost=cost, time=time, w_time=w_time if time == "variable" else 0.0,
                         **kw)
        assert self.hessian_mode == "gauss-newton"
        assert not (rate == "exact" and self.shooting == "multiple"), "shooting='multiple' does not combine with rate='exact' yet"
        self.rate_mode = rate
        if rate == "exact":
            self._rate_exact = True
        self.goal = goal
        self.loss = _lib.GoalLoss()
        ls = self.loss
        ls.w_goal, ls.w_rate, ls.eps_rate, ls.w_height, ls.w_speed = w_goal, w_rate, eps_rate, w_height, w_speed
        ls.w_vx, ls.w_vyz, ls.vx_max, ls.w_al, ls.time_row = vel_param * w_final_velocity, w_final_velocity, vx_max, w_al, self.time_row
        self._gws = None

    def _goal_ws(self, B, dev):
        torch = _torch()
        H = self.num_nodes
        if self._gws is None or self._gws["key"] != (B, H, str(dev)):
            f = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)  # noqa: E731
            g = torch.as_tensor(self.goal, dtype=torch.float32, device=dev).reshape(2, -1)
            if g.shape[1] == 1:
                g = g.expand(2, B)
            assert g.shape == (2, B), "goal: (2,) for every instance or (2, B)"
            self._gws = dict(key=(B, H, str(dev)), goal=g.contiguous(), lam=f(B), viol=f(B), nq=f(H + 1, 13, B),
                             nx=f(H + 1, 13, B), ng=f(H + 1, 13, B), ug=f(H, 7, B))
            ws = self._workspace(B, dev)
            if "Hz" not in ws:
                ws["Hz"] = f(H, 21, 21, B)
        return self._gws

    # the node arrays are produced together with the control gradient (one launch) in _goal_model; _node_cost hands them over
    def _node_cost(self, X, U):
        g = self._goal_ws(U.shape[2], U.device)
        return (g["nq"], g["nx"], g["ng"])

    def _goal_model(self, X, U, Hz):
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        g = self._goal_ws(B, U.device)
        _lib.check(lib.ac_goal_model_f32(self.system._handle, C.byref(self.loss), g["goal"].data_ptr(), g["lam"].data_ptr(),
                                         X.data_ptr(), U.data_ptr(), B, H, g["nq"].data_ptr(), g["nx"].data_ptr(),
                                         g["ng"].data_ptr(), g["ug"].data_ptr(), Hz.data_ptr(), self.system._stream()),
                   "ac_goal_model_f32")
        return g["ug"]

    def _goal_model_rate(self, X, U, rate):
        """The node arrays (as _goal_model) and the l0 term per difference u_k - u_{k-1} into rate = (rate_g, rate_h)."""
        lib = self.system._sync()
        H, B = U.shape[0], U.shape[2]
        g = self._goal_ws(B, U.device)
        _lib.check(lib.ac_goal_model_rate_f32(self.system._handle, C.byref(self.loss), g["goal"].data_ptr(), g["lam"].data_ptr(),
                                              X.data_ptr(), U.data_ptr(), B, H, g["nq"].data_ptr(), g["nx"].data_ptr(),
                                              g["ng"].data_ptr(), rate[0].data_ptr(), rate[1].data_ptr(),
                                              self.system._stream()), "ac_goal_model_rate_f32")
        return rate

    def trajectory_cost(self, X, U, out=None):
        """The exact loss of every column of (X, U) (a candidate batch reads instance b % B's goal and multiplier)."""
        lib = self.system._sync()
        out = super().trajectory_cost(X, U, out=out)  # control terms of the cost struct (actuation, time)
        Bc, H = U.shape[2], U.shape[0]
        Bn = self._gws["key"][0] if self._gws is not None else Bc
        g = self._goal_ws(Bn, U.device)
        _lib.check(lib.ac_goal_cost_f32(self.system._handle, C.byref(self.loss), g["goal"].data_ptr(), g["lam"].data_ptr(), Bn,
                                        X.data_ptr(), U.data_ptr(), Bc, H, out.data_ptr(), self.system._stream()),
                   "ac_goal_cost_f32")
        return out

    def update_goal_multiplier(self, X):
        """First-order update of the terminal inequality's multipliers at the iterate; returns max(0, v_x(N) - vx_max) (B,)."""
        lib = self.system._sync()
        H, B = X.shape[0] - 1, X.shape[2]
        g = self._goal_ws(B, X.device)
        _lib.check(lib.ac_goal_multiplier_f32(self.system._handle, C.byref(self.loss), X.data_ptr(), B, H, g["lam"].data_ptr(),
                                              g["viol"].data_ptr(), self.system._stream()), "ac_goal_multiplier_f32")
        return g["viol"]

    def solve(self, x0, U0, iters: int = 10, al_every: int = 0, **kw):
        torch = _torch()
        self._goal_ws(U0.shape[2], U0.device)
        if not al_every:
            return super().solve(x0, U0, iters=iters, **kw)
        # multiplier updates between blocks of sweeps (the objective changes with them: monotone within a block)
        X, U, hist = super().solve(x0, U0, iters=min(al_every, iters), **kw)
        hists, done = [hist], min(al_every, iters)
        dhs = [self.defect_history]
        while done < iters:
            self.update_goal_multiplier(X)
            n = min(al_every, iters - done)
            if self.shooting == "multiple":
                kw = dict(kw, X0=X)   # the iterate's states are decision variables: the next block starts from them
            X, U, h = super().solve(x0, U, iters=n, **kw)
            hists.append(h)
            dhs.append(self.defect_history)
            done += n
        if self.shooting == "multiple":
            self.defect_history = torch.cat(dhs)
        return X, U, torch.cat(hists)
