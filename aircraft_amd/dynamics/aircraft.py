"""Fixed-wing plugin of the batched 6-DoF model — the reference's `Aircraft(opts)` / `AircraftOpts`
(src/aircraft/dynamics/aircraft.py:22-330) on MI355X.

Same constructor options and mutable attributes (`com`, `mass`, `normalise`,
`physical_integration_substeps`, `stall_scaling`); 7 controls
[aileron, elevator, rudder (deg), thrust(3), flaps] (aircraft.py:143-166)."""
from __future__ import annotations

from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Tuple, Union

import ctypes as C

import numpy as np

from .. import _lib
from ..utils import AircraftConfiguration
from .base import SixDOF, SixDOFOpts
from .coefficient_models import COEFF_MODEL_REGISTRY, CoefficientModel, DefaultModel

__all__ = ["Aircraft", "AircraftOpts", "TrimResult", "LqrResult", "ModesResult", "EKF", "EkfTrace", "EkfSmooth", "EkfNoiseStats",
           "EkfNoiseFit", "UKF", "SensorModel", "LqgResult"]


def _torch_mod():
    import torch

    return torch


@dataclass
class AircraftOpts(SixDOFOpts):
    """reference dynamics/aircraft.py:22-38"""
    coeff_model_type: str = "default"  # "linear", "poly", "nn", or "default"
    coeff_model_path: Union[Path, str, object] = ""  # .csv / .pkl / .pth / .npz, or in-memory model data
    realtime: bool = False
    aircraft_config: AircraftConfiguration = field(default_factory=lambda: AircraftConfiguration({}))
    stall_angle_alpha: Tuple[float, float] = (float(np.deg2rad(-10)), float(np.deg2rad(10)))
    stall_angle_beta: Tuple[float, float] = (float(np.deg2rad(-10)), float(np.deg2rad(10)))
    stall_scaling: bool = False
    use_mfma: bool = True  # build-side: False selects the VALU matmul for the "nn" model

    def __post_init__(self):
        self.mass = self.aircraft_config.mass
        # unknown keys silently fall back to "default", as in the reference (aircraft.py:37)
        factory = COEFF_MODEL_REGISTRY.get(self.coeff_model_type, COEFF_MODEL_REGISTRY["default"])
        self.coefficient_model = lambda aircraft: factory(self.coeff_model_path, aircraft, realtime=self.realtime,
                                                          use_mfma=self.use_mfma)


@dataclass
class TrimResult:
    """Aircraft.trim's result for n instances (numpy in -> numpy out; tensors stay on the device).
    x (13, n) and u (7, n): the trimmed state and control; z (6, n) = (alpha, theta, phi [rad], aileron, elevator [deg],
    rudder [deg] (lateral mode 0) | beta [rad] (mode 1)); residual (6, n) = (r_v [m/s^2], r_w [rad/s^2]) at z; status (n,):
    0 converged, 1 not converged within iters, 2 stopped on a bound, 3 non-finite (include/aircraft_hip.h, ac_trim_f32);
    converged (n,) = status == 0."""
    x: Any
    u: Any
    z: Any
    residual: Any
    status: Any
    converged: Any


@dataclass
class LqrResult:
    """Aircraft.lqr's result for n instances (numpy in -> numpy out; tensors stay on the device).
    K (7, 12, n): the constant gain of u = u_b - K xi in the steady-flight chart xi (Aircraft.steady_error); P (12, 12, n): the
    solution of the discrete Riccati equation; A (12, 12, n), B (12, 7, n): the step linearised in the chart; x (13, n),
    u (7, n): the nominal; residual (n,): max|Q + A'PA - A'PB K - P| / max|P|; status (n,): 0 converged, 1 not converged
    within iters, 2 breakdown, 3 non-finite input (include/aircraft_hip.h, ac_lqr_f32); converged (n,) = status == 0;
    iterations (n,): doubling steps taken.  dt, q, r: what the gain was designed for."""
    K: Any
    P: Any
    A: Any
    B: Any
    x: Any
    u: Any
    residual: Any
    status: Any
    converged: Any
    iterations: Any
    dt: float = 0.0
    q: Any = None
    r: Any = None
    system: Any = field(default=None, repr=False)

    def gains(self, Xnom):
        """Raw-state gains K_x,k = -K E(x_k) along a nominal Xnom (H+1, 13, n) -> (H, 7, 13, n): the feedback
        u = U_k + K_x,k (x - Xnom_k) of ac_rollout_policy_f32 / ILQR.closed_loop."""
        return self.system._lqr_gains(Xnom, self.K)


@dataclass
class ModesResult:
    """Aircraft.modes' result for n instances (numpy in -> numpy out, float64 / complex128; tensors stay on the device,
    complex64).  lam (m, n): the eigenvalues of the step linearised in the kept chart coordinates, in the canonical order
    (descending |lam|, then descending imaginary part, then descending real part; include/aircraft_hip.h, ac_eig_f32);
    s (m, n) = log(lam) / dt = sigma + i omega [1/s, rad/s]; wn = |s| [rad/s]; zeta = -sigma / |s| (NaN where s = 0);
    rho (n,) = max |lam|; unstable (n,): the number of |lam| > 1; A (12, 12, n), B (12, 7, n): the step linearised in the
    chart (what Aircraft.lqr returns); coords: the kept chart coordinates; status (n,): 0 all eigenvalues found, 1 the
    iteration cap was reached, 3 non-finite input (lam, s NaN); converged (n,) = status == 0; iterations (n,): QR iterations
    used; dt: the step length."""
    lam: Any
    s: Any
    wn: Any
    zeta: Any
    rho: Any
    unstable: Any
    A: Any
    B: Any
    coords: Any
    status: Any
    converged: Any
    iterations: Any
    dt: float = 0.0


@dataclass
class EkfTrace:
    """What a filter step (EKF.step / EKF.update) or T of them (EKF.filter: a leading axis T on everything but ll) report for
    n instances (numpy in -> numpy out; tensors stay on the device).  X (13, n), P (12, 12, n): the posterior estimate and
    its covariance in the error coordinates (dp, dv, dtheta, dw); nu, S (15, n): innovation and innovation variance of every
    used row in the order the rows were applied (row i given the rows before it), 0 for unused rows; nis (n,) = sum nu^2 / S;
    ll (n,): the log-likelihood -1/2 sum (log 2 pi S + nu^2 / S), for a filter summed over its steps; used (n,): bits of the
    used rows; status (n,): 0, bit 1 a used row was rejected (S <= 0 or non-finite), bit 2 the prediction was not finite
    (include/aircraft_hip.h, ac_ekf_step_f32).  EKF.filter(record=True) adds what EKF.smooth reads: Xpred (T, 13, n), Ppred,
    Abar (T, 12, 12, n), the prediction of every step and the Jacobian that carried the error state into it, and X0, P0, the
    estimate the run started from."""
    X: Any
    P: Any
    nu: Any
    S: Any
    nis: Any
    ll: Any
    used: Any
    status: Any
    Xpred: Any = None
    Ppred: Any = None
    Abar: Any = None
    X0: Any = None
    P0: Any = None


@dataclass
class EkfSmooth:
    """What EKF.smooth returns for a recorded filter run of T steps (numpy in -> numpy out; tensors stay on the device): the
    fixed-interval (Rauch-Tung-Striebel) estimate of every node given the whole run (include/aircraft_hip.h,
    ac_ekf_smooth_f32).
    X (T, 13, n), P (T, 12, 12, n): the smoothed states and their covariances in the error coordinates (dp, dv, dtheta, dw);
    the last node is the filtered one.  X0 (13, n), P0 (12, 12, n): the smoothed initial estimate (initial=True; else None).
    C (T, 12, 12, n) (gains=True; else None): the smoother gain C_k of link k, which carries node k's correction back to node
    k-1 (C[0] belongs to the initial node and is zero without it); the lag-one smoothed covariance is
    Cov(d_k, d_{k-1} | all data) = P^s_k C_k', the cross term an EM estimate of Q and R needs.
    status (T, n): per link 0, bit 1 (value 1) the predicted covariance of node k was not positive definite, bit 2 (value 2) an
    operand of the link was not finite; in both cases the gain of that link is zero and node k-1 is the filtered one."""
    X: Any
    P: Any
    X0: Any
    P0: Any
    C: Any
    status: Any


@dataclass
class EkfMapSmooth:
    """What EKF.map_smooth returns (numpy in -> numpy out; tensors stay on the device): the maximum-a-posteriori trajectory of
    a log by Gauss-Newton, the iterated extended Kalman smoother (include/aircraft_hip.h, ac_ieks_solve_f32).
    X (T, 13, n), P (T, 12, 12, n), X0 (13, n), P0 (12, 12, n): the smoothed nodes and the smoothed initial node of the last
    linearised pass, as EkfSmooth's.  cost (iters + 1, n): the MAP cost J of the nominal before the first iteration and after
    each; alpha (iters, n): the accepted step length of each iteration, 0 where no candidate lowered J.  status (n,): bit 1
    (value 1) the prior covariance has no Cholesky factor, bit 2 (value 2) a node or J was not finite, bit 3 (value 4) a defect
    in a row whose q is 0, bit 4 (value 8) an iteration found no decrease (the nominal then stays where it is).  trace: the
    EkfTrace of the last pass (with Xpred, Ppred, Abar, X0, P0), which EKF.smooth and EKF.noise_stats accept; nominal
    (T + 1, 13, n): the final nominal, the initial node first."""
    X: Any
    P: Any
    X0: Any
    P0: Any
    cost: Any
    alpha: Any
    status: Any
    trace: Any
    nominal: Any


@dataclass
class EkfNoiseStats:
    """What EKF.noise_stats returns for a recorded filter run and its smoothed trace (numpy in -> numpy out; tensors stay on
    the device): the M-step of an EM estimate of the diagonal Q and R (include/aircraft_hip.h, ac_ekf_em_f32).
    Qsum (12, n), nq (n,): the sum over the counted nodes of E[w_kj^2 | all data] and their number; Rsum, nr (15, n): the sum of
    (z_i - h_i(x^s_k))^2 + h_i P^s_k h_i' over the nodes at which row i was used, and their number.  q (12, n), r (15, n): the new
    variances max(sum / count, floor x the bank's), the bank's own where nothing was counted.  status (T, n) per node: 0, 1 the
    predicted covariance was not positive definite (the node is out of Q, its R terms count), 2 an operand was not finite (the
    node adds nothing)."""
    Qsum: Any
    Rsum: Any
    nq: Any
    nr: Any
    q: Any
    r: Any
    status: Any


@dataclass
class EkfNoiseFit:
    """What EKF.fit_noise returns: q (12, n), r (15, n) the fitted variances (the bank holds them); ll (iters + 1, n): the
    filter's log-likelihood before each update and after the last one; nq, nr, status: EkfNoiseStats' of the last iteration."""
    q: Any
    r: Any
    ll: Any
    nq: Any
    nr: Any
    status: Any


class EKF:
    """A bank of n extended Kalman filters over one Aircraft's step sensitivities (Aircraft.ekf).  `x`
    (13, n) and `P` (12, 12, n) are the current estimate; step / update / filter advance it and return an EkfTrace.
    Measurement rows z (15, n): GPS position (3), GPS velocity NED (3), gyro (3), air data V, alpha, beta (3), magnetometer (3);
    a row is used when its mask bit is set (mask (n,) integers, bit i = row i; None: all) and its z is finite, so a sensor
    that did not report is a NaN or a cleared bit.  No host synchronisation: with `ws` from Aircraft.ekf_workspace(n) the
    calls can be captured in a graph.  For a recorded flight, filter(..., record=True) keeps what smooth(trace) reads: the
    fixed-interval (RTS) estimate of every step given the whole run, and noise_stats(trace, smooth, Z) /
    fit_noise(U, dt, Z) estimate the variances q, r from it by EM."""

    _STEP, _FILTER, _FILTER_REC = "ac_ekf_step_f32", "ac_ekf_filter_f32", "ac_ekf_filter_rec_f32"  # the entry points of the bank

    def __init__(self, system, X, P, Qd, Rd, mag_ned, ws, from_np, vec):
        self.system, self._X, self._P, self._Qd, self._Rd, self._ws = system, X, P, Qd, Rd, ws
        self.mag_ned = tuple(float(v) for v in mag_ned)
        self._np, self._vec = from_np, vec

    @property
    def n(self):
        return self._X.shape[1]

    def _give(self, t):
        if self._np:
            t = t.cpu().numpy()
            t = t.astype(np.float64) if t.dtype == np.float32 else t
        return t[..., 0] if self._vec else t

    @property
    def x(self):
        return self._give(self._X)

    @property
    def P(self):
        return self._give(self._P)

    @property
    def q(self):
        return self._give(self._Qd)

    @property
    def r(self):
        return self._give(self._Rd)

    def set_noise(self, q=None, r=None):
        """Replace the process-noise variances q ((12,) or (12, n); >= 0) and / or the measurement variances r ((15,) or (15, n);
        > 0).  Values on the host are checked (those of tensors already on a device are not read)."""
        torch = _torch_mod()
        new = {}
        for a, rows, name in ((q, 12, "q"), (r, _lib.EKF_ROWS, "r")):
            if a is None:
                continue
            shp = tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)
            if shp not in ((rows,), (rows, self.n)):
                raise ValueError(f"ekf: {name} must have shape ({rows},) or ({rows}, {self.n}), got {shp}")
            if not (isinstance(a, torch.Tensor) and a.is_cuda):
                v = a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
                if not np.isfinite(v).all() or (v < 0).any() or (name == "r" and (v <= 0).any()):
                    raise ValueError("ekf: q must be finite and >= 0" if name == "q" else "ekf: r must be finite and > 0")
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
            new[name] = t.to(device=self._X.device, dtype=torch.float32).reshape(rows, -1).expand(rows, self.n).contiguous().clone()
        self._Qd, self._Rd = new.get("q", self._Qd), new.get("r", self._Rd)

    def _opts(self, predict):
        o = _lib.EkfOpts()
        o.mag_ned[:] = self.mag_ned
        o.predict = int(predict)
        return o

    def _rows(self, a, lead, rows, name, dtype=None):
        """-> contiguous device tensor (*lead, rows, n) (rows None: (*lead, n))"""
        torch = _torch_mod()
        dtype = dtype or torch.float32
        want = tuple(lead) + (() if rows is None else (rows,)) + (self.n,)
        if not isinstance(a, torch.Tensor):
            a = np.asarray(a)
            if self._vec and a.shape == want[:-1]:
                a = a[..., None]
            if a.shape != want:
                raise ValueError(f"ekf: {name} must have shape {want}, got {a.shape}")
            a = torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32 if dtype == torch.int32 else np.float32))
        else:
            if self._vec and tuple(a.shape) == want[:-1]:
                a = a.unsqueeze(-1)
            if tuple(a.shape) != want:
                raise ValueError(f"ekf: {name} must have shape {want}, got {tuple(a.shape)}")
        return a.to(device=self._X.device, dtype=dtype).contiguous()

    @staticmethod
    def _dt(dt, predict):
        if not predict:
            return 0.0
        if isinstance(dt, bool) or np.ndim(dt) != 0 or not np.isfinite(float(dt)) or float(dt) <= 0:
            raise ValueError(f"ekf: dt must be a finite scalar > 0, got {dt!r}")
        return float(dt)

    def _one(self, u, dt, z, mask, predict):
        torch = _torch_mod()
        dt = self._dt(dt, predict)
        Z = self._rows(z, (), _lib.EKF_ROWS, "z")
        U = self._rows(u, (), _lib.NUM_CONTROLS, "u") if predict else None
        M = None if mask is None else self._rows(mask, (), None, "mask", torch.int32)
        sysm, n, dev = self.system, self.n, self._X.device
        lib = sysm._sync()
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        Xo, Po = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)
        nu, S = torch.empty((_lib.EKF_ROWS, n), **f32), torch.empty((_lib.EKF_ROWS, n), **f32)
        nis, ll = torch.empty((n,), **f32), torch.empty((n,), **f32)
        used, st = torch.empty((n,), **i32), torch.empty((n,), **i32)
        o = self._opts(predict)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(getattr(lib, self._STEP)(sysm._handle, C.byref(o), self._X.data_ptr(), self._P.data_ptr(), ptr(U), C.c_float(dt),
                                            Z.data_ptr(), ptr(M), self._Qd.data_ptr(), self._Rd.data_ptr(), n, Xo.data_ptr(), Po.data_ptr(),
                                            nu.data_ptr(), S.data_ptr(), nis.data_ptr(), ll.data_ptr(), used.data_ptr(), st.data_ptr(),
                                            None, None, None, self._ws.data_ptr(), self._ws.numel(), sysm._stream()), self._STEP)
        self._X, self._P = Xo, Po
        return EkfTrace(*(self._give(t) for t in (Xo, Po, nu, S, nis, ll, used, st)))

    def step(self, u, dt, z, mask=None) -> EkfTrace:
        """Time update over one step of length dt under the controls u (7, n), then the measurement update with z (15, n)."""
        return self._one(u, dt, z, mask, True)

    def update(self, z, mask=None) -> EkfTrace:
        """The measurement update alone, at the current estimate."""
        return self._one(None, 0.0, z, mask, False)

    def filter(self, U, dt, Z, mask=None, record=False) -> EkfTrace:
        """T steps: U (T, 7, n), Z (T, 15, n), mask (T, n) or None -> the per-step EkfTrace (leading axis T; ll (n,) summed).
        record=True: the trace also carries Xpred, Ppred, Abar of every step and the starting X0, P0 (what smooth reads)."""
        dt, T, Zt, Ut, M = self._filter_args(U, dt, Z, mask)
        return EkfTrace(*(self._give(t) for t in self._filter(Ut, dt, Zt, M, T, record)))

    def _filter_args(self, U, dt, Z, mask):
        torch = _torch_mod()
        dt = self._dt(dt, True)
        shape = tuple(Z.shape) if isinstance(Z, torch.Tensor) else np.shape(Z)
        if len(shape) < 2:
            raise ValueError(f"ekf: Z must have shape (T, 15, n), got {shape}")
        T = shape[0]
        Zt = self._rows(Z, (T,), _lib.EKF_ROWS, "Z")
        Ut = self._rows(U, (T,), _lib.NUM_CONTROLS, "U")
        M = None if mask is None else self._rows(mask, (T,), None, "mask", torch.int32)
        return dt, T, Zt, Ut, M

    def _filter(self, Ut, dt, Zt, M, T, record):
        """the device tensors of EkfTrace's fields, in order"""
        torch = _torch_mod()
        sysm, n, dev = self.system, self.n, self._X.device
        lib = sysm._sync()
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        Xo, Po, ll = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32), torch.zeros((n,), **f32)
        Xs, Ps = torch.empty((T, 13, n), **f32), torch.empty((T, 12, 12, n), **f32)
        nu, S = torch.empty((T, _lib.EKF_ROWS, n), **f32), torch.empty((T, _lib.EKF_ROWS, n), **f32)
        nis, used, st = torch.empty((T, n), **f32), torch.empty((T, n), **i32), torch.empty((T, n), **i32)
        o = self._opts(True)
        head = (sysm._handle, C.byref(o), self._X.data_ptr(), self._P.data_ptr(), Ut.data_ptr(), C.c_float(dt), Zt.data_ptr(),
                None if M is None else M.data_ptr(), self._Qd.data_ptr(), self._Rd.data_ptr(), n, T, Xo.data_ptr(), Po.data_ptr(),
                ll.data_ptr(), Xs.data_ptr(), Ps.data_ptr(), nu.data_ptr(), S.data_ptr(), nis.data_ptr(), used.data_ptr(), st.data_ptr())
        tail = (self._ws.data_ptr(), self._ws.numel(), sysm._stream())
        rec = ()
        if record:
            rec = (torch.empty((T, 13, n), **f32), torch.empty((T, 12, 12, n), **f32), torch.empty((T, 12, 12, n), **f32), self._X, self._P)
            _lib.check(getattr(lib, self._FILTER_REC)(*head, *(t.data_ptr() for t in rec[:3]), *tail), self._FILTER_REC)
        else:
            _lib.check(getattr(lib, self._FILTER)(*head, *tail), self._FILTER)
        if T:
            self._X, self._P = Xo, Po
        return (Xs, Ps, nu, S, nis, ll, used, st) + rec

    def smooth(self, trace, initial=True, gains=False) -> EkfSmooth:
        """The fixed-interval (RTS) smoother over a recorded run, trace = filter(..., record=True): every node's estimate given
        the whole run, in one backward sweep on the device.  initial: also smooth the estimate the run started from (trace.X0,
        trace.P0); gains: also return the smoother gains C.  -> EkfSmooth."""
        torch = _torch_mod()
        if not isinstance(trace, EkfTrace):
            raise ValueError("ekf smooth: expected the EkfTrace of filter(..., record=True)")
        need = ("X", "P", "Xpred", "Ppred", "Abar") + (("X0", "P0") if initial else ())
        missing = [k for k in need if getattr(trace, k) is None]
        if missing:
            raise ValueError(f"ekf smooth: the trace carries no {', '.join(missing)}: run filter(..., record=True)")
        shape = tuple(trace.X.shape) if isinstance(trace.X, torch.Tensor) else np.shape(trace.X)
        if len(shape) != (2 if self._vec else 3):
            raise ValueError(f"ekf smooth: trace.X must have shape (T, 13, n), got {shape}")
        T = shape[0]
        Xf, Xp = (self._rows(getattr(trace, k), (T,), 13, f"trace.{k}") for k in ("X", "Xpred"))
        Pf, Pp, Ab = (self._rows(getattr(trace, k), (T, 12), 12, f"trace.{k}") for k in ("P", "Ppred", "Abar"))
        X0 = self._rows(trace.X0, (), 13, "trace.X0") if initial else None
        P0 = self._rows(trace.P0, (12,), 12, "trace.P0") if initial else None
        return EkfSmooth(*(None if t is None else self._give(t) for t in self._smooth(X0, P0, Xf, Pf, Xp, Pp, Ab, T, gains)))

    def _smooth(self, X0, P0, Xf, Pf, Xp, Pp, Ab, T, gains):
        """the device tensors of EkfSmooth's fields, in order"""
        torch = _torch_mod()
        initial = X0 is not None
        sysm, n, dev = self.system, self.n, self._X.device
        lib = sysm._sync()
        f32 = dict(device=dev, dtype=torch.float32)
        Xs, Ps = torch.empty((T, 13, n), **f32), torch.empty((T, 12, 12, n), **f32)
        Xs0, Ps0 = (torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)) if initial else (None, None)
        Cg = torch.empty((T, 12, 12, n), **f32) if gains else None
        st = torch.empty((T, n), device=dev, dtype=torch.int32)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.ac_ekf_smooth_f32(sysm._handle, ptr(X0), ptr(P0), Xf.data_ptr(), Pf.data_ptr(), Xp.data_ptr(), Pp.data_ptr(),
                                         Ab.data_ptr(), n, T, Xs.data_ptr(), Ps.data_ptr(), ptr(Xs0), ptr(Ps0), ptr(Cg), st.data_ptr(),
                                         sysm._stream()), "ac_ekf_smooth_f32")
        return Xs, Ps, Xs0, Ps0, Cg, st

    # ---- MAP trajectory by Gauss-Newton (include/aircraft_hip.h, ac_ieks_solve_f32) -----------------------
    @staticmethod
    def _ladder(ladder):
        try:
            lad = [float(v) for v in ladder]
        except (TypeError, ValueError):
            raise ValueError(f"ekf map_smooth: ladder must be a sequence of numbers, got {ladder!r}") from None
        if not 1 <= len(lad) <= _lib.IEKS_MAX_CANDIDATES or not all(np.isfinite(v) and 0 < v <= 1 for v in lad) \
                or any(b >= a for a, b in zip(lad, lad[1:])):
            raise ValueError(f"ekf map_smooth: ladder must be 1 .. {_lib.IEKS_MAX_CANDIDATES} decreasing values in (0, 1], got {ladder!r}")
        return lad

    def map_smooth(self, U, dt, Z, mask=None, iters=5, init=None, ladder=(1, .5, .25, .125)) -> EkfMapSmooth:
        """The maximum-a-posteriori trajectory of a log U (T, 7, n), Z (T, 15, n), mask (T, n) or None, by `iters` Gauss-Newton
        iterations (the iterated extended Kalman smoother): linearise about a nominal trajectory, one affine filter pass and
        one RTS sweep, then a line search on the MAP cost over the `ladder` of step lengths.  The bank's (x, P) is the prior of
        the initial node and is NOT advanced; for a moving horizon slide the window and advance the bank with filter.
        init: the nominal to start from: None, the bank's own filter(record=True) + smooth on a copy of its state; an array
        (T + 1, 13, n) (the initial node first); an EkfSmooth with X0; or "rollout", the open-loop rollout of x under U.
        No host synchronisation.  -> EkfMapSmooth."""
        torch = _torch_mod()
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
            raise ValueError(f"ekf map_smooth: iters must be an integer >= 0, got {iters!r}")
        lad = self._ladder(ladder)
        shape = tuple(Z.shape) if isinstance(Z, torch.Tensor) else np.shape(Z)
        if len(shape) != (2 if self._vec else 3) or shape[0] < 1:
            raise ValueError(f"ekf map_smooth: Z must have shape (T, 15, n) with T >= 1, got {shape}")
        T = shape[0]
        if isinstance(init, str):
            if init != "rollout":
                raise ValueError(f"ekf map_smooth: init must be None, 'rollout', an array (T + 1, 13, n) or an EkfSmooth, got {init!r}")
        elif isinstance(init, EkfSmooth):
            if init.X is None or init.X0 is None:
                raise ValueError("ekf map_smooth: the EkfSmooth carries no X0: run smooth(trace, initial=True)")
        elif isinstance(init, EkfTrace):
            raise ValueError("ekf map_smooth: init takes the EkfSmooth of smooth(trace), not the trace")
        dt, T, Zt, Ut, M = self._filter_args(U, dt, Z, mask)
        if isinstance(init, EkfSmooth):
            Xb = torch.cat([self._rows(init.X0, (), 13, "init.X0").unsqueeze(0), self._rows(init.X, (T,), 13, "init.X")]).contiguous()
        elif init is not None and not isinstance(init, str):
            Xb = self._rows(init, (T + 1,), 13, "init").clone()

        # ---- device side ----
        sysm, n, dev = self.system, self.n, self._X.device
        X0, P0 = self._X, self._P
        if init is None:
            tr = self._filter(Ut, dt, Zt, M, T, True)
            self._X, self._P = X0, P0
            sm = self._smooth(X0, P0, tr[0], tr[1], tr[8], tr[9], tr[10], T, False)
            Xb = torch.cat([sm[2].unsqueeze(0), sm[0]]).contiguous()
        elif isinstance(init, str):
            Xb = sysm.rollout(X0, Ut, dt).contiguous().clone()
        lib = sysm._sync()
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        e = lambda *s: torch.empty(s, **f32)  # noqa: E731
        Xs, Ps, Xs0, Ps0, Xf, Pf = e(T, 13, n), e(T, 12, 12, n), e(13, n), e(12, 12, n), e(T, 13, n), e(T, 12, 12, n)
        ll, nu, S, nis = e(n), e(T, _lib.EKF_ROWS, n), e(T, _lib.EKF_ROWS, n), e(T, n)
        used, fst, st = torch.empty((T, n), **i32), torch.empty((T, n), **i32), torch.empty((n,), **i32)
        Xp, Pp, Ab = e(T, 13, n), e(T, 12, 12, n), e(T, 12, 12, n)
        cost, alpha = e(int(iters) + 1, n), e(int(iters), n)
        ws = sysm.ieks_workspace(n, T, len(lad))
        o = EKF._opts(self, True)
        cl = (C.c_float * len(lad))(*lad)
        _lib.check(lib.ac_ieks_solve_f32(sysm._handle, C.byref(o), X0.data_ptr(), P0.data_ptr(), Xb.data_ptr(), Ut.data_ptr(), C.c_float(dt),
                                         Zt.data_ptr(), None if M is None else M.data_ptr(), self._Qd.data_ptr(), self._Rd.data_ptr(), n, T,
                                         int(iters), cl, len(lad), *(t.data_ptr() for t in (Xs, Ps, Xs0, Ps0, Xf, Pf, ll, nu, S, nis, used, fst,
                                                                                           Xp, Pp, Ab, cost, alpha, st)),
                                         ws.data_ptr(), ws.numel(), sysm._stream()), "ac_ieks_solve_f32")
        g = self._give
        trace = EkfTrace(*(g(t) for t in (Xf, Pf, nu, S, nis, ll, used, fst, Xp, Pp, Ab, X0, P0)))
        return EkfMapSmooth(g(Xs), g(Ps), g(Xs0), g(Ps0), g(cost), g(alpha), g(st), trace, g(Xb))

    # ---- EM estimate of q and r (include/aircraft_hip.h, ac_ekf_em_f32) ---------------------------------
    @staticmethod
    def _floor(floor):
        if isinstance(floor, bool) or np.ndim(floor) != 0 or not np.isfinite(float(floor)) or float(floor) < 0:
            raise ValueError(f"ekf: floor must be a finite scalar >= 0, got {floor!r}")
        return float(floor)

    def noise_stats(self, trace, smooth, Z, floor=1e-4) -> EkfNoiseStats:
        """The M-step of an EM estimate of q and r from trace = filter(U, dt, Z, mask, record=True), made with the bank's present
        q, r, and smooth = smooth(trace): one launch pair over (instances) x (chunks of 32 nodes).  floor: the new variances are
        at least floor x the present ones (0 means 1e-4).  -> EkfNoiseStats; the bank's q, r are not changed (set_noise)."""
        torch = _torch_mod()
        floor = self._floor(floor)
        if not isinstance(trace, EkfTrace) or not isinstance(smooth, EkfSmooth):
            raise ValueError("ekf noise_stats: expected the EkfTrace of filter(..., record=True) and the EkfSmooth of smooth(trace)")
        missing = [f"trace.{k}" for k in ("Xpred", "Ppred", "used") if getattr(trace, k) is None]
        missing += [f"smooth.{k}" for k in ("X", "P") if getattr(smooth, k) is None]
        if missing:
            raise ValueError(f"ekf noise_stats: {', '.join(missing)} missing: run filter(..., record=True) and smooth(trace)")
        shape = tuple(Z.shape) if isinstance(Z, torch.Tensor) else np.shape(Z)
        if len(shape) != (2 if self._vec else 3):
            raise ValueError(f"ekf noise_stats: Z must have shape (T, 15, n), got {shape}")
        T = shape[0]
        Zt = self._rows(Z, (T,), _lib.EKF_ROWS, "Z")
        Xp, Xs = self._rows(trace.Xpred, (T,), 13, "trace.Xpred"), self._rows(smooth.X, (T,), 13, "smooth.X")
        Pp, Ps = self._rows(trace.Ppred, (T, 12), 12, "trace.Ppred"), self._rows(smooth.P, (T, 12), 12, "smooth.P")
        used = self._rows(trace.used, (T,), None, "trace.used", torch.int32)
        return EkfNoiseStats(*(self._give(t) for t in self._noise_stats(Xp, Pp, Xs, Ps, Zt, used, T, floor)))

    def _noise_stats(self, Xp, Pp, Xs, Ps, Zt, used, T, floor, ws=None):
        """the device tensors of EkfNoiseStats' fields, in order"""
        torch = _torch_mod()
        sysm, n, dev = self.system, self.n, self._X.device
        lib = sysm._sync()
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        if ws is None:
            ws = sysm.ekf_em_workspace(n, T)
        Qsum, Rsum, Qn, Rn = (torch.empty((rows, n), **f32) for rows in (12, _lib.EKF_ROWS, 12, _lib.EKF_ROWS))
        nq, nr, st = torch.empty((n,), **i32), torch.empty((_lib.EKF_ROWS, n), **i32), torch.empty((T, n), **i32)
        o = _lib.EkfEmOpts()
        o.mag_ned[:] = self.mag_ned
        o.floor_rel = floor
        _lib.check(lib.ac_ekf_em_f32(sysm._handle, C.byref(o), Xp.data_ptr(), Pp.data_ptr(), Xs.data_ptr(), Ps.data_ptr(), Zt.data_ptr(),
                                     used.data_ptr(), self._Qd.data_ptr(), self._Rd.data_ptr(), n, T, Qsum.data_ptr(), Rsum.data_ptr(),
                                     nq.data_ptr(), nr.data_ptr(), st.data_ptr(), Qn.data_ptr(), Rn.data_ptr(), ws.data_ptr(), ws.numel(),
                                     sysm._stream()), "ac_ekf_em_f32")
        return Qsum, Rsum, nq, nr, Qn, Rn, st

    def fit_noise(self, U, dt, Z, mask=None, iters=10, update=("q", "r"), share=False, floor=1e-4) -> EkfNoiseFit:
        """EM for the variances over a recorded flight U (T, 7, n), Z (T, 15, n), mask (T, n) or None.  Each of the `iters`
        iterations starts from the estimate the bank holds now: filter(record=True), smooth(initial=False), noise_stats,
        set_noise of the rows named in `update`.  share=True: one airframe, many logs: sums and counts are pooled over the
        instances (a float64 sum) before dividing, so every instance gets the same q, r (the floor is then floor x the mean of the
        present variances).  On return x, P are what they were, q, r are the fitted ones.  No host synchronisation before
        the result is handed out.  -> EkfNoiseFit."""
        torch = _torch_mod()
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
            raise ValueError(f"ekf fit_noise: iters must be an integer >= 1, got {iters!r}")
        if isinstance(update, str) or not set(update) <= {"q", "r"}:
            raise ValueError(f"ekf fit_noise: update names 'q' and / or 'r', got {update!r}")
        floor = self._floor(floor)
        dt, T, Zt, Ut, M = self._filter_args(U, dt, Z, mask)
        X0, P0 = self._X, self._P
        ws = self.system.ekf_em_workspace(self.n, T)
        lls, st = [], None
        for _ in range(int(iters)):
            self._X, self._P = X0, P0
            tr = self._filter(Ut, dt, Zt, M, T, True)
            lls.append(tr[5])
            sm = self._smooth(None, None, tr[0], tr[1], tr[8], tr[9], tr[10], T, False)
            st = self._noise_stats(tr[8], tr[9], sm[0], sm[1], Zt, tr[6], T, floor, ws)
            qn, rn = st[4], st[5]
            if share:
                lo = (floor if floor > 0 else 1e-4)
                pool = lambda s, c, old: torch.where(c.sum(-1, keepdim=True) > 0, torch.maximum(  # noqa: E731
                    s.double().sum(-1, keepdim=True) / c.sum(-1, keepdim=True).clamp(min=1), lo * old.double().mean(-1, keepdim=True)),
                    old.double()).float().expand(-1, self.n).contiguous()
                qn = pool(st[0], st[2].reshape(1, -1).expand(12, -1), self._Qd)
                rn = pool(st[1], st[3], self._Rd)
            if "q" in update:
                self._Qd = qn
            if "r" in update:
                self._Rd = rn
        self._X, self._P = X0, P0
        lls.append(self._filter(Ut, dt, Zt, M, T, False)[5])
        self._X, self._P = X0, P0
        return EkfNoiseFit(*(self._give(t) for t in (self._Qd, self._Rd, torch.stack(lls), st[2], st[3], st[6])))


class UKF(EKF):
    """A bank of n unscented Kalman filters (Aircraft.ukf): EKF's interface over sigma points in place of
    Jacobians (include/aircraft_hip.h, ac_ukf_step_f32).  step / update / filter return an EkfTrace whose status may also carry
    bit 3 (value 4): the covariance or its prediction had no Cholesky factor.  filter(..., record=True) records the statistical
    linearisation as Abar, so smooth(trace) is the unscented RTS smoother.  noise_stats / fit_noise are not defined here: the
    EM statistic's innovations form assumes P- = Abar P Abar' + Q exactly, which the sigma-point P- does not satisfy."""

    _STEP, _FILTER, _FILTER_REC = "ac_ukf_step_f32", "ac_ukf_filter_f32", "ac_ukf_filter_rec_f32"

    def __init__(self, *args, kappa=0.0):
        super().__init__(*args)
        self.kappa = float(kappa)

    def _opts(self, predict):
        o = _lib.UkfOpts()
        o.mag_ned[:] = self.mag_ned
        o.predict = int(predict)
        o.kappa = self.kappa
        return o

    def noise_stats(self, *args, **kwargs):
        raise NotImplementedError("ukf: the EM noise statistics assume the EKF's P- = Abar P Abar' + Q; use Aircraft.ekf for them")

    def fit_noise(self, *args, **kwargs):
        raise NotImplementedError("ukf: the EM noise fit assumes the EKF's P- = Abar P Abar' + Q; use Aircraft.ekf for it")


EKF_MAG_NED = (0.45, 0.03, 0.89)  # a northern mid-latitude field direction (north, east, down), the default of mag_ned


@dataclass
class SensorModel:
    """The simulated sensors of Aircraft.sense and the output-feedback rollouts (include/aircraft_hip.h, ac_sense_f32; DESIGN.md
    §4.19).  sigma (15,) or (15, n): the standard deviation of every measurement row (finite, >= 0; checked for values on the
    host, those of a tensor already on a device are not read, as in Aircraft.ekf).  The five sensor groups (GPS
    position, GPS velocity, gyro, air data, magnetometer; three rows each) report at the steps with (step - phase[j]) % period[j]
    == 0 and are then dropped with probability dropout[j] in [0, 1).  seed: a 64-bit integer; the draw of a row depends on (seed,
    step, instance_offset + i, row) alone, so a sharded batch draws what the whole batch would."""
    sigma: Any
    period: Any = (1, 1, 1, 1, 1)
    phase: Any = (0, 0, 0, 0, 0)
    dropout: Any = (0.0, 0.0, 0.0, 0.0, 0.0)
    seed: int = 0
    mag_ned: Any = EKF_MAG_NED
    instance_offset: int = 0

    def __post_init__(self):
        torch = _torch_mod()
        g = _lib.LQG_GROUPS
        if isinstance(self.sigma, torch.Tensor):
            shp = tuple(self.sigma.shape)
            sv = None if self.sigma.is_cuda else self.sigma.detach().numpy().astype(np.float64)
        else:
            sv = self.sigma = np.asarray(self.sigma, dtype=np.float64)
            shp = self.sigma.shape
        if sv is not None and (not np.isfinite(sv).all() or (sv < 0).any()):
            raise ValueError("sensors: sigma must be finite and >= 0")
        if len(shp) not in (1, 2) or shp[0] != _lib.EKF_ROWS:
            raise ValueError(f"sensors: sigma must have shape (15,) or (15, n), got {shp}")
        for name in ("period", "phase"):
            v = np.asarray(getattr(self, name))
            if v.shape != (g,) or v.dtype.kind not in "iu" or np.abs(v).max() >= 2 ** 31:
                raise ValueError(f"sensors: {name} must be {g} integers, got {getattr(self, name)!r}")
            setattr(self, name, tuple(int(x) for x in v))
        if min(self.period) < 1:
            raise ValueError("sensors: every period must be >= 1")
        d = np.asarray(self.dropout, dtype=np.float64)
        if d.shape != (g,) or not ((d >= 0) & (d < 1)).all():
            raise ValueError("sensors: dropout must be 5 probabilities in [0, 1)")
        self.dropout = tuple(float(x) for x in d)
        if isinstance(self.seed, bool) or not isinstance(self.seed, (int, np.integer)) or not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"sensors: seed must be an integer in [0, 2^64), got {self.seed!r}")
        if isinstance(self.instance_offset, bool) or not isinstance(self.instance_offset, (int, np.integer)) or not 0 <= int(self.instance_offset) < 2 ** 63:
            raise ValueError(f"sensors: instance_offset must be an integer >= 0, got {self.instance_offset!r}")
        mg = np.asarray(self.mag_ned, dtype=np.float64)
        if mg.shape != (3,) or not np.isfinite(mg).all():
            raise ValueError("sensors: mag_ned must be 3 finite numbers")
        self.mag_ned = tuple(float(x) for x in mg)

    def _opts(self):
        o = _lib.SenseOpts()
        o.mag_ned[:] = self.mag_ned
        o.seed_lo, o.seed_hi = int(self.seed) & 0xFFFFFFFF, int(self.seed) >> 32
        o.instance_offset = int(self.instance_offset)
        o.period[:], o.phase[:], o.dropout[:] = self.period, self.phase, self.dropout
        return o

    def _sigma(self, n, dev):
        torch = _torch_mod()
        s = self.sigma if isinstance(self.sigma, torch.Tensor) else torch.as_tensor(np.asarray(self.sigma, dtype=np.float32))
        if s.dim() == 2 and s.shape[1] != n:
            raise ValueError(f"sensors: sigma must have shape (15,) or (15, {n}), got {tuple(s.shape)}")
        return s.to(device=dev, dtype=torch.float32).reshape(_lib.EKF_ROWS, -1).expand(_lib.EKF_ROWS, n).contiguous()


@dataclass
class LqgResult:
    """What the output-feedback rollouts return for n instances and T steps (numpy in -> numpy out; tensors stay on the device;
    include/aircraft_hip.h, ac_lqg_rollout_f32).  X, Xhat (T+1, 13, n): the truth and the estimate, node 0 the
    starting ones; U (T, 7, n): the controls applied; Z (T, 15, n), mask (T, n): what the sensors reported after each step (NaN
    and a cleared bit for a row that did not report); nis (T, n), used (T, n), status (T, n): the estimator's own (EkfTrace);
    nees (T, n) = e' P^-1 e and err (T, 12, n) = x [-] x^ in the error coordinates, NaN nees where P had no Cholesky factor; P
    (T, 12, 12, n) when recorded (record=("P",)), else None; Xnom (T+1, 13, n): the nominal the law tracked."""
    X: Any
    Xhat: Any
    U: Any
    Z: Any
    mask: Any
    nis: Any
    nees: Any
    err: Any
    used: Any
    status: Any
    Xnom: Any
    P: Any = None


def inertia_about_com(cfg_Ixx, cfg_Iyy, cfg_Izz, cfg_Ixz, mass, com):
    """I = I0 + m K(com)   (reference dynamics/aircraft.py:137-141, 168-187), float64."""
    x, y, z = (float(c) for c in com)
    I0 = np.array([[cfg_Ixx, 0.0, cfg_Ixz], [0.0, cfg_Iyy, 0.0], [cfg_Ixz, 0.0, cfg_Izz]], dtype=np.float64)
    K = np.array([[y * y + z * z, -x * y, -x * z], [-y * x, x * x + z * z, -y * z], [-z * x, -z * y, x * x + y * y]],
                 dtype=np.float64)
    return I0 + float(mass) * K


class Aircraft(SixDOF):
    num_controls = _lib.NUM_CONTROLS

    def __init__(self, opts: AircraftOpts, **kwargs):
        super().__init__(opts=opts, **kwargs)
        self.opts = opts
        self.grav = self.gravity
        self.stall_scaling = opts.stall_scaling
        self.initialise_aircraft(opts.aircraft_config)
        self.coefficient_model: CoefficientModel = (
            opts.coefficient_model(self) if opts.coefficient_model else DefaultModel(self))

    def initialise_aircraft(self, config: AircraftConfiguration) -> None:
        """reference dynamics/aircraft.py:123-141"""
        self.S = config.reference_area
        self.b = config.span
        self.c = config.chord
        self.mass = config.mass
        self.com = np.asarray(config.aero_centre_offset, dtype=np.float64)
        self.rudder_moment_arm = config.rudder_moment_arm
        self.length = config.length
        self.Ixx, self.Iyy, self.Izz, self.Ixz = config.Ixx, config.Iyy, config.Izz, config.Ixz

    @property
    def inertia_tensor(self) -> np.ndarray:
        return inertia_about_com(self.Ixx, self.Iyy, self.Izz, self.Ixz, self.mass, self.com)

    @property
    def inverse_inertia_tensor(self) -> np.ndarray:
        return np.linalg.inv(self.inertia_tensor)

    @property
    def model_kind(self) -> str:
        return self.coefficient_model.kind

    def _param_struct(self) -> "_lib.AcParams":
        p = _lib.AcParams()
        p.mass, p.S, p.b, p.c = float(self.mass), float(self.S), float(self.b), float(self.c)
        I = self.inertia_tensor
        p.inertia[:] = [float(v) for v in I.ravel()]
        p.inertia_inv[:] = [float(v) for v in np.linalg.inv(I).ravel()]
        p.com[:] = [float(v) for v in np.asarray(self.com, dtype=np.float64).ravel()]
        p.rudder_moment_arm = float(self.rudder_moment_arm)
        p.epsilon = float(self.epsilon)
        p.gravity[:] = [float(g) for g in self.gravity]
        ns = self.physical_integration_substeps
        p.substeps = int(self.opts.physical_integration_substeps if ns is None else ns)
        p.normalise = int(bool(self.normalise))
        p.stall_scaling = int(bool(self.stall_scaling))
        p.model_kind = _lib.MODEL_KINDS[self.coefficient_model.kind]
        return p

    def _install_model(self) -> None:
        self.coefficient_model.install(self._handle)

    # ---- flight envelope (reference control/aircraft.py:44-59) ------------------------------------------------------
    ENVELOPE_BOUNDS = ((20.0 ** 2, 100.0 ** 2), (-float(np.deg2rad(10)), float(np.deg2rad(10))),
                       (-float(np.deg2rad(20)), float(np.deg2rad(20))), (-float("inf"), 0.0))

    def envelope(self, x, want_jacobian: bool = True):
        """Rows of AircraftControl.state_constraint for a column batch x (13, n): rows (4, n) = (|v_rel|^2, beta, alpha, z),
        bounded by ENVELOPE_BOUNDS, and their state Jacobian Jx (4, 13, n) (None if not wanted)."""
        torch = _torch_mod()
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        n = X.shape[1]
        rows = torch.empty((4, n), device=X.device, dtype=torch.float32)
        Jx = torch.empty((4, 13, n), device=X.device, dtype=torch.float32) if want_jacobian else None
        _lib.check(lib.ac_envelope_f32(self._handle, X.data_ptr(), n, rows.data_ptr(),
                                       Jx.data_ptr() if Jx is not None else None, self._stream()), "ac_envelope_f32")
        if npx:
            rows = rows.cpu().numpy().astype(np.float64)
            Jx = None if Jx is None else Jx.cpu().numpy().astype(np.float64)
        if vec:
            rows = rows[..., 0]
            Jx = None if Jx is None else Jx[..., 0]
        return rows, Jx

    # ---- steady-flight trim (include/aircraft_hip.h, ac_trim_f32) -------------------------------------
    def trim_bounds(self, lateral: int = 0):
        """Default bounds (lo (6,), hi (6,)) of z: alpha +-20 deg and beta +-10 deg (the envelope, control/aircraft.py:53-58),
        theta +-60 deg, phi +-80 deg (rad), the surfaces +-10 deg (problem_definition.json:32-34)."""
        d = np.deg2rad
        hi = np.array([d(20.0), d(60.0), d(80.0), 10.0, 10.0, d(10.0) if lateral else 10.0])
        return -hi, hi

    def trim_workspace(self, n: int):
        """Device workspace of a trim of n instances (ac_trim_workspace_floats); allocate it before capturing a graph."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_trim_workspace_floats(self._handle, int(n), C.byref(need)), "ac_trim_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def trim(self, airspeed, *, psi=0.0, turn_rate=0.0, beta=0.0, rudder=None, position=(0.0, 0.0, -200.0), thrust=0.0,
             flaps=0.0, guess=None, bounds=None, iters=30, tol=(1e-4, 1e-4), ws=None) -> TrimResult:
        """Steady flight for n instances: z = (alpha, theta, phi, aileron, elevator, rudder | beta) such that body velocity
        and body rates stay constant at airspeed V, heading psi, turn rate psid (rad/s about NED down; 0 = straight).
        beta (rad) is held and the rudder solved for; passing `rudder` (deg) holds it and solves for beta instead.
        Per-instance arguments are scalars or (n,); position (3,) or (3, n); thrust a scalar, (3,) or (3, n); flaps a scalar
        or (n,); guess (6,) or (6, n); bounds (lo (6,), hi (6,)) (default trim_bounds()); tol (tol_v, tol_w).
        Default guess: alpha 4 deg, theta = alpha + the glide angle -atan(1 / glide_ratio), phi = atan(V psid / g), surfaces 0.
        `iters` Levenberg-Marquardt iterations, each three kernel launches; no host synchronisation (graph-capturable with a
        workspace `ws` from trim_workspace(n))."""
        torch = _torch_mod()
        lateral = 0 if rudder is None else 1
        if lateral and (isinstance(beta, torch.Tensor) or np.ndim(beta) != 0 or float(beta) != 0.0):
            raise ValueError("trim: pass beta (held sideslip, rudder solved) or rudder (held rudder, beta solved), not both")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
            raise ValueError(f"trim: iters must be an integer >= 1, got {iters!r}")
        tol = tuple(float(t) for t in np.ravel(tol))
        if len(tol) != 2 or not all(np.isfinite(t) and t > 0 for t in tol):
            raise ValueError(f"trim: tol must be two finite values > 0 (tol_v, tol_w), got {tol}")
        lo, hi = self.trim_bounds(lateral) if bounds is None else (np.asarray(b, dtype=np.float64) for b in bounds)
        if np.shape(lo) != (6,) or np.shape(hi) != (6,) or np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any():
            raise ValueError("trim: bounds must be (lo (6,), hi (6,)) with lo <= hi")
        if ws is not None and (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_cuda
                               or not ws.is_contiguous()):
            raise ValueError("trim: ws must be a contiguous float32 device tensor (trim_workspace(n))")
        lat = beta if rudder is None else rudder
        args = {"airspeed": (airspeed, None), "psi": (psi, None), "turn_rate": (turn_rate, None),
                ("rudder" if lateral else "beta"): (lat, None), "position": (position, 3), "thrust": (thrust, 3),
                "flaps": (flaps, None), "guess": (guess, 6)}

        def cols(name, a, rows):
            shp = tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)
            if rows is None and len(shp) <= 1:
                return shp[0] if shp else 1
            if rows is not None and (len(shp) == 0 and name == "thrust" or shp == (rows,)):
                return 1
            if rows is not None and len(shp) == 2 and shp[0] == rows:
                return shp[1]
            want = "a scalar or (n,)" if rows is None else f"({rows},) or ({rows}, n)"
            raise ValueError(f"trim: {name} must be {want}, got shape {shp}")

        m = {k: cols(k, a, r) for k, (a, r) in args.items() if a is not None}
        sizes = {v for v in m.values() if v != 1}
        if len(sizes) > 1:
            raise ValueError(f"trim: arguments do not broadcast to one n: {m}")
        n = sizes.pop() if sizes else 1
        tensors = any(isinstance(a, torch.Tensor) for a, _ in args.values())

        # ---- device side ----
        lib = self._sync()
        dev = self._device_obj()

        def rows_of(a, rows):
            if not isinstance(a, torch.Tensor) and np.size(a) <= rows:
                # a constant: filled on the device (no host-to-device copy, so a default argument can be graph-captured)
                v = np.asarray(a, dtype=np.float32).ravel()
                t = torch.empty((v.size, 1), device=dev, dtype=torch.float32)
                for k, e in enumerate(v):
                    t[k].fill_(float(e))
                return t.expand(rows, n)
            t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float32))
            t = t.to(device=dev, dtype=torch.float32)
            return t.reshape(rows if t.numel() != 1 else 1, -1).expand(rows, n)

        V = rows_of(airspeed, 1)
        psid = rows_of(turn_rate, 1)
        target = torch.cat([rows_of(position, 3), V, rows_of(psi, 1), psid, rows_of(lat, 1)]).contiguous()
        Uhold = torch.zeros((_lib.NUM_CONTROLS, n), device=dev, dtype=torch.float32)
        Uhold[3:6] = rows_of(thrust, 3)
        Uhold[6:7] = rows_of(flaps, 1)
        if guess is None:
            a0 = float(np.deg2rad(4.0))
            gamma0 = -float(np.arctan(1.0 / float(self.opts.aircraft_config.glide_ratio)))
            Z0 = torch.zeros((6, n), device=dev, dtype=torch.float32)
            Z0[0] = a0
            Z0[1] = a0 + gamma0
            Z0[2] = torch.atan(V[0] * psid[0] / float(self.gravity[2]))
        else:
            Z0 = rows_of(guess, 6).contiguous()
        opts = _lib.TrimOpts()
        opts.lateral = lateral
        opts.tol_v, opts.tol_w = tol
        opts.lo[:] = [float(v) for v in lo]
        opts.hi[:] = [float(v) for v in hi]
        if ws is None:
            ws = self.trim_workspace(n)
        X = torch.empty((13, n), device=dev, dtype=torch.float32)
        U = torch.empty((_lib.NUM_CONTROLS, n), device=dev, dtype=torch.float32)
        Z = torch.empty((6, n), device=dev, dtype=torch.float32)
        R = torch.empty((6, n), device=dev, dtype=torch.float32)
        S = torch.empty((n,), device=dev, dtype=torch.int32)
        _lib.check(lib.ac_trim_f32(self._handle, C.byref(opts), target.data_ptr(), Uhold.data_ptr(), Z0.data_ptr(), int(iters),
                                   n, X.data_ptr(), U.data_ptr(), Z.data_ptr(), R.data_ptr(), S.data_ptr(), ws.data_ptr(),
                                   ws.numel(), self._stream()), "ac_trim_f32")
        if not tensors:
            X, U, Z, R = (t.cpu().numpy().astype(np.float64) for t in (X, U, Z, R))
            S = S.cpu().numpy()
        return TrimResult(X, U, Z, R, S, S == 0)

    # ---- LQR about a steady-flight trim (include/aircraft_hip.h, ac_lqr_f32) ---------------------------
    LQR_Q_DEFAULT = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0)  # the eight-state stability augmentation

    def lqr_workspace(self, n: int):
        """Device workspace of an LQR design of n instances (ac_lqr_workspace_floats); allocate it before capturing a graph."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_lqr_workspace_floats(self._handle, int(n), C.byref(need)), "ac_lqr_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def lqr(self, trim_or_xu, dt, q=None, r=None, iters=24, tol=1e-6, ws=None) -> LqrResult:
        """Constant-gain discrete LQR about steady flight for n instances: `trim_or_xu` is a TrimResult or an (x (13, n),
        u (7, n)) pair.  The step of length dt is linearised in the 12 steady-flight error coordinates (steady_error), in
        which a trim is a fixed point, and P = Q + A'PA - A'PB (R + B'PB)^-1 B'PA is solved with Q = diag(q), R = diag(r).
        q (12,) >= 0: weights of (along-track, cross-track, down, body velocity (3), tilt (2), heading, body rates (3)); a 0 on
        along-track, cross-track, down or heading drops that coordinate from the design.  The default weights 1 on body
        velocity, tilt and rates only: the eight-state stability augmentation; q = 1 on 1, 2, 8 as well holds the path.
        r (7,) > 0: control weights (default 1).  `iters` doubling steps at most (an instance is frozen once its iterate
        moves by less than tol, relative); no host synchronisation (graph-capturable with a workspace from lqr_workspace(n))."""
        torch = _torch_mod()
        if isinstance(trim_or_xu, TrimResult):
            x, u = trim_or_xu.x, trim_or_xu.u
        elif isinstance(trim_or_xu, (tuple, list)) and len(trim_or_xu) == 2:
            x, u = trim_or_xu
        else:
            raise ValueError("lqr: pass a TrimResult or an (x, u) pair")
        shp = lambda a: tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)  # noqa: E731
        sx, su = shp(x), shp(u)
        if len(sx) not in (1, 2) or sx[0] != 13 or len(su) != len(sx) or su[0] != _lib.NUM_CONTROLS or sx[1:] != su[1:]:
            raise ValueError(f"lqr: expected x (13, n) and u (7, n), got {sx} and {su}")
        if isinstance(dt, bool) or np.ndim(dt) != 0 or not np.isfinite(float(dt)) or float(dt) <= 0:
            raise ValueError(f"lqr: dt must be a finite scalar > 0, got {dt!r}")
        if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 1:
            raise ValueError(f"lqr: iters must be an integer >= 1, got {iters!r}")
        if np.ndim(tol) != 0 or not np.isfinite(float(tol)) or float(tol) < 0:
            raise ValueError(f"lqr: tol must be a finite scalar >= 0, got {tol!r}")
        qv = np.asarray(self.LQR_Q_DEFAULT if q is None else q, dtype=np.float64)
        rv = np.ones(_lib.NUM_CONTROLS) if r is None else np.asarray(r, dtype=np.float64)
        if qv.shape != (12,) or not np.isfinite(qv).all() or (qv < 0).any():
            raise ValueError("lqr: q must be 12 finite weights >= 0")
        if rv.shape != (_lib.NUM_CONTROLS,) or not np.isfinite(rv).all() or (rv <= 0).any():
            raise ValueError("lqr: r must be 7 finite weights > 0")
        if ws is not None and (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_cuda
                               or not ws.is_contiguous()):
            raise ValueError("lqr: ws must be a contiguous float32 device tensor (lqr_workspace(n))")

        # ---- device side ----
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in(u, _lib.NUM_CONTROLS, "u")
        n = X.shape[1]
        dev = X.device
        opts = _lib.LqrOpts()
        opts.q[:] = [float(v) for v in qv]
        opts.r[:] = [float(v) for v in rv]
        opts.tol = float(tol)
        if ws is None:
            ws = self.lqr_workspace(n)
        f32 = dict(device=dev, dtype=torch.float32)
        A, Bm = torch.empty((12, 12, n), **f32), torch.empty((12, 7, n), **f32)
        P, K = torch.empty((12, 12, n), **f32), torch.empty((7, 12, n), **f32)
        res = torch.empty((n,), **f32)
        S, it = torch.empty((n,), device=dev, dtype=torch.int32), torch.empty((n,), device=dev, dtype=torch.int32)
        _lib.check(lib.ac_lqr_f32(self._handle, C.byref(opts), X.data_ptr(), U.data_ptr(), C.c_float(float(dt)), int(iters), n,
                                  A.data_ptr(), Bm.data_ptr(), P.data_ptr(), K.data_ptr(), res.data_ptr(), S.data_ptr(),
                                  it.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), "ac_lqr_f32")
        if npx:
            K, P, A, Bm, X, U, res = (t.cpu().numpy().astype(np.float64) for t in (K, P, A, Bm, X, U, res))
            S, it = S.cpu().numpy(), it.cpu().numpy()
        if vec:
            K, P, A, Bm, X, U, res, S, it = (t[..., 0] for t in (K, P, A, Bm, X, U, res, S, it))
        return LqrResult(K, P, A, Bm, X, U, res, S, S == 0, it, float(dt), qv, rv, self)

    def _lqr_gains(self, Xnom, K):
        torch = _torch_mod()
        lib = self._sync()
        dev = self._device_obj()
        from_np = not isinstance(Xnom, torch.Tensor)
        Xt = torch.as_tensor(np.asarray(Xnom, dtype=np.float32) if from_np else Xnom).to(device=dev, dtype=torch.float32)
        Kt = torch.as_tensor(np.asarray(K, dtype=np.float32) if not isinstance(K, torch.Tensor) else K).to(device=dev, dtype=torch.float32)
        vec = Xt.dim() == 2
        if vec:
            Xt, Kt = Xt.unsqueeze(-1), Kt.unsqueeze(-1)
        if Xt.dim() != 3 or Xt.shape[0] < 1 or Xt.shape[1] != 13 or tuple(Kt.shape) != (7, 12, Xt.shape[2]):
            raise ValueError(f"gains: expected Xnom (H+1, 13, n) and K (7, 12, n), got {tuple(Xt.shape)} and {tuple(Kt.shape)}")
        Xt, Kt = Xt.contiguous(), Kt.contiguous()
        H, n = Xt.shape[0] - 1, Xt.shape[2]
        Kx = torch.empty((H, 7, 13, n), device=dev, dtype=torch.float32)
        _lib.check(lib.ac_lqr_gains_f32(self._handle, Xt.data_ptr(), Kt.data_ptr(), n, H, Kx.data_ptr(), self._stream()),
                   "ac_lqr_gains_f32")
        if from_np:
            Kx = Kx.cpu().numpy().astype(np.float64)
        return Kx[..., 0] if vec else Kx

    def steady_error(self, x, xnom):
        """xi (12, n): the steady-flight error coordinates of x (13, n) about the nominal xnom (13, n): heading-frame position
        error (along-track, cross-track, down), body-velocity error, tilt about the heading frame's forward and right axes,
        heading error, body-rate error.  Exactly 0 for x = xnom."""
        torch = _torch_mod()
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        Xb, _, _ = self._in(xnom, self.num_states, "xnom")
        if Xb.shape != X.shape:
            raise ValueError("x and xnom must have the same shape")
        n = X.shape[1]
        xi = torch.empty((12, n), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_steady_error_f32(self._handle, X.data_ptr(), Xb.data_ptr(), n, xi.data_ptr(), self._stream()),
                   "ac_steady_error_f32")
        return self._out(xi, npx, vec)

    def rollout_lqr(self, res: LqrResult, x0, H, dt=None, limits=None):
        """Fly the closed loop u_k = clip(u_b + K_x,k (x_k - Xnom_k)) for H steps from x0 (13, n): Xnom is this handle's
        rollout of the design's nominal (res.x, res.u), the gains come from res.gains(Xnom), the loop runs through
        ac_rollout_policy_f32 (and inherits its model restrictions).  dt defaults to the design's; limits = (u_min (7,),
        u_max (7,)) (default: none).  -> X (H+1, 13, n), U (H, 7, n), Xnom (H+1, 13, n)."""
        torch = _torch_mod()
        if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or H < 1:
            raise ValueError(f"rollout_lqr: H must be an integer >= 1, got {H!r}")
        dt = res.dt if dt is None else float(dt)
        lo, hi = (np.full(7, -np.inf), np.full(7, np.inf)) if limits is None else (np.asarray(b, dtype=np.float64) for b in limits)
        if lo.shape != (7,) or hi.shape != (7,) or np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any():
            raise ValueError("rollout_lqr: limits must be (u_min (7,), u_max (7,)) with u_min <= u_max")
        lib = self._sync()
        X0, npx, vec = self._in(x0, self.num_states, "x0")
        Xb, _, _ = self._in(res.x, self.num_states, "res.x")
        Ub, _, _ = self._in(res.u, _lib.NUM_CONTROLS, "res.u")
        n = X0.shape[1]
        if Xb.shape[1] != n or Ub.shape[1] != n:
            raise ValueError("rollout_lqr: x0 and the design's nominal must have the same number of columns")
        Un = Ub.unsqueeze(0).expand(H, -1, -1).contiguous()
        Xnom = self.rollout(Xb, Un, dt)
        K = res.K if isinstance(res.K, torch.Tensor) else torch.as_tensor(np.asarray(res.K, dtype=np.float32))
        K = K.to(device=X0.device, dtype=torch.float32).reshape(7, 12, n)
        Kx = self._lqr_gains(Xnom, K)
        kff = torch.zeros((H, 7, n), device=X0.device, dtype=torch.float32)
        Xc = torch.empty((H + 1, 13, n), device=X0.device, dtype=torch.float32)
        Uc = torch.empty((H, 7, n), device=X0.device, dtype=torch.float32)
        lim = _lib.IlqrCost()
        lim.u_min[:] = [float(v) for v in lo]
        lim.u_max[:] = [float(v) for v in hi]
        lim.dt_row = 0
        alphas = (C.c_float * 1)(1.0)
        _lib.check(lib.ac_rollout_policy_f32(self._handle, C.byref(lim), X0.data_ptr(), Xnom.data_ptr(), Un.data_ptr(),
                                             Kx.data_ptr(), kff.data_ptr(), alphas, 1, C.c_float(dt), n, H, Xc.data_ptr(),
                                             Uc.data_ptr(), self._stream()), "ac_rollout_policy_f32")
        out = (Xc, Uc, Xnom)
        if npx:
            out = tuple(t.cpu().numpy().astype(np.float64) for t in out)
        return tuple(t[..., 0] for t in out) if vec else out

    # ---- flight modes: eigenvalues of the linearised step (include/aircraft_hip.h, ac_modes_f32) -------
    MODES_COORDS = {"flight": (3, 4, 5, 6, 7, 9, 10, 11), "path": (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11), "all": tuple(range(12))}

    def modes_workspace(self, n: int):
        """Device workspace of a modes call of n instances (ac_modes_workspace_floats); allocate it before capturing a graph."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_modes_workspace_floats(self._handle, int(n), C.byref(need)), "ac_modes_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    @classmethod
    def _modes_coords(cls, coords):
        if isinstance(coords, str):
            if coords not in cls.MODES_COORDS:
                raise ValueError(f"modes: coords must be one of {sorted(cls.MODES_COORDS)} or a sequence of indices, got {coords!r}")
            return cls.MODES_COORDS[coords]
        try:
            seq = list(coords)
            idx = [int(c) for c in seq]
            if any(isinstance(c, bool) or float(c) != i for c, i in zip(seq, idx)):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"modes: coords must be a name or a sequence of chart coordinate indices, got {coords!r}") from None
        if len(set(idx)) != len(idx) or any(c < 0 or c > 11 for c in idx) or not set(cls.MODES_COORDS["flight"]) <= set(idx):
            raise ValueError("modes: coords must be distinct indices 0 .. 11 that include the flight coordinates 3-7 and 9-11")
        return tuple(sorted(idx))

    def modes(self, trim_or_xu, dt, gains=None, coords="flight", max_iters=30, ws=None) -> ModesResult:
        """Flight modes of n instances: the eigenvalues of the step of length dt linearised in the steady-flight chart
        (steady_error) at `trim_or_xu`, a TrimResult or an (x (13, n), u (7, n)) pair; any state will do, at a trim the
        linearisation is that of the whole trim helix.  gains: None (open loop), an LqrResult (its K; its dt must be this
        dt) or a (7, 12, n) array K: the closed loop A - B K.  coords: "flight" (body velocity, tilt, body rates: 8), "path"
        (without along-track: 11), "all" (12) or a sequence of chart coordinate indices that includes the flight eight.
        max_iters: QR iterations per eigenvalue at most.  No host synchronisation (graph-capturable with a workspace from
        modes_workspace(n))."""
        torch = _torch_mod()
        if isinstance(trim_or_xu, TrimResult):
            x, u = trim_or_xu.x, trim_or_xu.u
        elif isinstance(trim_or_xu, (tuple, list)) and len(trim_or_xu) == 2:
            x, u = trim_or_xu
        else:
            raise ValueError("modes: pass a TrimResult or an (x, u) pair")
        shp = lambda a: tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)  # noqa: E731
        sx, su = shp(x), shp(u)
        if len(sx) not in (1, 2) or sx[0] != 13 or len(su) != len(sx) or su[0] != _lib.NUM_CONTROLS or sx[1:] != su[1:]:
            raise ValueError(f"modes: expected x (13, n) and u (7, n), got {sx} and {su}")
        if isinstance(dt, bool) or np.ndim(dt) != 0 or not np.isfinite(float(dt)) or float(dt) <= 0:
            raise ValueError(f"modes: dt must be a finite scalar > 0, got {dt!r}")
        if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or max_iters < 1:
            raise ValueError(f"modes: max_iters must be an integer >= 1, got {max_iters!r}")
        kept = self._modes_coords(coords)
        Kin = None
        if isinstance(gains, LqrResult):
            if float(gains.dt) != float(dt):
                raise ValueError(f"modes: the gains were designed for dt = {gains.dt!r}, not {dt!r}")
            Kin = gains.K
        elif gains is not None:
            Kin = gains
        if Kin is not None and shp(Kin) != (7, 12) + sx[1:]:
            raise ValueError(f"modes: expected gains (7, 12, n) for x {sx}, got {shp(Kin)}")
        if ws is not None and (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_cuda
                               or not ws.is_contiguous()):
            raise ValueError("modes: ws must be a contiguous float32 device tensor (modes_workspace(n))")

        # ---- device side ----
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in(u, _lib.NUM_CONTROLS, "u")
        n = X.shape[1]
        dev = X.device
        Kt = None
        if Kin is not None:
            Kt = Kin if isinstance(Kin, torch.Tensor) else torch.as_tensor(np.asarray(Kin, dtype=np.float32))
            Kt = Kt.to(device=dev, dtype=torch.float32).reshape(7, 12, n).contiguous()
        opts = _lib.ModesOpts()
        opts.coords = sum(1 << c for c in kept)
        opts.max_iters = int(max_iters)
        if ws is None:
            ws = self.modes_workspace(n)
        f32 = dict(device=dev, dtype=torch.float32)
        A, Bm = torch.empty((12, 12, n), **f32), torch.empty((12, 7, n), **f32)
        out = torch.empty((4, 12, n), **f32)
        S, it = torch.empty((n,), device=dev, dtype=torch.int32), torch.empty((n,), device=dev, dtype=torch.int32)
        _lib.check(lib.ac_modes_f32(self._handle, C.byref(opts), X.data_ptr(), U.data_ptr(), C.c_float(float(dt)),
                                    Kt.data_ptr() if Kt is not None else None, n, A.data_ptr(), Bm.data_ptr(), out[0].data_ptr(),
                                    out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), S.data_ptr(), it.data_ptr(),
                                    ws.data_ptr(), ws.numel(), self._stream()), "ac_modes_f32")
        m = len(kept)
        lam = torch.complex(out[0, :m], out[1, :m])
        s = torch.complex(out[2, :m], out[3, :m])
        if npx:
            lam, s = lam.cpu().numpy().astype(np.complex128), s.cpu().numpy().astype(np.complex128)
            A, Bm = (t.cpu().numpy().astype(np.float64) for t in (A, Bm))
            S, it = S.cpu().numpy(), it.cpu().numpy()
            mag, wn = np.abs(lam), np.abs(s)
            with np.errstate(invalid="ignore", divide="ignore"):
                zeta = -s.real / wn
            rho, unstable = mag.max(axis=0), (mag > 1).sum(axis=0)
        else:
            mag, wn = lam.abs(), s.abs()
            zeta = -s.real / wn
            rho, unstable = mag.max(dim=0).values, (mag > 1).sum(dim=0)
        res = [lam, s, wn, zeta, rho, unstable, A, Bm]
        tail = [S, S == 0, it]
        if vec:
            res, tail = [t[..., 0] for t in res], [t[..., 0] for t in tail]
        return ModesResult(*res, kept, *tail, float(dt))

    def eig(self, M):
        """Eigenvalues of n real m x m matrices M (m, m, n) or (m, m), 1 <= m <= 13, on the device (ac_eig_f32) ->
        (lam (m, n) complex in the canonical order of ModesResult.lam, status (n,): 0 found, 1 iteration cap, 3 non-finite)."""
        torch = _torch_mod()
        from_np = not isinstance(M, torch.Tensor)
        sm = np.shape(M) if from_np else tuple(M.shape)
        if len(sm) not in (2, 3) or sm[0] != sm[1] or not 1 <= sm[0] <= _lib.EIG_MAX_M:
            raise ValueError(f"eig: expected M (m, m, n) or (m, m) with 1 <= m <= {_lib.EIG_MAX_M}, got {sm}")
        lib = self._sync()
        dev = self._device_obj()
        Mt = torch.as_tensor(np.asarray(M, dtype=np.float32) if from_np else M).to(device=dev, dtype=torch.float32)
        vec = Mt.dim() == 2
        if vec:
            Mt = Mt.unsqueeze(-1)
        Mt = Mt.contiguous()
        m, n = Mt.shape[0], Mt.shape[2]
        w = torch.empty((2, m, n), device=dev, dtype=torch.float32)
        S = torch.empty((n,), device=dev, dtype=torch.int32)
        _lib.check(lib.ac_eig_f32(self._handle, Mt.data_ptr(), m, 0, n, w[0].data_ptr(), w[1].data_ptr(), S.data_ptr(), None,
                                  self._stream()), "ac_eig_f32")
        lam = torch.complex(w[0], w[1])
        if from_np:
            lam, S = lam.cpu().numpy().astype(np.complex128), S.cpu().numpy()
        return (lam[..., 0], S[..., 0]) if vec else (lam, S)

    # ---- extended Kalman filter (include/aircraft_hip.h, ac_ekf_step_f32) -------------------------------
    EKF_MAG_NED = EKF_MAG_NED  # (the module's: SensorModel's default too)

    def ekf_workspace(self, n: int):
        """Device workspace of a bank of n filters (ac_ekf_workspace_floats); allocate it before capturing a graph."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_ekf_workspace_floats(self._handle, int(n), C.byref(need)), "ac_ekf_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def ekf_em_workspace(self, n: int, T: int):
        """Device workspace of EKF.noise_stats over n instances and T nodes (ac_ekf_em_workspace_floats)."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_ekf_em_workspace_floats(self._handle, int(n), int(T), C.byref(need)), "ac_ekf_em_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def ieks_workspace(self, n: int, T: int, candidates: int):
        """Device workspace of EKF.map_smooth over n instances, T steps and a ladder of `candidates` step lengths
        (ac_ieks_workspace_floats)."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_ieks_workspace_floats(self._handle, int(n), int(T), int(candidates), C.byref(need)), "ac_ieks_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def ukf_workspace(self, n: int):
        """Device workspace of a bank of n unscented filters (ac_ukf_workspace_floats); allocate it before capturing a graph."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_ukf_workspace_floats(self._handle, int(n), C.byref(need)), "ac_ukf_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def ukf(self, x0, P0, *, q, r, kappa=0.0, mag_ned=EKF_MAG_NED, ws=None) -> UKF:
        """A bank of n unscented Kalman filters: Aircraft.ekf's arguments and checks, plus kappa >= 0 (the centre point's weight
        is kappa / (12 + kappa); 0, the default, leaves it out of the means).  ws: ukf_workspace(n)."""
        if isinstance(kappa, bool) or np.ndim(kappa) != 0 or not np.isfinite(float(kappa)) or float(kappa) < 0:
            raise ValueError(f"ukf: kappa must be a finite scalar >= 0, got {kappa!r}")
        return self.ekf(x0, P0, q=q, r=r, mag_ned=mag_ned, ws=ws, _bank=lambda *a: UKF(*a, kappa=float(kappa)))

    def ekf(self, x0, P0, *, q, r, mag_ned=EKF_MAG_NED, ws=None, _bank=None) -> EKF:
        """A bank of n extended Kalman filters started at x0 (13, n) with covariance P0 (12, 12, n) in the error coordinates
        (dp NED, dv NED, dtheta body-frame rotation vector, dw).  q: process-noise variances per step, (12,) for every
        instance or (12, n); r: measurement variances > 0 of the 15 rows, (15,) or (15, n); mag_ned: the magnetic field in NED
        (in the units the magnetometer reports).  Shapes, the symmetry and positive diagonal of P0 and the sign of q and r
        are checked before any device is touched (values of tensors already on a device are not read)."""
        torch = _torch_mod()
        host = lambda a: not (isinstance(a, torch.Tensor) and a.is_cuda)  # noqa: E731
        shp = lambda a: tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)  # noqa: E731
        val = lambda a: a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)  # noqa: E731
        sx, sp = shp(x0), shp(P0)
        if len(sx) not in (1, 2) or sx[0] != 13 or sp != (12, 12) + sx[1:]:
            raise ValueError(f"ekf: expected x0 (13, n) and P0 (12, 12, n), got {sx} and {sp}")
        n = sx[1] if len(sx) == 2 else 1
        for a, rows, name in ((q, 12, "q"), (r, _lib.EKF_ROWS, "r")):
            if shp(a) not in ((rows,), (rows, n)):
                raise ValueError(f"ekf: {name} must have shape ({rows},) or ({rows}, {n}), got {shp(a)}")
        mg = np.asarray(mag_ned, dtype=np.float64)
        if mg.shape != (3,) or not np.isfinite(mg).all():
            raise ValueError("ekf: mag_ned must be 3 finite numbers")
        if host(P0):
            Pv = val(P0).reshape(12, 12, -1)
            if not np.isfinite(Pv).all() or not np.array_equal(Pv, Pv.transpose(1, 0, 2)):
                raise ValueError("ekf: P0 must be finite and symmetric")
            if (Pv[np.arange(12), np.arange(12)] <= 0).any():
                raise ValueError("ekf: the diagonal of P0 must be > 0")
        if host(q) and (not np.isfinite(val(q)).all() or (val(q) < 0).any()):
            raise ValueError("ekf: q must be finite and >= 0")
        if host(r) and (not np.isfinite(val(r)).all() or (val(r) <= 0).any()):
            raise ValueError("ekf: r must be finite and > 0")
        if ws is not None and (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_cuda
                               or not ws.is_contiguous()):
            raise ValueError("ekf: ws must be a contiguous float32 device tensor (ekf_workspace(n))")

        # ---- device side ----
        self._sync()
        X, npx, vec = self._in(x0, self.num_states, "x0")
        dev = X.device
        to = lambda a: (torch.as_tensor(np.asarray(a, dtype=np.float32)) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=torch.float32)  # noqa: E731
        P = to(P0).reshape(12, 12, n).contiguous().clone()
        Qd = to(q).reshape(12, -1).expand(12, n).contiguous()
        Rd = to(r).reshape(_lib.EKF_ROWS, -1).expand(_lib.EKF_ROWS, n).contiguous()
        if ws is None:
            ws = self.ekf_workspace(n) if _bank is None else self.ukf_workspace(n)
        return (_bank or EKF)(self, X.clone(), P, Qd, Rd, mg, ws, npx, vec)

    def measure(self, x, mag_ned=EKF_MAG_NED):
        """z (15, n) = h(x): what the filter's sensors read at the state x (13, n) without noise: GPS position, GPS velocity
        (NED), gyro, air data (V, alpha, beta: the airspeed, alpha, beta getters bit for bit), magnetometer R(q)' mag_ned."""
        torch = _torch_mod()
        mg = np.asarray(mag_ned, dtype=np.float64)
        if mg.shape != (3,) or not np.isfinite(mg).all():
            raise ValueError("measure: mag_ned must be 3 finite numbers")
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        n = X.shape[1]
        Z = torch.empty((_lib.EKF_ROWS, n), device=X.device, dtype=torch.float32)
        o = _lib.EkfOpts()
        o.mag_ned[:] = [float(v) for v in mg]
        _lib.check(lib.ac_ekf_measure_f32(self._handle, C.byref(o), X.data_ptr(), n, Z.data_ptr(), self._stream()), "ac_ekf_measure_f32")
        return self._out(Z, npx, vec)

    # ---- the loop closed through the estimator (include/aircraft_hip.h, ac_lqg_rollout_f32) ----------------
    @staticmethod
    def _step_index(step, name):
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)) or not -2 ** 31 <= int(step) < 2 ** 31:
            raise ValueError(f"{name}: step must be a 32-bit integer, got {step!r}")
        return int(step)

    def sense(self, x, sensors: SensorModel, step, step_dev=None):
        """(z (15, n), mask (n,)): what the simulated sensors report at the state x (13, n) at step `step`: h(x) plus the seeded
        noise of `sensors`, NaN and a cleared mask bit for a group that does not report.  step_dev: an int32 device tensor of one
        element that is added to `step` on the device (a captured call draws fresh noise when the caller increments it)."""
        torch = _torch_mod()
        if not isinstance(sensors, SensorModel):
            raise ValueError("sense: sensors must be a SensorModel")
        step = self._step_index(step, "sense")
        if step_dev is not None and (not isinstance(step_dev, torch.Tensor) or step_dev.dtype != torch.int32 or step_dev.numel() != 1
                                     or not step_dev.is_cuda):
            raise ValueError("sense: step_dev must be an int32 device tensor of one element")
        shp = tuple(x.shape) if isinstance(x, torch.Tensor) else np.shape(x)
        if len(shp) not in (1, 2) or shp[0] != 13:
            raise ValueError(f"sense: expected x (13, n), got {shp}")
        n = shp[1] if len(shp) == 2 else 1
        sg = sensors.sigma
        if len(sg.shape) == 2 and sg.shape[1] != n:
            raise ValueError(f"sensors: sigma must have shape (15,) or (15, {n}), got {tuple(sg.shape)}")
        lib = self._sync()
        X, npx, vec = self._in(x, self.num_states, "x")
        S = sensors._sigma(n, X.device)
        Z = torch.empty((_lib.EKF_ROWS, n), device=X.device, dtype=torch.float32)
        M = torch.empty((n,), device=X.device, dtype=torch.int32)
        o = sensors._opts()
        _lib.check(lib.ac_sense_f32(self._handle, C.byref(o), step, None if step_dev is None else step_dev.data_ptr(), X.data_ptr(),
                                    S.data_ptr(), n, Z.data_ptr(), M.data_ptr(), self._stream()), "ac_sense_f32")
        Z = self._out(Z, npx, vec)
        M = M.cpu().numpy() if npx else M
        return Z, (M[0] if vec else M)

    def lqg_workspace(self, est, n: int):
        """Device workspace of an output-feedback rollout of n instances with the estimator `est` (an EKF or UKF bank, or
        "ekf" / "ukf") (ac_lqg_workspace_floats); allocate it before capturing a graph."""
        kind = est if isinstance(est, str) else ("ukf" if isinstance(est, UKF) else "ekf")
        if kind not in _lib.LQG_ESTIMATORS:
            raise ValueError(f"lqg_workspace: expected 'ekf' or 'ukf', got {est!r}")
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_lqg_workspace_floats(self._handle, _lib.LQG_ESTIMATORS[kind], int(n), C.byref(need)), "ac_lqg_workspace_floats")
        return _torch_mod().empty(max(need.value, 1), device=self._device_obj(), dtype=_torch_mod().float32)

    def rollout_output_feedback(self, est, x0, Xnom, Unom, Kx, dt, sensors: SensorModel, process_sigma=None, limits=None,
                                feedback="estimate", record=(), step0=0, ws=None) -> LqgResult:
        """Fly T steps of the closed loop in which the controller sees only what the estimator gives it.  est: an EKF or UKF bank
        of this aircraft (Aircraft.ekf / Aircraft.ukf): it supplies x^0, P0, q, r and holds the final estimate afterwards, as
        est.filter leaves it.  x0 (13, n): the true starting state; Xnom (T+1, 13, n), Unom (T, 7, n), Kx (T, 7, 13, n): the
        nominal and the raw-state gains of u_k = clip(Unom_k + Kx_k (fb_k - Xnom_k)) (LqrResult.gains, ILQR), fb the estimate
        (feedback="estimate") or the truth ("truth").  After every step the truth gets process noise of standard deviation
        process_sigma ((12,) or (12, n) in the error coordinates, finite and >= 0, checked for host values; None: none), is
        measured by `sensors` at step step0 + k + 1 and the estimator takes its own step.  step0 + T must stay below 2^31.  limits = (u_min (7,), u_max (7,)) (default: none); record=("P",) also returns the
        covariances; ws: lqg_workspace(est, n).  The bank's mag_ned must be the sensors'.  Shapes and host values are checked
        before any device is touched."""
        torch = _torch_mod()
        name = "rollout_output_feedback"
        dt, lo, hi, record, step0 = self._lqg_args(name, est, sensors, dt, process_sigma, limits, feedback, record, step0, ws)
        shp = lambda a: tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)  # noqa: E731
        n, vec = est.n, est._vec
        tail = () if vec else (n,)
        sx, sn = shp(x0), shp(Xnom)
        if sx != (13,) + tail:
            raise ValueError(f"{name}: x0 must have shape {(13,) + tail}, got {sx}")
        if len(sn) != 2 + len(tail) or sn[0] < 1 or sn[1:] != (13,) + tail:
            raise ValueError(f"{name}: Xnom must have shape (T+1, 13{', n' if tail else ''}), got {sn}")
        T = sn[0] - 1
        if shp(Unom) != (T, 7) + tail or shp(Kx) != (T, 7, 13) + tail:
            raise ValueError(f"{name}: expected Unom {(T, 7) + tail} and Kx {(T, 7, 13) + tail}, got {shp(Unom)} and {shp(Kx)}")
        if step0 + T > 2 ** 31 - 1:
            raise ValueError(f"{name}: step0 + T must stay below 2^31, got {step0} + {T}")
        # ---- device side ----
        self._sync()
        dev = est._X.device
        to = lambda a: (torch.as_tensor(np.asarray(a, dtype=np.float32)) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=torch.float32)  # noqa: E731
        X0 = to(x0).reshape(13, n).contiguous()
        Xn, Un, Kt = to(Xnom).reshape(T + 1, 13, n).contiguous(), to(Unom).reshape(T, 7, n).contiguous(), to(Kx).reshape(T, 7, 13, n).contiguous()
        out = self._lqg_run(est, X0, Xn, Un, Kt, dt, sensors, process_sigma, lo, hi, feedback, record, step0, ws)
        return LqgResult(*(None if t is None else est._give(t) for t in out))

    def _lqg_args(self, name, est, sensors, dt, process_sigma, limits, feedback, record, step0, ws):
        """the checks the output-feedback rollouts share (no device is touched) -> dt, u_min, u_max, record, step0"""
        torch = _torch_mod()
        if not isinstance(est, EKF) or est.system is not self:
            raise ValueError(f"{name}: est must be an EKF or UKF bank of this aircraft (Aircraft.ekf / Aircraft.ukf)")
        if not isinstance(sensors, SensorModel):
            raise ValueError(f"{name}: sensors must be a SensorModel")
        if tuple(est.mag_ned) != tuple(sensors.mag_ned):  # (the loop hands the filter the sensors' field: one model, not two)
            raise ValueError(f"{name}: the bank's mag_ned {est.mag_ned} differs from the sensors' {sensors.mag_ned}")
        if feedback not in _lib.LQG_FEEDBACK:
            raise ValueError(f"{name}: feedback must be 'estimate' or 'truth', got {feedback!r}")
        record = (record,) if isinstance(record, str) else tuple(record)
        if any(r != "P" for r in record):
            raise ValueError(f"{name}: record may hold 'P' only, got {record!r}")
        dt = EKF._dt(dt, True)
        step0 = self._step_index(step0, name)
        lo, hi = (np.full(7, -np.inf), np.full(7, np.inf)) if limits is None else (np.asarray(b, dtype=np.float64) for b in limits)
        if lo.shape != (7,) or hi.shape != (7,) or np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any():
            raise ValueError(f"{name}: limits must be (u_min (7,), u_max (7,)) with u_min <= u_max")
        n = est.n
        sg = sensors.sigma
        if len(sg.shape) == 2 and sg.shape[1] != n:
            raise ValueError(f"sensors: sigma must have shape (15,) or (15, {n}), got {tuple(sg.shape)}")
        if process_sigma is not None:
            ps = tuple(process_sigma.shape) if isinstance(process_sigma, torch.Tensor) else np.shape(process_sigma)
            if ps not in ((12,), (12, n)):
                raise ValueError(f"{name}: process_sigma must have shape (12,) or (12, {n}), got {ps}")
            if not (isinstance(process_sigma, torch.Tensor) and process_sigma.is_cuda):  # (device values are not read)
                pv = process_sigma.detach().numpy() if isinstance(process_sigma, torch.Tensor) else process_sigma
                pv = np.asarray(pv, dtype=np.float64)
                if not np.isfinite(pv).all() or (pv < 0).any():
                    raise ValueError(f"{name}: process_sigma must be finite and >= 0")
        if ws is not None and (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or not ws.is_cuda or not ws.is_contiguous()):
            raise ValueError(f"{name}: ws must be a contiguous float32 device tensor (lqg_workspace(est, n))")
        return dt, lo, hi, record, step0

    def _lqg_run(self, est, X0, Xn, Un, Kt, dt, sensors, process_sigma, lo, hi, feedback, record, step0, ws):
        """the device tensors of LqgResult's fields, in order, from checked device operands"""
        torch = _torch_mod()
        lib = self._sync()
        dev, n, T = est._X.device, est.n, Un.shape[0]
        to = lambda a: (torch.as_tensor(np.asarray(a, dtype=np.float32)) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=torch.float32)  # noqa: E731
        Sr = sensors._sigma(n, dev)
        Sq = None if process_sigma is None else to(process_sigma).reshape(12, -1).expand(12, n).contiguous()
        ukf = isinstance(est, UKF)
        if ws is None:
            ws = self.lqg_workspace(est, n)
        f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
        Xo, Po = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)
        Xt, Xh, U = torch.empty((T + 1, 13, n), **f32), torch.empty((T + 1, 13, n), **f32), torch.empty((T, 7, n), **f32)
        Ps = torch.empty((T, 12, 12, n), **f32) if "P" in record else None
        Z, M = torch.empty((T, _lib.EKF_ROWS, n), **f32), torch.empty((T, n), **i32)
        nis, nees, err = torch.empty((T, n), **f32), torch.empty((T, n), **f32), torch.empty((T, 12, n), **f32)
        used, st, sst = torch.empty((T, n), **i32), torch.empty((T, n), **i32), torch.empty((T, n), **i32)
        o = _lib.LqgOpts()
        o.estimator, o.feedback = _lib.LQG_ESTIMATORS["ukf" if ukf else "ekf"], _lib.LQG_FEEDBACK[feedback]
        o.kappa, o.step0 = (est.kappa if ukf else 0.0), step0
        so = sensors._opts()
        lim = _lib.IlqrCost()
        lim.u_min[:] = [float(v) for v in lo]
        lim.u_max[:] = [float(v) for v in hi]
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _lib.check(lib.ac_lqg_rollout_f32(self._handle, C.byref(o), C.byref(so), C.byref(lim), X0.data_ptr(), est._X.data_ptr(),
                                          est._P.data_ptr(), Xn.data_ptr(), Un.data_ptr(), Kt.data_ptr(), est._Qd.data_ptr(),
                                          est._Rd.data_ptr(), ptr(Sq), Sr.data_ptr(), C.c_float(dt), n, T, Xo.data_ptr(), Po.data_ptr(),
                                          Xt.data_ptr(), Xh.data_ptr(), U.data_ptr(), ptr(Ps), Z.data_ptr(), M.data_ptr(), nis.data_ptr(),
                                          nees.data_ptr(), used.data_ptr(), st.data_ptr(), sst.data_ptr(), err.data_ptr(), ws.data_ptr(),
                                          ws.numel(), self._stream()), "ac_lqg_rollout_f32")
        if T:
            est._X, est._P = Xo, Po
        else:
            Xt[0], Xh[0] = X0, est._X
        return (Xt, Xh, U, Z, M, nis, nees, err, used, st, Xn, Ps)

    def rollout_lqg(self, res: LqrResult, est, x0, T, sensors: SensorModel, dt=None, process_sigma=None, limits=None,
                    feedback="estimate", record=(), step0=0, ws=None) -> LqgResult:
        """rollout_lqr flown on the estimate: Xnom is this handle's rollout of the design's nominal (res.x, res.u), the gains are
        res.gains(Xnom) (exactly what rollout_lqr builds), and the loop is rollout_output_feedback's (see there for the other
        arguments).  dt defaults to the design's."""
        torch = _torch_mod()
        if not isinstance(res, LqrResult):
            raise ValueError("rollout_lqg: res must be an LqrResult (Aircraft.lqr)")
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
            raise ValueError(f"rollout_lqg: T must be an integer >= 1, got {T!r}")
        dt, lo, hi, record, step0 = self._lqg_args("rollout_lqg", est, sensors, res.dt if dt is None else dt, process_sigma, limits,
                                                   feedback, record, step0, ws)
        if step0 + int(T) > 2 ** 31 - 1:
            raise ValueError(f"rollout_lqg: step0 + T must stay below 2^31, got {step0} + {T}")
        shp = lambda a: tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)  # noqa: E731
        tail = () if est._vec else (est.n,)
        if shp(x0) != (13,) + tail or shp(res.x) != (13,) + tail or shp(res.u) != (7,) + tail:
            raise ValueError(f"rollout_lqg: x0 and the design's nominal must have shapes {(13,) + tail} and {(7,) + tail}, got {shp(x0)}, "
                             f"{shp(res.x)}, {shp(res.u)}")
        Xb, _, _ = self._in(res.x, self.num_states, "res.x")
        Ub, _, _ = self._in(res.u, _lib.NUM_CONTROLS, "res.u")
        n = est.n
        Un = Ub.unsqueeze(0).expand(int(T), -1, -1).contiguous()
        Xnom = self.rollout(Xb, Un, dt)
        K = res.K if isinstance(res.K, torch.Tensor) else torch.as_tensor(np.asarray(res.K, dtype=np.float32))
        K = K.to(device=Xb.device, dtype=torch.float32).reshape(7, 12, n)
        Kx = self._lqr_gains(Xnom, K)
        X0 = (torch.as_tensor(np.asarray(x0, dtype=np.float32)) if not isinstance(x0, torch.Tensor) else x0)
        X0 = X0.to(device=Xb.device, dtype=torch.float32).reshape(13, n).contiguous()
        out = self._lqg_run(est, X0, Xnom, Un, Kx, dt, sensors, process_sigma, lo, hi, feedback, record, step0, ws)
        return LqgResult(*(None if t is None else est._give(t) for t in out))

    # what the test oracle needs to rebuild the same airframe (tests only)
    def airframe_dict(self) -> dict:
        return {"mass": float(self.mass), "reference_area": float(self.S), "span": float(self.b), "chord": float(self.c),
                "Ixx": self.Ixx, "Iyy": self.Iyy, "Izz": self.Izz, "Ixz": self.Ixz,
                "com": [float(v) for v in np.asarray(self.com).ravel()],
                "rudder_moment_arm": float(self.rudder_moment_arm)}
