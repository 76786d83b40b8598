"""Batched 6-DoF NED rigid body on MI355X — the `SixDOF` plugin surface of the reference
(src/aircraft/dynamics/base.py:16-480) with the CasADi graph replaced by HIP kernels.

What stays the same for a caller (control/base.py:187-190 is the consumer):
    system.state_update          callable  F(x, u, dt) -> x+          with .size1_in(0) == 13, .size1_in(1) == 7
    system.state_derivative      callable  f(x, u)     -> x_dot
    system.normalise, .physical_integration_substeps, .com, .mass   plain attributes, read at call time
    getters v_frd_rel / airspeed / alpha / beta / qbar / coefficients / forces_frd / moments_frd / phi / theta / psi
What changes: arguments are column batches `(13, n)` / `(7, n)` (the reference's column-mapped call
convention, main/control/control.py:63) living on the GPU as float32 torch tensors; numpy in -> numpy out.
New on this surface: `rollout`, `step_sens` (A = dF/dx, B = dF/du, c = dF/ddt).
"""
from __future__ import annotations

import ctypes as C
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from .. import _lib

NUM_STATES = _lib.NUM_STATES


@dataclass
class SixDOFOpts:
    """reference dynamics/base.py:9-14"""
    epsilon: float = 1e-6
    physical_integration_substeps: int = 10
    gravity: Sequence[float] = field(default_factory=lambda: (0.0, 0.0, 9.81))
    mass: float = 1.0


class BatchedFunction:
    """Stand-in for the `ca.Function` objects the reference hands to its controllers."""

    def __init__(self, name, in_dims, out_dim, fn):
        self._name, self._in_dims, self._out_dim, self._fn = name, tuple(in_dims), out_dim, fn

    def name(self):
        return self._name

    def size1_in(self, i):
        return self._in_dims[i]

    def size1_out(self, i=0):
        return self._out_dim

    def n_in(self):
        return len(self._in_dims)

    def __call__(self, *args, **kw):
        return self._fn(*args, **kw)

    def __repr__(self):
        return f"BatchedFunction({self._name}: {self._in_dims} -> {self._out_dim})"


def _torch():
    import torch

    return torch


# Handles whose release was requested while a stream was capturing.  ac_destroy frees device memory (hipFree), which is
# not permitted while a capture is open and invalidates it ("operation failed due to a previous error during capture") —
# and a release can be requested at any point of a capture: a cyclic-GC pass or a refcount reaching zero runs
# SixDOF.__del__ wherever it happens to.  Such handles are parked here and destroyed by the next call that finds no
# capture open (_drain_parked: every _sync(), every close()).
_PARKED: list = []


def _capturing() -> bool:
    import sys

    torch = sys.modules.get("torch")
    try:
        return bool(torch is not None and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())
    except Exception:
        return False


def _drain_parked() -> None:
    if _PARKED and not _capturing():
        lib = _lib.load()
        while _PARKED:
            lib.ac_destroy(_PARKED.pop())


class SixDOF(ABC):
    """Base class for batched 6-DoF dynamics in a NED frame."""

    num_states: int = NUM_STATES
    num_controls: int

    def __init__(self, *, opts: Optional[SixDOFOpts] = None, device=None, **kwargs) -> None:
        if opts is None:
            opts = SixDOFOpts()
        self.opts = opts
        self.gravity = tuple(float(g) for g in opts.gravity)
        self.epsilon = opts.epsilon
        self.mass = opts.mass
        self.normalise = False  # controllers flip this (control/base.py:182-185)
        self.vjp_route = "auto"  # reverse mode: "auto" (fused where a fused kernel exists), "fused" or "composed"
        # hidden layers of the width-128 sensitivity kernels: "auto" (two-plane f16 MFMA where the net passes the range gate,
        # else three-plane bf16), "bf16" or "f16" (an error on a net the gate rejects); ac_set_hidden_route
        self.hidden_route = "auto"
        self._installed_route = "auto"
        self.physical_integration_substeps: int = opts.physical_integration_substeps
        self.stall_scaling = False
        self._handle = C.c_void_p()
        self._installed_key = None
        self._device = device

    # ---- subclass hooks ---------------------------------------------------------------------
    @abstractmethod
    def _param_struct(self) -> "_lib.AcParams":
        """Current constants as an ac_params (rebuilt whenever an attribute changed)."""

    @abstractmethod
    def _install_model(self) -> None:
        """Push coefficient-model data into the handle."""

    # ---- handle management ------------------------------------------------------------------
    def _device_obj(self):
        torch = _torch()
        if self._device is None:
            if not torch.cuda.is_available():
                raise _lib.AircraftHipError("no GPU visible: aircraft_amd runs on MI355X only (no CPU fallback)")
            self._device = torch.device("cuda", torch.cuda.current_device())
        return torch.device(self._device)

    def _sync(self):
        """Create the handle on first use; re-send constants if any attribute changed since the last call."""
        lib = _lib.load()
        _drain_parked()
        p = self._param_struct()
        key = bytes(p)
        torch = _torch()
        dev = self._device_obj()
        if not self._handle:
            with torch.cuda.device(dev):
                _lib.check(lib.ac_create(C.byref(p), C.byref(self._handle)), "ac_create")
                self._install_model()
            self._installed_key = key
        elif key != self._installed_key:
            _lib.check(lib.ac_set_params(self._handle, C.byref(p)), "ac_set_params")
            self._installed_key = key
        if self.hidden_route != self._installed_route:
            if self.hidden_route not in _lib.HIDDEN_ROUTES:
                raise ValueError(f"hidden_route: expected one of {sorted(_lib.HIDDEN_ROUTES)}, got {self.hidden_route!r}")
            _lib.check(lib.ac_set_hidden_route(self._handle, _lib.HIDDEN_ROUTES[self.hidden_route]), "ac_set_hidden_route")
            self._installed_route = self.hidden_route
        return lib

    def close(self):
        if getattr(self, "_handle", None):
            if _capturing():
                _PARKED.append(C.c_void_p(self._handle.value))  # destroyed after the capture (see _PARKED)
            else:
                _lib.load().ac_destroy(self._handle)
            self._handle = C.c_void_p()
            # the workspaces died with the handle: a re-created one must be reserved again
            self._hess_reserved = 0
            self._installed_key = None
            self._installed_route = "auto"
        _drain_parked()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tensor hand-off --------------------------------------------------------------------
    def _in_u(self, u):
        """Controls -> the 7-row device layout.  A plugin with fewer controls (the quadrotor's four thrusts) passes
        (num_controls, n); rows beyond are zero and ignored by its kernels.  A ready 7-row buffer passes through."""
        torch = _torch()
        rows = self.num_controls
        shape = tuple(getattr(u, "shape", ()))
        if rows < _lib.NUM_CONTROLS and len(shape) >= 1 and shape[0] == _lib.NUM_CONTROLS:
            rows = _lib.NUM_CONTROLS
        U, npu, vec = self._in(u, rows, "u")
        if rows < _lib.NUM_CONTROLS:
            U = torch.cat([U, torch.zeros((_lib.NUM_CONTROLS - rows, U.shape[1]), device=U.device, dtype=U.dtype)])
        return U, npu, vec

    def _in(self, a, rows, name):
        """-> (float32 contiguous cuda tensor (rows, n), came_from_numpy, was_vector)"""
        torch = _torch()
        dev = self._device_obj()
        from_np = not isinstance(a, torch.Tensor)
        t = torch.as_tensor(np.asarray(a, dtype=np.float32) if from_np else a)
        vec = t.dim() == 1
        if vec:
            t = t.reshape(-1, 1)
        if t.dim() != 2 or t.shape[0] != rows:
            raise ValueError(f"{name}: expected ({rows}, n), got {tuple(t.shape)}")
        t = t.to(device=dev, dtype=torch.float32).contiguous()
        return t, from_np, vec

    @staticmethod
    def _out(t, from_np, vec):
        if vec:
            t = t.reshape(t.shape[0] if t.dim() == 2 else t.shape[:-1])
        return t.cpu().numpy().astype(np.float64) if from_np else t

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self._device_obj()).cuda_stream)

    def _dt_args(self, dt, n):
        """scalar dt -> (dt, NULL) ; per-unit dt (n,) -> (0, ptr)."""
        torch = _torch()
        if isinstance(dt, torch.Tensor) and dt.numel() > 1 or (not isinstance(dt, torch.Tensor) and np.ndim(dt) > 0 and np.size(dt) > 1):
            t = torch.as_tensor(np.asarray(dt, dtype=np.float32) if not isinstance(dt, torch.Tensor) else dt)
            t = t.to(device=self._device_obj(), dtype=torch.float32).contiguous().reshape(-1)
            if t.numel() != n:
                raise ValueError(f"dt: expected a scalar or {n} values, got {t.numel()}")
            return C.c_float(0.0), C.c_void_p(t.data_ptr()), t
        return C.c_float(float(dt)), C.c_void_p(0), None

    # ---- the plugin surface -----------------------------------------------------------------
    @property
    def state_derivative(self) -> BatchedFunction:
        """x_dot = f(x, u)   (reference dynamics/base.py:385-406)"""

        def f(x, u):
            lib = self._sync()
            torch = _torch()
            X, npx, vec = self._in(x, self.num_states, "x")
            U, _, _ = self._in_u(u)
            n = X.shape[1]
            if U.shape[1] != n:
                raise ValueError("x and u must have the same number of columns")
            out = torch.empty_like(X)
            _lib.check(lib.ac_state_derivative_f32(self._handle, X.data_ptr(), U.data_ptr(), n, out.data_ptr(),
                                                   self._stream()), "ac_state_derivative_f32")
            return self._out(out, npx, vec)

        return BatchedFunction("dynamics", (self.num_states, self.num_controls), self.num_states, f)

    @property
    def state_update(self) -> BatchedFunction:
        """x+ = F(x, u, dt): RK4 with `physical_integration_substeps` sub-steps (reference dynamics/base.py:450-480)"""

        def F(x, u, dt):
            lib = self._sync()
            torch = _torch()
            X, npx, vec = self._in(x, self.num_states, "x")
            U, _, _ = self._in_u(u)
            n = X.shape[1]
            if U.shape[1] != n:
                raise ValueError("x and u must have the same number of columns")
            dts, dtp, keep = self._dt_args(dt, n)
            out = torch.empty_like(X)
            _lib.check(lib.ac_step_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, out.data_ptr(),
                                       self._stream()), "ac_step_f32")
            del keep
            return self._out(out, npx, vec)

        return BatchedFunction("state_update", (self.num_states, self.num_controls, 1), self.num_states, F)

    def rollout(self, x0, U, dt, out=None):
        """X[k+1] = F(X[k], U[k], dt).  x0 (13, B); U (H, 7, B) -> X (H+1, 13, B).
        The batched form of Controller.initialise (reference main/control/control.py:72-93)."""
        lib = self._sync()
        torch = _torch()
        X0, npx, vec = self._in(x0, self.num_states, "x0")
        B = X0.shape[1]
        from_np = not isinstance(U, torch.Tensor)
        Ut = torch.as_tensor(np.asarray(U, dtype=np.float32) if from_np else U)
        if vec and Ut.dim() == 2:
            Ut = Ut.unsqueeze(-1)
        if Ut.dim() != 3 or Ut.shape[1] not in (self.num_controls, _lib.NUM_CONTROLS) or Ut.shape[2] != B:
            raise ValueError(f"U: expected (H, {self.num_controls}, {B}), got {tuple(Ut.shape)}")
        Ut = Ut.to(device=X0.device, dtype=torch.float32)
        if Ut.shape[1] < _lib.NUM_CONTROLS:  # fewer controls than device rows: zero-fill (see _in_u)
            Ut = torch.cat([Ut, torch.zeros((Ut.shape[0], _lib.NUM_CONTROLS - Ut.shape[1], B), device=Ut.device)], dim=1)
        Ut = Ut.contiguous()
        H = Ut.shape[0]
        if out is None:
            out = torch.empty((H + 1, self.num_states, B), device=X0.device, dtype=torch.float32)
        else:
            assert out.shape == (H + 1, self.num_states, B) and out.is_contiguous() and out.dtype == torch.float32
        _lib.check(lib.ac_rollout_f32(self._handle, X0.data_ptr(), Ut.data_ptr() if H else None, C.c_float(float(dt)),
                                      B, H, out.data_ptr(), self._stream()), "ac_rollout_f32")
        if npx:
            res = out.cpu().numpy().astype(np.float64)
            return res[:, :, 0] if vec else res
        return out[:, :, 0] if vec else out

    def step_sens(self, x, u, dt, want_c=True, out=None):
        """(x+, A, B, c): the step and its Jacobians A = dF/dx (13,13,n), B = dF/du (13,7,n),
        c = dF/ddt (13,n) — what `ca.jacobian(state_update, .)` yields in the reference
        (control/aircraft.py:85-95; the defect rows of control/base.py:279-280)."""
        lib = self._sync()
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        n = X.shape[1]
        if U.shape[1] != n:
            raise ValueError("x and u must have the same number of columns")
        dts, dtp, keep = self._dt_args(dt, n)
        ns, nc = self.num_states, _lib.NUM_CONTROLS
        fresh = out is None
        if out is None:
            Xn = torch.empty_like(X)
            A = torch.empty((ns, ns, n), device=X.device, dtype=torch.float32)
            Bm = torch.empty((ns, nc, n), device=X.device, dtype=torch.float32)
            c = torch.empty((ns, n), device=X.device, dtype=torch.float32) if want_c else None
        else:
            Xn, A, Bm, c = out
        _lib.check(lib.ac_step_sens_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, Xn.data_ptr(),
                                        A.data_ptr(), Bm.data_ptr(), c.data_ptr() if c is not None else None,
                                        self._stream()), "ac_step_sens_f32")
        del keep
        if npx:
            cv = (lambda t: None if t is None else t.cpu().numpy().astype(np.float64))
            Xn, A, Bm, c = cv(Xn), cv(A), cv(Bm), cv(c)
        if fresh and self.num_controls < nc:
            Bm = Bm[:, : self.num_controls]  # the plugin's own controls; the remaining columns are zero
        if vec:
            Xn, A, Bm = Xn[..., 0], A[..., 0], Bm[..., 0]
            c = None if c is None else c[..., 0]
        return Xn, A, Bm, c

    def state_derivative_sens(self, x, u, out=None):
        """(x_dot, Fx, Fu): f(x, u) with Fx = df/dx (13,13,n) and Fu = df/du (13,7,n) — `ca.jacobian(state_derivative, .)`,
        which the reference's implicit defect row and Baumgarte row (control/base.py:282-304) and its LQR wrapper
        (dynamics/base.py:51-52) differentiate."""
        lib = self._sync()
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        n = X.shape[1]
        if U.shape[1] != n:
            raise ValueError("x and u must have the same number of columns")
        ns, nc = self.num_states, _lib.NUM_CONTROLS
        fresh = out is None
        if out is None:
            out = (torch.empty_like(X), torch.empty((ns, ns, n), device=X.device, dtype=torch.float32),
                   torch.empty((ns, nc, n), device=X.device, dtype=torch.float32))
        Xd, Fx, Fu = out
        _lib.check(lib.ac_state_derivative_sens_f32(self._handle, X.data_ptr(), U.data_ptr(), n, Xd.data_ptr(),
                                                    Fx.data_ptr(), Fu.data_ptr(), self._stream()),
                   "ac_state_derivative_sens_f32")
        if npx:
            Xd, Fx, Fu = (t.cpu().numpy().astype(np.float64) for t in (Xd, Fx, Fu))
        if fresh and self.num_controls < nc:
            Fu = Fu[:, : self.num_controls]
        if vec:
            Xd, Fx, Fu = Xd[..., 0], Fx[..., 0], Fu[..., 0]
        return Xd, Fx, Fu

    def step_hess(self, x, u, dt, lam, out=None):
        """Hessian of lam . F(x, u, dt) over z = (x[13], u[7], dt): (21, 21, n) — the block the defect rows contribute to
        the Lagrangian Hessian IPOPT evaluates as `nlp_hess_l` (control/base.py:279-280; todo.md:102).
        lam (13, n): multipliers of the rows of F.  Any number of RK4 sub-steps (composed per sub-step on the device)."""
        lib = self._sync()
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        L, _, _ = self._in(lam, self.num_states, "lam")
        n = X.shape[1]
        if U.shape[1] != n or L.shape[1] != n:
            raise ValueError("x, u and lam must have the same number of columns")
        dts, dtp, keep = self._dt_args(dt, n)
        if out is None:
            out = torch.empty((21, 21, n), device=X.device, dtype=torch.float32)
        self._reserve_hess(n)
        _lib.check(lib.ac_step_hess_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, L.data_ptr(), n,
                                        out.data_ptr(), self._stream()), "ac_step_hess_f32")
        del keep
        res = out.cpu().numpy().astype(np.float64) if npx else out
        return res[..., 0] if vec else res

    def _reserve_hess(self, n: int) -> None:
        """Size the handle's second-order workspace for n units.  Host-side and idempotent (the library only grows
        it); the compute calls themselves never allocate, so call this before capturing a hipGraph."""
        n = int(n)
        ns = int(self.physical_integration_substeps or 1)
        if ns != getattr(self, "_hess_reserved_substeps", ns):
            self._hess_reserved = 0  # the composition buffers are sized for the sub-step count
        self._hess_reserved_substeps = ns
        if n > getattr(self, "_hess_reserved", 0):
            torch = _torch()
            if torch.cuda.is_current_stream_capturing():
                raise _lib.AircraftHipError("second-order workspace must be reserved before stream capture: "
                                            "call system._reserve_hess(n) (ac_reserve_hess_workspace) first")
            self._sync()  # push the current sub-step count first: the reservation is sized for it
            _lib.check(_lib.load().ac_reserve_hess_workspace(self._handle, n), "ac_reserve_hess_workspace")
            self._hess_reserved = n

    # ---- reverse mode: vector-Jacobian products (include/aircraft_hip.h, ac_*_vjp_f32) ----------------------------------
    _VJP_KINDS = {"step": _lib.VJP_STEP, "rollout": _lib.VJP_ROLLOUT, "derivative": _lib.VJP_DERIVATIVE}

    def _set_vjp_route(self):
        lib = self._sync()
        if self.vjp_route not in _lib.VJP_ROUTES:
            raise ValueError(f"vjp_route: expected one of {sorted(_lib.VJP_ROUTES)}, got {self.vjp_route!r}")
        _lib.check(lib.ac_set_vjp_route(self._handle, _lib.VJP_ROUTES[self.vjp_route]), "ac_set_vjp_route")
        return lib

    def vjp_workspace(self, kind, n, H=0):
        """Device workspace the VJP of `kind` ("step", "rollout" with n = B, "derivative") needs on the current route, or
        None (the fused kernels need none).  Allocate it before capturing a graph and pass it as `ws=`."""
        lib = self._set_vjp_route()
        need = C.c_size_t()
        _lib.check(lib.ac_vjp_workspace_floats(self._handle, self._VJP_KINDS[kind], int(n), int(H), C.byref(need)),
                   "ac_vjp_workspace_floats")
        if need.value == 0:
            return None
        return _torch().empty(need.value, device=self._device_obj(), dtype=_torch().float32)

    def _vjp_ws(self, kind, n, H, ws):
        """-> (lib, workspace tensor or None, its size in floats); a caller's workspace is passed on as it is (the library
        checks its size)."""
        if ws is None:
            ws = self.vjp_workspace(kind, n, H)
        else:
            self._set_vjp_route()
        return _lib.load(), ws, (0 if ws is None else ws.numel())

    def step_vjp(self, x, u, dt, lam, ws=None):
        """Reverse mode of state_update: (x_bar, u_bar, dt_bar) = (A' lam, B' lam, c . lam) per unit — the gradient of
        sum(lam * F(x, u, dt)) without forming A, B, c.  lam (13, n); dt a scalar or (n,); dt_bar is per unit (n,).
        The route follows `self.vjp_route` ("auto", "fused", "composed"); `ws` is an optional pre-allocated workspace
        (vjp_workspace("step", n))."""
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        L, _, _ = self._in(lam, self.num_states, "lam")
        n = X.shape[1]
        if U.shape[1] != n or L.shape[1] != n:
            raise ValueError("x, u and lam must have the same number of columns")
        lib, ws, wsn = self._vjp_ws("step", n, 0, ws)
        dts, dtp, keep = self._dt_args(dt, n)
        Xb = torch.empty_like(X)
        Ub = torch.empty((_lib.NUM_CONTROLS, n), device=X.device, dtype=torch.float32)
        db = torch.empty((n,), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_step_vjp_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, L.data_ptr(), Xb.data_ptr(),
                                       Ub.data_ptr(), db.data_ptr(), ws.data_ptr() if ws is not None else None, wsn,
                                       self._stream()), "ac_step_vjp_f32")
        del keep
        Ub = Ub[: self.num_controls]
        if npx:
            Xb, Ub, db = (t.cpu().numpy().astype(np.float64) for t in (Xb, Ub, db))
        if vec:
            Xb, Ub, db = Xb[..., 0], Ub[..., 0], db[0]
        return Xb, Ub, db

    def _rollout_args(self, who, X, U, dt, G):
        """The saved rollout (X, U, dt, G) of the reverse sweeps as contiguous fp32 device tensors, U padded to the ABI's seven
        controls: -> (Xt (H+1, 13, B), Ut (H, 7, B), Gt, B, H, from_np)."""
        torch = _torch()
        dev = self._device_obj()
        from_np = not isinstance(X, torch.Tensor)

        def t3(a, name, rows):
            t = torch.as_tensor(np.asarray(a, dtype=np.float32) if not isinstance(a, torch.Tensor) else a)
            if t.dim() != 3 or t.shape[1] not in rows:
                raise ValueError(f"{name}: expected (., {rows[0]}, B), got {tuple(t.shape)}")
            return t.to(device=dev, dtype=torch.float32)

        Xt = t3(X, "X", (self.num_states,)).contiguous()
        Gt = t3(G, "G", (self.num_states,)).contiguous()
        Hp1, _, B = Xt.shape
        H = Hp1 - 1
        Ut = t3(U, "U", (self.num_controls, _lib.NUM_CONTROLS)) if H > 0 else torch.zeros((0, _lib.NUM_CONTROLS, B), device=dev)
        if Gt.shape != Xt.shape or Ut.shape[0] != H or Ut.shape[2] != B:
            raise ValueError(f"X {tuple(Xt.shape)}, U {tuple(Ut.shape)} and G {tuple(Gt.shape)} do not describe one rollout")
        if Ut.shape[1] < _lib.NUM_CONTROLS:
            Ut = torch.cat([Ut, torch.zeros((H, _lib.NUM_CONTROLS - Ut.shape[1], B), device=dev)], dim=1)
        if np.ndim(dt) > 0 or (isinstance(dt, torch.Tensor) and dt.numel() != 1):
            raise ValueError(f"{who}: dt must be a scalar (as in rollout)")
        return Xt, Ut.contiguous(), Gt, B, H, from_np

    def rollout_vjp(self, X, U, dt, G, ws=None):
        """Reverse mode of rollout: X (H+1, 13, B) the trajectory rollout() returned for (x0, U, dt), G (H+1, 13, B) the
        cotangent of every node -> (x0_bar (13, B), U_bar (H, num_controls, B), dt_bar (B,)).  dt is a scalar, as in
        rollout(); dt_bar is the per-instance sum over the nodes."""
        torch = _torch()
        dev = self._device_obj()
        Xt, Ut, Gt, B, H, from_np = self._rollout_args("rollout_vjp", X, U, dt, G)
        lib, ws, wsn = self._vjp_ws("rollout", B, H, ws)
        X0b = torch.empty((self.num_states, B), device=dev, dtype=torch.float32)
        Ub = torch.empty((H, _lib.NUM_CONTROLS, B), device=dev, dtype=torch.float32)
        db = torch.empty((B,), device=dev, dtype=torch.float32)
        _lib.check(lib.ac_rollout_vjp_f32(self._handle, Xt.data_ptr(), Ut.data_ptr() if H else None, C.c_float(float(dt)), B,
                                          H, Gt.data_ptr(), X0b.data_ptr(), Ub.data_ptr() if H else None, db.data_ptr(),
                                          ws.data_ptr() if ws is not None else None, wsn, self._stream()),
                   "ac_rollout_vjp_f32")
        Ub = Ub[:, : self.num_controls]
        if from_np:
            X0b, Ub, db = (t.cpu().numpy().astype(np.float64) for t in (X0b, Ub, db))
        return X0b, Ub, db

    def state_derivative_vjp(self, x, u, w, ws=None):
        """Reverse mode of state_derivative: (x_bar, u_bar) = ((df/dx)' w, (df/du)' w) per unit; w (13, n)."""
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        W, _, _ = self._in(w, self.num_states, "w")
        n = X.shape[1]
        if U.shape[1] != n or W.shape[1] != n:
            raise ValueError("x, u and w must have the same number of columns")
        lib, ws, wsn = self._vjp_ws("derivative", n, 0, ws)
        Xb = torch.empty_like(X)
        Ub = torch.empty((_lib.NUM_CONTROLS, n), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_state_derivative_vjp_f32(self._handle, X.data_ptr(), U.data_ptr(), n, W.data_ptr(), Xb.data_ptr(),
                                                   Ub.data_ptr(), ws.data_ptr() if ws is not None else None, wsn,
                                                   self._stream()), "ac_state_derivative_vjp_f32")
        Ub = Ub[: self.num_controls]
        if npx:
            Xb, Ub = (t.cpu().numpy().astype(np.float64) for t in (Xb, Ub))
        if vec:
            Xb, Ub = Xb[..., 0], Ub[..., 0]
        return Xb, Ub

    # ---- reverse mode to the weights of the MLP surrogate (include/aircraft_hip.h, ac_*_wgrad_*) -------------------------
    _WGRAD_KINDS = {"seeds": _lib.WGRAD_SEEDS, "step": _lib.WGRAD_STEP, "rollout": _lib.WGRAD_ROLLOUT}

    def mlp_folded_shape(self):
        """Widths [5, ..., 6] of the net as the handle holds it (activation-free layers folded into their successors)."""
        lib = self._sync()
        nl = C.c_int()
        widths = (C.c_int * (_lib.MAX_LAYERS + 1))()
        _lib.check(lib.ac_mlp_folded_shape(self._handle, C.byref(nl), widths), "ac_mlp_folded_shape")
        return [int(widths[i]) for i in range(nl.value + 1)]

    def mlp_grad_floats(self):
        """Length of the weight-gradient vector: per folded layer W[l] (nout, nin) row-major, then b[l]."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_mlp_grad_floats(self._handle, C.byref(need)), "ac_mlp_grad_floats")
        return int(need.value)

    def wgrad_workspace(self, kind, n, H=0):
        """Device workspace of the weight-gradient call `kind` ("seeds", "step", "rollout" with n = B).  Allocate it before
        capturing a graph and pass it as `ws=`."""
        return self._grad_workspace("ac_wgrad_workspace_floats", self._WGRAD_KINDS[kind], n, H)

    def _grad_workspace(self, getter, which, n, H):
        """A device workspace of the size the ABI's `getter` (ac_{wgrad,cgrad,agrad}_workspace_floats) reports; never empty."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(getattr(lib, getter)(self._handle, which, int(n), int(H), C.byref(need)), getter)
        return _torch().empty(max(int(need.value), 1), device=self._device_obj(), dtype=_torch().float32)

    def _wgrad_units(self, x, u, lam):
        X, _, _ = self._in(x, self.num_states, "x")
        U, _, _ = self._in_u(u)
        L, _, _ = self._in(lam, self.num_states, "lam")
        n = X.shape[1]
        if U.shape[1] != n or L.shape[1] != n:
            raise ValueError("x, u and lam must have the same number of columns")
        return X, U, L, n

    def step_wgrad_seeds(self, x, u, dt, lam, ws=None):
        """Per RK4 stage, the normalised network input Z (4, 5, n) and the cotangent Ybar (4, 6, n) of the raw network output
        for the loss sum(lam * F(x, u, dt)): the weight gradient of any surrogate evaluated at Z is its backward pass with
        Ybar (device tensors)."""
        torch = _torch()
        X, U, L, n = self._wgrad_units(x, u, lam)
        if ws is None:
            ws = self.wgrad_workspace("seeds", n)
        lib = self._sync()
        dts, dtp, keep = self._dt_args(dt, n)
        Z = torch.empty((4, 5, n), device=X.device, dtype=torch.float32)
        Yb = torch.empty((4, 6, n), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_step_wgrad_seeds_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, L.data_ptr(), Z.data_ptr(),
                                               Yb.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "ac_step_wgrad_seeds_f32")
        del keep
        return Z, Yb

    def step_wgrad(self, x, u, dt, lam, ws=None, out=None):
        """Gradient of sum(lam * F(x, u, dt)) over the weights of the folded MLP surrogate: a device tensor
        (mlp_grad_floats(),), per folded layer W[l] (nout, nin) row-major followed by b[l]."""
        torch = _torch()
        X, U, L, n = self._wgrad_units(x, u, lam)
        if ws is None:
            ws = self.wgrad_workspace("step", n)
        lib = self._sync()
        dts, dtp, keep = self._dt_args(dt, n)
        if out is None:
            out = torch.empty((self.mlp_grad_floats(),), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_step_wgrad_f32(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, L.data_ptr(), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), self._stream()), "ac_step_wgrad_f32")
        del keep
        return out

    def rollout_wgrad(self, X, U, dt, G, ws=None, out=None):
        """Gradient of sum(G * X) over the weights of the folded MLP surrogate, X (H+1, 13, B) the trajectory rollout()
        returned for (x0, U, dt) and G (H+1, 13, B) the cotangent of every node: the layout of step_wgrad."""
        torch = _torch()
        dev = self._device_obj()
        Xt, Ut, Gt, B, H, _ = self._rollout_args("rollout_wgrad", X, U, dt, G)
        if ws is None:
            ws = self.wgrad_workspace("rollout", B, H)
        lib = self._sync()
        if out is None:
            out = torch.empty((self.mlp_grad_floats(),), device=dev, dtype=torch.float32)
        _lib.check(lib.ac_rollout_wgrad_f32(self._handle, Xt.data_ptr(), Ut.data_ptr() if H else None, C.c_float(float(dt)), B, H,
                                            Gt.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "ac_rollout_wgrad_f32")
        return out

    # ---- reverse mode to the coefficients of the cubic-fit / linear model (include/aircraft_hip.h, ac_*_cgrad_*) ----------
    _CGRAD_KINDS = {"step": _lib.CGRAD_STEP, "rollout": _lib.CGRAD_ROLLOUT}

    def coef_grad_floats(self):
        """Length of the coefficient-gradient vector: 210 (poly: coef (6, 34) row-major, then intercept (6,)) or 36 (linear:
        W (6, 6) row-major)."""
        lib = self._sync()
        need = C.c_size_t()
        _lib.check(lib.ac_coef_grad_floats(self._handle, C.byref(need)), "ac_coef_grad_floats")
        return int(need.value)

    def set_coef_grad_grid(self, max_workgroups=0):
        """Cap the workgroups of the coefficient-gradient kernels (0: the handle's own choice).  The partial sums, and with them
        the last bits of the result, follow the grid: size the workspace after this call."""
        lib = self._sync()
        _lib.check(lib.ac_set_cgrad_grid(self._handle, int(max_workgroups)), "ac_set_cgrad_grid")

    def coef_grad_workspace(self, kind, n, H=0):
        """Device workspace of the coefficient-gradient call `kind` ("step", "rollout" with n = B).  Allocate it before
        capturing a graph and pass it as `ws=`."""
        return self._grad_workspace("ac_cgrad_workspace_floats", self._CGRAD_KINDS[kind], n, H)

    def _step_param_grad(self, call, floats, workspace, x, u, dt, lam, ws, out, need):
        """One recording reverse sweep over n units (ac_step_cgrad_f32, ac_step_agrad_f32): -> (parameter gradient (floats,),
        x_bar, u_bar, dt_bar); need = (x, u, dt): an output that is not needed is not written and comes back as None."""
        torch = _torch()
        X, U, L, n = self._wgrad_units(x, u, lam)
        if ws is None:
            ws = workspace("step", n)
        lib = self._sync()
        dts, dtp, keep = self._dt_args(dt, n)
        if out is None:
            out = torch.empty((floats(),), device=X.device, dtype=torch.float32)
        Xb = torch.empty_like(X) if need[0] else None
        Ub = torch.empty((_lib.NUM_CONTROLS, n), device=X.device, dtype=torch.float32) if need[1] else None
        db = torch.empty((n,), device=X.device, dtype=torch.float32) if need[2] else None
        ptr = [t.data_ptr() if t is not None else None for t in (Xb, Ub, db)]
        _lib.check(getattr(lib, call)(self._handle, X.data_ptr(), U.data_ptr(), dts, dtp, n, L.data_ptr(), ptr[0], ptr[1], ptr[2],
                                      out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()), call)
        del keep
        return out, Xb, (Ub[: self.num_controls] if Ub is not None else None), db

    def _rollout_param_grad(self, who, call, floats, workspace, X, U, dt, G, ws, out, need):
        """The same over a saved rollout (ac_rollout_cgrad_f32, ac_rollout_agrad_f32): -> (parameter gradient, x0_bar (13, B),
        U_bar (H, num_controls, B), dt_bar (B,))."""
        torch = _torch()
        dev = self._device_obj()
        Xt, Ut, Gt, B, H, _ = self._rollout_args(who, X, U, dt, G)
        if ws is None:
            ws = workspace("rollout", B, H)
        lib = self._sync()
        if out is None:
            out = torch.empty((floats(),), device=dev, dtype=torch.float32)
        X0b = torch.empty((self.num_states, B), device=dev, dtype=torch.float32) if need[0] else None
        Ub = torch.empty((H, _lib.NUM_CONTROLS, B), device=dev, dtype=torch.float32) if need[1] else None
        db = torch.empty((B,), device=dev, dtype=torch.float32) if need[2] else None
        ptr = [t.data_ptr() if t is not None and t.numel() else None for t in (X0b, Ub, db)]
        _lib.check(getattr(lib, call)(self._handle, Xt.data_ptr(), Ut.data_ptr() if H else None, C.c_float(float(dt)), B, H,
                                      Gt.data_ptr(), ptr[0], ptr[1], ptr[2], out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      self._stream()), call)
        return out, X0b, (Ub[:, : self.num_controls] if Ub is not None else None), db

    def step_coef_grad(self, x, u, dt, lam, ws=None, out=None, need=(True, True, True)):
        """Gradient of sum(lam * F(x, u, dt)) over the coefficients of the cubic-fit or linear model, and in the same sweep the
        per-unit (x_bar, u_bar, dt_bar) of step_vjp: -> (theta_bar (coef_grad_floats(),), x_bar, u_bar, dt_bar), device
        tensors.  need = (x, u, dt): an output that is not needed is not written and comes back as None."""
        return self._step_param_grad("ac_step_cgrad_f32", self.coef_grad_floats, self.coef_grad_workspace, x, u, dt, lam, ws, out,
                                     need)

    def rollout_coef_grad(self, X, U, dt, G, ws=None, out=None, need=(True, True, True)):
        """Gradient of sum(G * X) over the coefficients of the cubic-fit or linear model, X (H+1, 13, B) the trajectory rollout()
        returned for (x0, U, dt), and in the same sweep the outputs of rollout_vjp:
        -> (theta_bar, x0_bar (13, B), U_bar (H, num_controls, B), dt_bar (B,)); need = (x0, U, dt) as in step_coef_grad."""
        return self._rollout_param_grad("rollout_coef_grad", "ac_rollout_cgrad_f32", self.coef_grad_floats,
                                        self.coef_grad_workspace, X, U, dt, G, ws, out, need)

    # ---- reverse mode to mass, inertia, inertia_inv and com (include/aircraft_hip.h, ac_*_agrad_*) -----------
    def airframe_grad_workspace(self, kind, n, H=0):
        """Device workspace of the airframe-gradient call `kind` ("step", "rollout" with n = B).  Allocate it before capturing a
        graph and pass it as `ws=`."""
        return self._grad_workspace("ac_agrad_workspace_floats", self._CGRAD_KINDS[kind], n, H)

    def step_airframe_grad(self, x, u, dt, lam, ws=None, out=None, need=(True, True, True)):
        """Gradient of sum(lam * F(x, u, dt)) over the 22 airframe floats the kernels read, each as an independent number —
        mass, inertia (9, row-major), inertia_inv (9), com (3) — and in the same sweep the per-unit outputs of step_vjp:
        -> (phi_bar (22,), x_bar, u_bar, dt_bar), device tensors; need = (x, u, dt) as in step_coef_grad.  The default, linear
        and cubic-fit models; autodiff.AirframeParameters carries phi_bar back to mass, (Ixx, Iyy, Izz, Ixz) and com."""
        return self._step_param_grad("ac_step_agrad_f32", lambda: _lib.AIRFRAME_GRAD_FLOATS, self.airframe_grad_workspace, x, u, dt,
                                     lam, ws, out, need)

    def rollout_airframe_grad(self, X, U, dt, G, ws=None, out=None, need=(True, True, True)):
        """Gradient of sum(G * X) over the 22 airframe floats (see step_airframe_grad), X (H+1, 13, B) the trajectory rollout()
        returned for (x0, U, dt): -> (phi_bar (22,), x0_bar (13, B), U_bar (H, num_controls, B), dt_bar (B,))."""
        return self._rollout_param_grad("rollout_airframe_grad", "ac_rollout_agrad_f32", lambda: _lib.AIRFRAME_GRAD_FLOATS,
                                        self.airframe_grad_workspace, X, U, dt, G, ws, out, need)

    # ---- getters (reference dynamics/base.py:147-278, aircraft.py:255-330) ------------------------
    def _aero(self, x, u):
        lib = self._sync()
        torch = _torch()
        X, npx, vec = self._in(x, self.num_states, "x")
        if u is None:
            U = torch.zeros((_lib.NUM_CONTROLS, X.shape[1]), device=X.device, dtype=torch.float32)
        else:
            U, _, _ = self._in_u(u)
        n = X.shape[1]
        out = torch.empty((_lib.AERO_ROWS, n), device=X.device, dtype=torch.float32)
        _lib.check(lib.ac_aero_f32(self._handle, X.data_ptr(), U.data_ptr(), n, out.data_ptr(), self._stream()),
                   "ac_aero_f32")
        return out, npx, vec

    def _getter(self, name, rows):
        def fn(x, u=None):
            out, npx, vec = self._aero(x, u)
            return self._out(out[rows], npx, vec)

        dim = (rows.stop - rows.start) if isinstance(rows, slice) else 1
        return BatchedFunction(name, (self.num_states, self.num_controls), dim, fn)

    v_frd_rel = property(lambda self: self._getter("v_frd_rel", slice(0, 3)))
    airspeed = property(lambda self: self._getter("airspeed", 3))
    alpha = property(lambda self: self._getter("alpha", 4))
    beta = property(lambda self: self._getter("beta", 5))
    qbar = property(lambda self: self._getter("qbar", 6))
    coefficients = property(lambda self: self._getter("coefficients", slice(7, 13)))
    forces_frd = property(lambda self: self._getter("forces_frd", slice(13, 16)))
    moments_frd = property(lambda self: self._getter("moments_frd", slice(16, 19)))

    # Euler angles of the attitude (reference base.py:179-195); state-only getters f(x)
    phi = property(lambda self: self._getter("phi", 19))
    theta = property(lambda self: self._getter("theta", 20))
    psi = property(lambda self: self._getter("psi", 21))

    def hidden_route_in_use(self):
        """(route, gate) of the handle's net: route "f16" / "bf16" for the width-128 matrix-core sensitivity kernels ("auto":
        the net has none), gate = the range gate's verdict (0 passes, see ac_hidden_route_of; -1 no such kernels)."""
        lib = self._sync()
        r, g = C.c_int(), C.c_int()
        _lib.check(lib.ac_hidden_route_of(self._handle, C.byref(r), C.byref(g)), "ac_hidden_route_of")
        return {v: k for k, v in _lib.HIDDEN_ROUTES.items()}[r.value], g.value

    def last_launch(self):
        """(kernel name, grid, block, dynamic LDS bytes) of the most recent dispatch."""
        name = C.create_string_buffer(64)
        g, b, l = C.c_int(), C.c_int(), C.c_int()
        _lib.load().ac_last_launch(self._handle, name, 64, C.byref(g), C.byref(b), C.byref(l))
        return name.value.decode(), g.value, b.value, l.value
