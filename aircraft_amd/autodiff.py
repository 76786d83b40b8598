"""Differentiable forms of the hot path: `step`, `rollout` and `state_derivative` as torch.autograd.Functions.

The forward passes are the library's own kernels (ac_step_f32, ac_rollout_f32, ac_state_derivative_f32); the backward passes
are its reverse-mode kernels (ac_step_vjp_f32, ac_rollout_vjp_f32, ac_state_derivative_vjp_f32), which take one
cotangent per unit.  A loss written in plain torch over the outputs then back-propagates to the states, the controls and dt:

    X = autodiff.rollout(ac, x0, U, dt)          # (H+1, 13, B), X[0] = x0
    loss = ((X[-1, :3] - goal) ** 2).sum()
    loss.backward()                              # U.grad, x0.grad (where they require grad)

Conventions: tensors only (NumPy arrays are refused: autograd cannot track them); outputs and gradients come back in the
dtype and on the device of the state input (the kernels compute in float32 on the handle's GPU); dt may be a Python number,
a 0-d tensor or, for `step`, a per-unit tensor (n,) — a tensor dt that requires grad receives one.  First order only:
differentiating a backward pass again raises.

With the MLP surrogate the loss also back-propagates to the network's weights:

    params = autodiff.MlpParameters(ac)          # a torch.nn.Module over the aircraft's net
    opt = torch.optim.Adam(params.parameters(), lr=1e-3)
    X = autodiff.rollout(ac, x0, U, dt, params=params)
    ((X - X_measured) ** 2).mean().backward()    # fills .grad of every weight and bias (ac_rollout_wgrad_f32)
    opt.step()                                   # the next forward pass re-installs the changed weights (params.sync())

With the cubic-fit ("poly") or the linear model it reaches the model's coefficients the same way, through
any number of RK4 sub-steps, and the backward pass is one fused sweep (ac_step_cgrad_f32 / ac_rollout_cgrad_f32) that yields
the state, control, dt and coefficient gradients together:

    params = autodiff.CoefficientParameters(ac)  # coef (6, 34) and intercept (6,), or W (6, 6)

With the default, the linear or the cubic-fit model it reaches the airframe's mass properties: one fused
sweep (ac_step_agrad_f32 / ac_rollout_agrad_f32) yields the gradient over the 22 floats the kernels read, and autograd carries
it back to the eight physical numbers:

    frame = autodiff.AirframeParameters(ac)      # mass (), inertia (4,) = (Ixx, Iyy, Izz, Ixz), com (3,)
    X = autodiff.rollout(ac, x0, U, dt, params=frame)          # or params=(CoefficientParameters(ac), frame)
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

__all__ = ["step", "rollout", "state_derivative", "MlpParameters", "CoefficientParameters", "AirframeParameters"]


class MlpParameters(torch.nn.Module):
    """The weights of an aircraft's MLP surrogate as torch Parameters: one float32 Parameter per weight matrix and bias of the
    net AS THE USER GAVE IT (activation-free layers included); the four scalers are buffers.  Passed as `params=` to `step` /
    `rollout`, a loss back-propagates into their `.grad`.

    The library runs the FOLDED net (every activation-free layer that is not the last merged into its successor, in float64:
    ac_set_mlp) and its weight-gradient kernels differentiate that; `folded()` performs the same fold in torch, so autograd
    carries the folded gradient back to the original tensors."""

    def __init__(self, ac):
        super().__init__()
        model = getattr(ac, "coefficient_model", None)
        if getattr(ac, "model_kind", None) != "nn" or model is None or not hasattr(model, "data"):
            raise ValueError("MlpParameters: the aircraft's coefficient model is not the MLP surrogate (coeff_model_type 'nn')")
        d = model.data
        self._ac = ac
        self.act = [int(a) for a in d.act]
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(w.copy())) for w in d.weights])
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(b.copy())) for b in d.biases])
        for name in ("input_mean", "input_std", "output_mean", "output_std"):
            self.register_buffer(name, torch.from_numpy(getattr(d, name).copy()))
        self._installed = self._versions()  # the aircraft holds exactly these values

    def _versions(self):
        return tuple((id(p), p._version) for p in self.parameters())

    def folded(self):
        """[(W, b), ...] of the folded net, float32 (the fold itself in float64: fold_linear_layers of the library)."""
        net = [(w.double(), b.double(), a) for w, b, a in zip(self.weights, self.biases, self.act)]
        l = 0
        while l + 1 < len(net):
            (Wa, ba, aa), (Wb, bb, ab) = net[l], net[l + 1]
            if aa:
                l += 1
                continue
            net[l:l + 2] = [(Wb @ Wa, Wb @ ba + bb, ab)]
        return [(W.float(), b.float()) for W, b, _ in net]

    def flat(self):
        """The folded net in the layout of the weight-gradient vector: per layer W (nout, nin) row-major, then b."""
        return torch.cat([t.reshape(-1) for W, b in self.folded() for t in (W, b)])

    def sync(self):
        """Install the current parameter values in the aircraft (ac_set_mlp).  Called by `step` / `rollout` before a forward
        pass when a parameter changed since the last installation."""
        from .dynamics.base import _capturing
        from .utils import MlpData

        if _capturing():
            raise RuntimeError("MlpParameters.sync(): the weights changed and ac_set_mlp allocates and copies — not possible "
                               "while a stream is capturing; call params.sync() before the capture")
        ac, model = self._ac, self._ac.coefficient_model
        old = model.data
        model.data = MlpData([w.detach().cpu().numpy() for w in self.weights], [b.detach().cpu().numpy() for b in self.biases],
                             self.act, old.input_mean, old.input_std, old.output_mean, old.output_std)
        ac._sync()
        with torch.cuda.device(ac._device_obj()):
            model.install(ac._handle)
        self._installed = self._versions()

    def sync_if_changed(self):
        if self._versions() != self._installed:
            self.sync()


class CoefficientParameters(torch.nn.Module):
    """The coefficients of an aircraft's cubic-fit or linear model as float32 torch Parameters, copied from the model:
    `coef` (6, 34) and `intercept` (6,) for "poly", `W` (6, 6) (the last column the bias) for "linear".  Passed as `params=` to
    `step` / `rollout`, a loss back-propagates into their `.grad`."""

    def __init__(self, ac):
        super().__init__()
        kind, model = getattr(ac, "model_kind", None), getattr(ac, "coefficient_model", None)
        if kind not in ("poly", "linear") or model is None:
            raise ValueError("CoefficientParameters: the aircraft's coefficient model is neither the cubic fits "
                             "(coeff_model_type 'poly') nor the linear model ('linear')")
        self._ac, self.kind = ac, kind

        def par(a):
            return torch.nn.Parameter(torch.tensor(a, dtype=torch.float32))

        if kind == "poly":
            self.coef, self.intercept = par(model.coef), par(model.intercept)
        else:
            self.W = par(model.W)
        self._installed = self._versions()  # the aircraft holds exactly these values (its float32 rounding of the model data)

    def _versions(self):
        return tuple((id(p), p._version) for p in self.parameters())

    def flat(self):
        """The parameters in the layout of the coefficient-gradient vector (ac_coef_grad_floats): coef row-major then
        intercept, or W row-major."""
        if self.kind == "poly":
            return torch.cat([self.coef.reshape(-1), self.intercept.reshape(-1)])
        return self.W.reshape(-1)

    def sync(self):
        """Install the current parameter values in the aircraft through the model's own `install` (ac_set_poly rebuilds the
        gradient and second-derivative tables).  Called by `step` / `rollout` before a forward pass when a parameter changed
        since the last installation."""
        from .dynamics.base import _capturing

        if _capturing():
            raise RuntimeError("CoefficientParameters.sync(): the coefficients changed and installing them copies to the device "
                               "— not possible while a stream is capturing; call params.sync() before the capture")
        ac, model = self._ac, self._ac.coefficient_model
        for name in (("coef", "intercept") if self.kind == "poly" else ("W",)):
            setattr(model, name, getattr(self, name).detach().cpu().numpy().astype("float64"))
        ac._sync()
        with torch.cuda.device(ac._device_obj()):
            model.install(ac._handle)
        self._installed = self._versions()

    def sync_if_changed(self):
        if self._versions() != self._installed:
            self.sync()


class AirframeParameters(torch.nn.Module):
    """The mass properties of a fixed-wing aircraft as float32 torch Parameters, copied from the aircraft: `mass` (),
    `inertia` (4,) = (Ixx, Iyy, Izz, Ixz) about the reference point, `com` (3,).  Passed as `params=` to `step` / `rollout`
    (alone, or as the second entry of a tuple after a CoefficientParameters), a loss back-propagates into their `.grad`.

    The kernels read 22 derived floats (mass, inertia about the centre of mass, its inverse, com) and their gradient kernels
    differentiate those as independent numbers; `derived()` restates the derivation in torch, so autograd carries the raw
    gradient back to the eight physical numbers.  S, b, c and rudder_moment_arm are not parameters here."""

    def __init__(self, ac):
        super().__init__()
        kind = getattr(ac, "model_kind", None)
        if kind not in ("default", "linear", "poly") or not all(hasattr(ac, k) for k in ("Ixx", "Iyy", "Izz", "Ixz", "com")):
            raise ValueError("AirframeParameters: airframe gradients exist for a fixed-wing aircraft with the default, the linear "
                             f"or the cubic-fit model, not for {'the MLP surrogate' if kind == 'nn' else 'this model'} "
                             f"({type(ac).__name__}, model {kind!r})")
        self._ac = ac
        self.mass = torch.nn.Parameter(torch.tensor(float(ac.mass), dtype=torch.float32))
        self.inertia = torch.nn.Parameter(torch.tensor([float(ac.Ixx), float(ac.Iyy), float(ac.Izz), float(ac.Ixz)],
                                                       dtype=torch.float32))
        self.com = torch.nn.Parameter(torch.tensor([float(c) for c in ac.com], dtype=torch.float32))
        # the aircraft holds its own float64 numbers, not their float32 rounding, until the first sync(): never "installed"
        self._installed = None

    def _versions(self):
        return tuple((id(p), p._version) for p in self.parameters())

    def derived(self):
        """The 22 floats of ac_params that enter f, in the order of the airframe-gradient vector (AC_AIRFRAME_GRAD_FLOATS):
        mass, I = I0 + m K(com) row-major, I^-1 row-major, com — float64 (inertia_about_com and its inverse, restated)."""
        m, (ixx, iyy, izz, ixz), (x, y, z) = self.mass.double(), self.inertia.double(), self.com.double()
        o = torch.zeros((), dtype=torch.float64, device=m.device)
        I0 = torch.stack([ixx, o, ixz, o, iyy, o, ixz, o, izz]).reshape(3, 3)
        K = torch.stack([y * y + z * z, -x * y, -x * z, -y * x, x * x + z * z, -y * z, -z * x, -z * y, x * x + y * y]).reshape(3, 3)
        I = I0 + m * K
        return torch.cat([m.reshape(1), I.reshape(9), torch.linalg.inv(I).reshape(9), self.com.double()])

    def sync(self):
        """Write the current values into the aircraft's attributes (mass, Ixx, Iyy, Izz, Ixz, com); its own _sync() then sends
        the constants (ac_set_params).  Called by `step` / `rollout` before a forward pass when a parameter changed."""
        from .dynamics.aircraft import inertia_about_com
        from .dynamics.base import _capturing
        import numpy as np

        if _capturing():
            raise RuntimeError("AirframeParameters.sync(): the constants changed and ac_set_params copies to the device — not "
                               "possible while a stream is capturing; call params.sync() before the capture")
        m = float(self.mass.detach())
        ixx, iyy, izz, ixz = (float(v) for v in self.inertia.detach().cpu())
        com = self.com.detach().cpu().numpy().astype(np.float64)
        if not (np.isfinite(m) and m > 0.0):
            raise ValueError(f"AirframeParameters.sync(): mass must be positive, got {m}")
        I = inertia_about_com(ixx, iyy, izz, ixz, m, com)
        if not (np.isfinite(I).all() and np.linalg.eigvalsh(I).min() > 0.0):
            raise ValueError("AirframeParameters.sync(): the inertia tensor about the centre of mass is not positive definite: "
                             f"{I.tolist()}")
        ac = self._ac
        ac.mass, ac.Ixx, ac.Iyy, ac.Izz, ac.Ixz, ac.com = m, ixx, iyy, izz, ixz, com
        ac._sync()
        self._installed = self._versions()

    def sync_if_changed(self):
        if self._versions() != self._installed:
            self.sync()


def _theta(ac, params):
    """-> (theta, phi, coef): theta the flattened MLP or coefficient parameters, phi the airframe's derived 22-vector (autograd
    inputs, or None), coef True where theta belongs to a CoefficientParameters — after making sure the aircraft runs on the
    current values"""
    if params is None:
        return None, None, False
    parts = params if isinstance(params, tuple) else (params,)
    pair = len(parts) == 2 and isinstance(parts[0], CoefficientParameters) and isinstance(parts[1], AirframeParameters)
    if not pair and (isinstance(params, tuple) or not isinstance(params, (MlpParameters, CoefficientParameters, AirframeParameters))):
        raise TypeError("params: expected an MlpParameters, a CoefficientParameters, an AirframeParameters or a tuple "
                        f"(CoefficientParameters, AirframeParameters), got {type(params).__name__}"
                        + (f" of ({', '.join(type(q).__name__ for q in parts)})" if isinstance(params, tuple) else ""))
    theta = phi = None
    for q in parts:
        if q._ac is not ac:
            raise ValueError(f"params: this {type(q).__name__} was built from another aircraft")
        q.sync_if_changed()
        if isinstance(q, AirframeParameters):
            phi = q.derived()
        else:
            theta = q.flat()
    return theta, phi, isinstance(parts[0], CoefficientParameters)


def _tensor(a, name):
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(a).__name__} (aircraft_amd.autodiff is tensor-only; "
                        "use SixDOF.step_vjp / rollout_vjp for NumPy)")
    return a


def _dt(dt, n, per_unit_ok):
    """-> (value handed to the kernels, tensor or None)"""
    if isinstance(dt, torch.Tensor):
        if dt.numel() == 1:
            return float(dt.detach().reshape(())), dt
        if not per_unit_ok:
            raise ValueError("rollout: dt must be a scalar")
        if dt.dim() != 1 or dt.numel() != n:
            raise ValueError(f"dt: expected a scalar or ({n},), got {tuple(dt.shape)}")
        return dt.detach(), dt
    if hasattr(dt, "__array__") or isinstance(dt, (list, tuple)):
        raise TypeError("dt: expected a Python number or a torch.Tensor")
    return float(dt), None


def _check_states(ac, x, rows, name):
    if x.dim() not in (1, 2) or x.shape[0] != rows:
        raise ValueError(f"{name}: expected ({rows}, n) or ({rows},), got {tuple(x.shape)}")


def _grad_like(g, ref):
    if g is not None and g.shape[-ref.dim():] != ref.shape:  # a 7-row control buffer of a plugin with fewer controls
        pad = list(ref.shape)
        pad[-ref.dim()] = ref.shape[-ref.dim()] - g.shape[-ref.dim()]
        g = torch.cat([g, g.new_zeros(pad)], dim=-ref.dim())
    return None if g is None else g.to(device=ref.device, dtype=ref.dtype)


def _dt_grad(gdt, dt_t):
    """dt_bar per unit (n,) -> the gradient of the dt the caller passed (a scalar sums the units)."""
    if dt_t is None:
        return None
    g = gdt.sum() if dt_t.numel() == 1 else gdt
    return g.reshape(dt_t.shape).to(device=dt_t.device, dtype=dt_t.dtype)


class _Step(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, dt_t, theta, phi, ac, dt_val, coef):
        ctx.ac, ctx.dt_val, ctx.coef = ac, dt_val, coef
        ctx.save_for_backward(x, u, dt_t, theta, phi)
        y = ac.state_update(x.detach(), u.detach(), dt_val)
        return y.to(device=x.device, dtype=x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, u, dt_t, theta, phi = ctx.saved_tensors
        need_x, need_u, need_dt, need_w, need_a = ctx.needs_input_grad[:5]
        xb = ub = db = wb = ab = None
        if need_w and ctx.coef:  # ONE fused sweep: the coefficient gradient and whichever of x, u, dt are needed
            wb, xb, ub, db = ctx.ac.step_coef_grad(x.detach(), u.detach(), ctx.dt_val, gy.contiguous(),
                                                   need=(need_x, need_u, need_dt))
            if x.dim() == 1:
                xb, ub, db = (None if t is None else t[..., 0] for t in (xb, ub, db))
            wb = wb.to(device=theta.device, dtype=theta.dtype)
            if need_a:  # (a second sweep for the airframe alone: its state outputs stay NULL)
                ab = ctx.ac.step_airframe_grad(x.detach(), u.detach(), ctx.dt_val, gy.contiguous(), need=(False, False, False))[0]
        elif need_a:  # ONE fused sweep: the airframe gradient and whichever of x, u, dt are needed
            ab, xb, ub, db = ctx.ac.step_airframe_grad(x.detach(), u.detach(), ctx.dt_val, gy.contiguous(),
                                                       need=(need_x, need_u, need_dt))
            if x.dim() == 1:
                xb, ub, db = (None if t is None else t[..., 0] for t in (xb, ub, db))
        else:
            if need_x or need_u or need_dt:
                xb, ub, db = ctx.ac.step_vjp(x.detach(), u.detach(), ctx.dt_val, gy.contiguous())
            if need_w:
                wb = ctx.ac.step_wgrad(x.detach(), u.detach(), ctx.dt_val, gy.contiguous()).to(device=theta.device, dtype=theta.dtype)
        if ab is not None:
            ab = ab.to(device=phi.device, dtype=phi.dtype)
        return (_grad_like(xb, x) if need_x else None, _grad_like(ub, u) if need_u else None,
                _dt_grad(db, dt_t) if need_dt else None, wb, ab, None, None, None)


class _Rollout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x0, U, dt_t, theta, phi, ac, dt_val, coef):
        ctx.ac, ctx.dt_val, ctx.coef = ac, dt_val, coef
        X = ac.rollout(x0.detach(), U.detach(), dt_val)  # float32 on the handle's device: saved as the kernels read it
        ctx.save_for_backward(x0, U, X, dt_t, theta, phi)
        return X.to(device=x0.device, dtype=x0.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        x0, U, X, dt_t, theta, phi = ctx.saved_tensors
        need_x, need_u, need_dt, need_w, need_a = ctx.needs_input_grad[:5]
        vec = x0.dim() == 1
        Xs, Us, G = (X, U, gX) if not vec else (X.unsqueeze(-1), U.unsqueeze(-1), gX.unsqueeze(-1))
        x0b = ub = db = wb = ab = None
        if need_w and ctx.coef:  # ONE fused sweep (see _Step.backward)
            wb, x0b, ub, db = ctx.ac.rollout_coef_grad(Xs, Us.detach(), ctx.dt_val, G.contiguous(), need=(need_x, need_u, need_dt))
            if vec:
                x0b, ub = (None if t is None else t[..., 0] for t in (x0b, ub))
            wb = wb.to(device=theta.device, dtype=theta.dtype)
            if need_a:
                ab = ctx.ac.rollout_airframe_grad(Xs, Us.detach(), ctx.dt_val, G.contiguous(), need=(False, False, False))[0]
        elif need_a:
            ab, x0b, ub, db = ctx.ac.rollout_airframe_grad(Xs, Us.detach(), ctx.dt_val, G.contiguous(),
                                                           need=(need_x, need_u, need_dt))
            if vec:
                x0b, ub = (None if t is None else t[..., 0] for t in (x0b, ub))
        else:
            if need_x or need_u or need_dt:
                x0b, ub, db = ctx.ac.rollout_vjp(Xs, Us.detach(), ctx.dt_val, G.contiguous())
                if vec:
                    x0b, ub, db = x0b[..., 0], ub[..., 0], db[0:1]
            if need_w:
                wb = ctx.ac.rollout_wgrad(Xs, Us.detach(), ctx.dt_val, G.contiguous()).to(device=theta.device, dtype=theta.dtype)
        if ab is not None:
            ab = ab.to(device=phi.device, dtype=phi.dtype)
        return (_grad_like(x0b, x0) if need_x else None, _grad_like(ub, U) if need_u else None,
                _dt_grad(db, dt_t) if need_dt else None, wb, ab, None, None, None)


class _Derivative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, ac):
        ctx.ac = ac
        ctx.save_for_backward(x, u)
        y = ac.state_derivative(x.detach(), u.detach())
        return y.to(device=x.device, dtype=x.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, u = ctx.saved_tensors
        need_x, need_u = ctx.needs_input_grad[:2]
        if not (need_x or need_u):
            return None, None, None
        xb, ub = ctx.ac.state_derivative_vjp(x.detach(), u.detach(), gy.contiguous())
        return _grad_like(xb, x) if need_x else None, _grad_like(ub, u) if need_u else None, None


def step(ac, x, u, dt, params=None):
    """x+ = F(x, u, dt) (SixDOF.state_update) with a grad_fn.  x (13, n) or (13,), u (num_controls, n), dt a number, a 0-d
    tensor or a per-unit tensor (n,).  params: an MlpParameters, a CoefficientParameters, an AirframeParameters or a tuple
    (CoefficientParameters, AirframeParameters) of `ac` — the loss then reaches the surrogate's weights, the coefficients of the
    cubic-fit / linear model, or mass, inertia and centre of mass, too."""
    _tensor(x, "x"); _tensor(u, "u")
    _check_states(ac, x, ac.num_states, "x")
    if u.dim() != x.dim() or u.shape[0] not in (ac.num_controls, 7) or u.shape[1:] != x.shape[1:]:
        raise ValueError(f"u: expected ({ac.num_controls},{' n' if x.dim() == 2 else ''}) matching x, got {tuple(u.shape)}")
    n = x.shape[1] if x.dim() == 2 else 1
    dt_val, dt_t = _dt(dt, n, per_unit_ok=True)
    theta, phi, coef = _theta(ac, params)
    return _Step.apply(x, u, dt_t, theta, phi, ac, dt_val, coef)


def rollout(ac, x0, U, dt, params=None):
    """X[k+1] = F(X[k], U[k], dt) (SixDOF.rollout) with a grad_fn.  x0 (13, B) or (13,), U (H, num_controls, B) or
    (H, num_controls), dt a number or a 0-d tensor -> X (H+1, 13, B).  params: as in `step`."""
    _tensor(x0, "x0"); _tensor(U, "U")
    _check_states(ac, x0, ac.num_states, "x0")
    if U.dim() != x0.dim() + 1 or U.shape[1] not in (ac.num_controls, 7) or U.shape[2:] != x0.shape[1:]:
        raise ValueError(f"U: expected (H, {ac.num_controls}, B) matching x0, got {tuple(U.shape)}")
    dt_val, dt_t = _dt(dt, 1, per_unit_ok=False)
    theta, phi, coef = _theta(ac, params)
    return _Rollout.apply(x0, U, dt_t, theta, phi, ac, dt_val, coef)


def state_derivative(ac, x, u):
    """x_dot = f(x, u) (SixDOF.state_derivative) with a grad_fn."""
    _tensor(x, "x"); _tensor(u, "u")
    _check_states(ac, x, ac.num_states, "x")
    if u.dim() != x.dim() or u.shape[0] not in (ac.num_controls, 7) or u.shape[1:] != x.shape[1:]:
        raise ValueError(f"u: expected ({ac.num_controls},{' n' if x.dim() == 2 else ''}) matching x, got {tuple(u.shape)}")
    return _Derivative.apply(x, u, ac)
