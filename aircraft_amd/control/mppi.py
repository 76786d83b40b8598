"""Batched MPPI (model-predictive path-integral control) on top of the plain rollout engines.

The derivative-free sibling of the sweep in ilqr.py: per instance, K perturbed control sequences are drawn around the nominal
(ac_mppi_sample_f32, noise generated in the kernel), rolled out with the plain rollout engine, scored with the problem's own
cost kernels, and blended by exp(-cost / temperature) (ac_mppi_update_f32).  No derivatives, so the stall sigmoid, hard clips,
non-smooth losses and the wide nets cost no more than their forward rollout.  The problem — an `ILQR`, `GoalAcquisition` or
`MHTT` object — supplies the system, the horizon, the control box and the loss; everything stays on the device and torch
supplies the buffers only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Sequence

from .. import _lib


def _torch():
    import torch

    return torch


class MPPI:
    def __init__(self, problem, samples: int = 1024, sigma: Sequence[float] = (1, 1, 1, 0, 0, 0, 0), temperature: float = 1.0,
                 seed: int = 0, keep_nominal: bool = True, accept: bool = True, instance_offset: int = 0):
        """problem: an object of the ILQR family (system, dt, num_nodes, cost.u_min / u_max, rollout, trajectory_cost,
        envelope_cost).  samples: K candidates per instance and iteration.  sigma: std of the control noise per row, in the
        row's units (0: the row is not sampled).  temperature: lambda of exp(-J / lambda).  keep_nominal: candidate 0 is the
        unperturbed nominal.  accept: keep the blended controls only where they beat the current iterate (the history of
        `solve` is then non-increasing, like the sweep's); False takes them unconditionally (textbook MPPI).
        instance_offset: global index of local instance 0, for a batch that is one shard of a larger one (the noise of an
        instance depends on its global index only)."""
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
            raise ValueError("samples: an integer >= 1")
        try:
            sg = [float(s) for s in sigma]
        except TypeError:
            raise ValueError("sigma: seven numbers >= 0") from None
        if len(sg) != 7 or not all(math.isfinite(s) and s >= 0.0 for s in sg):
            raise ValueError("sigma: seven finite numbers >= 0")
        if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
            raise ValueError("temperature: a finite number > 0")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise ValueError("seed: an integer in [0, 2^64)")
        if isinstance(instance_offset, bool) or not isinstance(instance_offset, int) or not 0 <= instance_offset < 2 ** 32:
            raise ValueError("instance_offset: an integer in [0, 2^32)")
        for name in ("system", "dt", "num_nodes", "cost", "rollout", "trajectory_cost"):
            if not hasattr(problem, name):
                raise ValueError(f"problem: an ILQR, GoalAcquisition or MHTT object (no `{name}`)")
        if getattr(problem, "time_row", 0) != 0:
            raise ValueError("MPPI needs a fixed-time problem (time='fixed'): the rollout integrates at the fixed dt")
        u_min, u_max = [float(v) for v in problem.cost.u_min], [float(v) for v in problem.cost.u_max]
        if len(u_min) != 7 or len(u_max) != 7 or not all(a <= b for a, b in zip(u_min, u_max)):
            raise ValueError("problem.cost: u_min <= u_max, seven rows each")
        self.problem = problem
        self.samples, self.sigma, self.temperature, self.seed = samples, sg, float(temperature), seed
        self.keep_nominal, self.accept_improving, self.instance_offset = bool(keep_nominal), bool(accept), instance_offset
        o = _lib.MppiOpts()
        o.sigma[:], o.u_min[:], o.u_max[:] = sg, u_min, u_max
        o.lambda_, o.seed, o.instance_offset, o.keep_nominal = self.temperature, seed, instance_offset, int(self.keep_nominal)
        self._opts = o
        self._mws = None
        self.last_stats = None

    def __getattr__(self, name):  # everything MPPI does not define is the problem's (RecedingHorizon reads it through here)
        if name == "problem":
            raise AttributeError(name)
        return getattr(self.problem, name)

    # ---- device workspace (allocated once per (B, K, H)) ------------------------------------------------
    def _workspace(self, B, dev):
        torch = _torch()
        K, H = self.samples, self.problem.num_nodes
        key = (B, K, H, str(dev))
        if self._mws is None or self._mws["key"] != key:
            f = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)  # noqa: E731
            n = C.c_size_t(0)
            lib = self.system._sync()
            _lib.check(lib.ac_mppi_workspace_floats(self.system._handle, K, B, H, C.byref(n)), "ac_mppi_workspace_floats")
            self._mws = dict(key=key, Uc=f(H, 7, K * B), X0c=f(13, K * B), Xc=f(H + 1, 13, K * B), Jc=f(K * B), w=f(max(n.value, 1)),
                             Un=f(H, 7, B), Xn=f(H + 1, 13, B), Jn=f(B), J0=f(B), Ja=f(B), stats=f(4, B),
                             improved=torch.empty((B,), device=dev, dtype=torch.bool),
                             it=torch.zeros((1,), device=dev, dtype=torch.int32))
            if hasattr(self.problem, "progress"):  # MHTT: candidate progress from the tiled s0
                self._mws.update(s0c=f(K * B), Sc=f(H + 1, K * B), Sn=f(H + 1, B))
            self.last_stats = self._mws["stats"]
            if hasattr(self.problem, "_goal_ws"):
                self.problem._goal_ws(B, dev)
        return self._mws

    @property
    def iteration(self):
        """The device iteration counter (one int32), or None before the first workspace."""
        return self._mws["it"] if self._mws is not None else None

    def set_iteration(self, it: int = 0):
        """Set the device iteration counter (the `it` of the noise counter); the buffer is kept, so a captured graph sees it."""
        if self._mws is None:
            raise ValueError("set_iteration: no workspace yet (call sample / iterate / solve first)")
        self._mws["it"].fill_(int(it))

    # ---- the two kernels ------------------------------------------------------------------------------------
    def _check_U(self, U, what="U"):
        if U.dim() != 3 or U.shape[0] != self.problem.num_nodes or U.shape[1] != 7:
            raise ValueError(f"{what}: expected ({self.problem.num_nodes}, 7, B), got {tuple(U.shape)}")
        if U.dtype != _torch().float32 or not U.is_contiguous():
            raise ValueError(f"{what}: a contiguous float32 tensor")

    def sample(self, U, x0=None, out=None):
        """K candidates per instance around U (H, 7, B): Uc (H, 7, K*B), column k*B + b, and — when x0 (13, B) is given —
        its K-fold tiling X0c (13, K*B)."""
        torch = _torch()
        self._check_U(U)
        H, B, K = U.shape[0], U.shape[2], self.samples
        if x0 is not None and (tuple(x0.shape) != (13, B) or x0.dtype != torch.float32 or not x0.is_contiguous()):
            raise ValueError(f"x0: expected a contiguous float32 (13, {B})")
        lib = self.system._sync()
        ws = self._workspace(B, U.device)
        Uc, X0c = out if out is not None else (torch.empty((H, 7, K * B), device=U.device),
                                               torch.empty((13, K * B), device=U.device) if x0 is not None else None)
        _lib.check(lib.ac_mppi_sample_f32(self.system._handle, C.byref(self._opts), ws["it"].data_ptr(), U.data_ptr(),
                                          x0.data_ptr() if x0 is not None else None, K, B, H, Uc.data_ptr(),
                                          X0c.data_ptr() if x0 is not None else None, self.system._stream()),
                   "ac_mppi_sample_f32")
        return Uc, (X0c if x0 is not None else None)

    def update(self, J, Uc, U, out=None):
        """Softmin blend of the candidates Uc (H, 7, K*B) with costs J (K*B,) around U (H, 7, B) -> (Unew (H, 7, B),
        stats (4, B): Jmin, effective sample size, finite costs, index of the cheapest).  Advances the iteration counter."""
        torch = _torch()
        self._check_U(U)
        H, B, K = U.shape[0], U.shape[2], self.samples
        if tuple(Uc.shape) != (H, 7, K * B) or J.numel() != K * B:
            raise ValueError(f"Uc: expected ({H}, 7, {K * B}) and J ({K * B},)")
        lib = self.system._sync()
        ws = self._workspace(B, U.device)
        Unew, stats = out if out is not None else (torch.empty_like(U), torch.empty((4, B), device=U.device))
        _lib.check(lib.ac_mppi_update_f32(self.system._handle, C.byref(self._opts), ws["it"].data_ptr(), J.data_ptr(),
                                          Uc.data_ptr(), U.data_ptr(), K, B, H, Unew.data_ptr(), stats.data_ptr(),
                                          ws["w"].data_ptr(), ws["w"].numel(), self.system._stream()), "ac_mppi_update_f32")
        return Unew, stats

    # ---- scoring: the problem's own loss -----------------------------------------------------------------------
    def _cost(self, X, U, out, S=None, s0=None):
        p = self.problem
        if hasattr(p, "progress"):  # MHTT sizes its own candidate buffers for len(alphas): score through its public calls
            p.loss(X, U, p.progress(X, s0, mode=1, out=S), out=out)
        else:
            p.trajectory_cost(X, U, out=out)
        if getattr(p, "envelope_weight", 0.0) > 0:
            p.envelope_cost(X, out)
        return out

    def candidate_cost(self, Xc, Uc, out=None):
        """Cost of every candidate column (K*B,)."""
        B = Uc.shape[2] // self.samples
        ws = self._workspace(B, Uc.device)
        out = ws["Jc"] if out is None else out
        if hasattr(self.problem, "progress"):
            ws["s0c"].view(self.samples, B).copy_(self.problem.s0[None, :].expand(self.samples, B))
            return self._cost(Xc, Uc, out, S=ws["Sc"], s0=ws["s0c"])
        return self._cost(Xc, Uc, out)

    def nominal_cost(self, X, U, out):
        ws = self._workspace(U.shape[2], U.device)
        if hasattr(self.problem, "progress"):
            return self._cost(X, U, out, S=ws["Sn"], s0=self.problem.s0)
        return self._cost(X, U, out)

    # ---- one iteration ----------------------------------------------------------------------------------------------
    def iterate(self, x0, X, U):
        """One MPPI iteration in place on (X, U): sample, roll out and cost the K*B candidates, update, roll out and cost the
        blend, accept.  Returns (cost (B,), improved (B,) bool).  Allocation-free after the first call at a given B."""
        p = self.problem
        B = U.shape[2]
        ws = self._workspace(B, U.device)
        self.sample(U, x0, out=(ws["Uc"], ws["X0c"]))
        p.rollout(ws["X0c"], ws["Uc"], out=ws["Xc"])
        self.candidate_cost(ws["Xc"], ws["Uc"], out=ws["Jc"])
        self.update(ws["Jc"], ws["Uc"], U, out=(ws["Un"], ws["stats"]))
        p.rollout(x0, ws["Un"], out=ws["Xn"])
        self.nominal_cost(ws["Xn"], ws["Un"], ws["Jn"])
        if not self.accept_improving:
            X.copy_(ws["Xn"]); U.copy_(ws["Un"])
            return ws["Jn"], ws["improved"].fill_(True)
        self.nominal_cost(X, U, ws["J0"])
        lib = self.system._sync()
        H = U.shape[0]
        _lib.check(lib.ac_ilqr_accept_f32(self.system._handle, ws["Jn"].data_ptr(), ws["J0"].data_ptr(), ws["Xn"].data_ptr(),
                                          ws["Un"].data_ptr(), 1, B, H, X.data_ptr(), U.data_ptr(), ws["Ja"].data_ptr(),
                                          ws["improved"].data_ptr(), self.system._stream()), "ac_ilqr_accept_f32")
        return ws["Ja"], ws["improved"]

    def solve(self, x0, U0, iters: int = 10):
        """Rollout from x0 with U0, then `iters` MPPI iterations.  Returns (X, U, cost history (iters+1, B))."""
        torch = _torch()
        self._check_U(U0, "U0")
        U = U0.clone()
        X = self.problem.rollout(x0, U)
        ws = self._workspace(U.shape[2], U.device)
        hist = [self.nominal_cost(X, U, ws["J0"]).clone()]
        for _ in range(iters):
            J, _ = self.iterate(x0, X, U)
            hist.append(J.clone())
        return X, U, torch.stack(hist)
