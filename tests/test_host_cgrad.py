"""The recording coefficient provider and the sub-step reverse sweep of the coefficient gradient (aircraft_amd/csrc/ac_cgrad.hpp)
compiled for the host with g++ (tests/host_cgrad/cgrad_host.cpp, -DAC_HOST_CHECK) and checked against float64 central
differences through the oracle (tests/cgrad_ref.py): every sample added into ONE fp32 chain per parameter, the least
favourable order.  Also the checks of aircraft_amd.autodiff.CoefficientParameters and of the ABI that need no device.

Measured here (g++ -ffp-contract=off), worst tensor error / agreement of the two reference steps:
  poly, 1 sub-step, dt 0.01, stall off / on     n = 1, 65, 130   <= 7.6e-7 / 1.3e-9
  linear, 1 sub-step, stall off                 n = 1, 65, 130   <= 6.6e-7 / 9.2e-8
  poly, 10 sub-steps, dt 0.1, stall off         n = 1, 65, 130   <= 3.8e-6 / 3.0e-7
  poly rollout B = 65, H = 12, dt 0.01 (nodes: the oracle's, rounded)  1.8e-6 / 7.6e-9"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import cgrad_ref as R
from tests.helpers import f32_exact, make_aircraft

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_cgrad")
SO = os.path.join(HERE, "libcgrad_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc")
FP = C.POINTER(C.c_float)


def _lib():
    src = os.path.join(HERE, "cgrad_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_dynamics.hpp", "ac_adjoint.hpp", "ac_vjp.hpp", "ac_cgrad.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        # -ffp-contract=off: the bar then holds for the least favourable (unfused) rounding
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SO, src], check=True)
    L = C.CDLL(SO)
    L.host_step_cgrad.restype = C.c_int
    L.host_step_cgrad.argtypes = [C.c_void_p, FP, FP, FP, FP, FP, FP, C.c_int, FP, C.c_long, FP, FP, FP, FP]
    L.host_rollout_cgrad.restype = C.c_int
    L.host_rollout_cgrad.argtypes = [C.c_void_p, FP, FP, FP, FP, FP, C.c_float, C.c_long, C.c_long, FP, FP, FP, FP, FP]
    return L


def _model_ptrs(ac):
    d = R.theta_of(ac)
    keep = [np.ascontiguousarray(d[k], dtype=np.float32) if k in d else None for k in ("W", "coef", "intercept")]
    return keep, [a.ctypes.data_as(FP) if a is not None else None for a in keep]


def _f32(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]


def host_step(ac, X, U, dt, lam):
    n = X.shape[1]
    p = ac._param_struct()
    keep, ptr = _model_ptrs(ac)
    Xf, Uf, Lf, Df = _f32(X, U, lam, np.atleast_1d(dt))
    Xb, Ub, db = np.zeros((13, n), np.float32), np.zeros((7, n), np.float32), np.zeros(n, np.float32)
    th = np.zeros(210 if ac.model_kind == "poly" else 36, np.float32)
    rc = _lib().host_step_cgrad(C.byref(p), *ptr, Xf.ctypes.data_as(FP), Uf.ctypes.data_as(FP), Df.ctypes.data_as(FP),
                                int(np.ndim(dt) > 0), Lf.ctypes.data_as(FP), n, Xb.ctypes.data_as(FP), Ub.ctypes.data_as(FP),
                                db.ctypes.data_as(FP), th.ctypes.data_as(FP))
    assert rc == 0, rc
    return R.split_theta(ac.model_kind, th), Xb, Ub, db


def host_rollout(ac, Xtraj, U, dt, G):
    H, _, B = U.shape
    p = ac._param_struct()
    keep, ptr = _model_ptrs(ac)
    Xf, Uf, Gf = _f32(Xtraj, U, G)
    X0b, Ub, db = np.zeros((13, B), np.float32), np.zeros((H, 7, B), np.float32), np.zeros(B, np.float32)
    th = np.zeros(210 if ac.model_kind == "poly" else 36, np.float32)
    rc = _lib().host_rollout_cgrad(C.byref(p), *ptr, Xf.ctypes.data_as(FP), Uf.ctypes.data_as(FP), float(dt), B, H,
                                   Gf.ctypes.data_as(FP), X0b.ctypes.data_as(FP), Ub.ctypes.data_as(FP), db.ctypes.data_as(FP),
                                   th.ctypes.data_as(FP))
    assert rc == 0, rc
    return R.split_theta(ac.model_kind, th)


CASES = {  # name -> (model, sub-steps, dt, stall)
    "poly": ("poly", 1, 0.01, False),
    "poly_stall": ("poly", 1, 0.01, True),
    "linear": ("linear", 1, 0.01, False),
    "poly_sub10": ("poly", 10, 0.1, False),
}
_REF = {}


def _reference(case, n, seed):
    """(units, per-unit reference), computed once per (case, pool)"""
    key = (case, n, seed)
    if key not in _REF:
        model, ns, dt, stall = CASES[case]
        ac = make_aircraft(model, normalise=True, substeps=ns, stall_scaling=stall)
        X, U, lam = R.units(n, seed)
        _REF[key] = (ac, X, U, lam, dt, R.step_reference(ac, X, U, dt, lam))
    return _REF[key]


@pytest.mark.parametrize("n,seed", [(1, 5), (65, 5), (130, 7)])
@pytest.mark.parametrize("case", list(CASES))
def test_step_coef_grad_on_host(case, n, seed):
    ac, X, U, lam, dt, refs = _reference(case, n, seed)
    want, agree = R.check_reference([R.summed(r) for r in refs])
    got, Xb, Ub, db = host_step(ac, X, U, dt, lam)
    errs = R.tensor_errors(got, want)
    print(f"[host cgrad] {case} n={n} errs {errs} reference agreement {agree}")
    assert max(errs.values()) < R.BAR, errs
    # the other outputs of the recording sweep are those of the plain one
    from tests.test_host_vjp import _run as plain_vjp

    Xp, Up, dp = plain_vjp(ac, 0, X, U, dt, lam)
    assert np.array_equal(Xb, Xp) and np.array_equal(Ub, Up) and np.array_equal(db, dp)


def test_rollout_coef_grad_on_host():
    ac = make_aircraft("poly", normalise=True)
    B, H, dt = 65, 12, 0.01
    X0, U, G = R.rollout_problem(B, H)
    want, agree = R.check_reference([R.summed(r) for r in R.rollout_reference(ac, X0, U, dt, G)])
    Xtraj = f32_exact(R.oracle_with(ac, R.theta_of(ac)).rollout(X0, U, dt))  # the saved nodes, as an fp32 rollout stores them
    errs = R.tensor_errors(host_rollout(ac, Xtraj, U, dt, G), want)
    print(f"[host cgrad] poly rollout B={B} H={H} errs {errs} reference agreement {agree}")
    assert max(errs.values()) < R.BAR, errs


def test_host_sweep_refuses_too_many_substeps_and_other_models():
    X, U, lam = R.units(2, 5)
    with pytest.raises(AssertionError):
        host_step(make_aircraft("poly", substeps=31), X, U, 0.1, lam)
    assert host_step(make_aircraft("poly", normalise=True, substeps=30), X, U, 0.1, lam)[0]["coef"].shape == (6, 34)


# ---- aircraft_amd.autodiff.CoefficientParameters: the checks that come before any device work ------------------------------------
def test_coefficient_parameters_shapes_and_refusals():
    import torch

    from aircraft_amd import Quadrotor, autodiff

    poly = make_aircraft("poly")
    p = autodiff.CoefficientParameters(poly)
    assert tuple(p.coef.shape) == (6, 34) and tuple(p.intercept.shape) == (6,) and p.coef.dtype == torch.float32
    assert len(list(p.parameters())) == 2 and tuple(p.flat().shape) == (210,)
    assert np.array_equal(p.flat().detach().numpy()[:204].reshape(6, 34), np.asarray(poly.coefficient_model.coef, np.float32))
    assert np.array_equal(p.flat().detach().numpy()[204:], np.asarray(poly.coefficient_model.intercept, np.float32))
    lin = make_aircraft("linear")
    q = autodiff.CoefficientParameters(lin)
    assert tuple(q.W.shape) == (6, 6) and tuple(q.flat().shape) == (36,)
    assert np.array_equal(q.flat().detach().numpy().reshape(6, 6), np.asarray(lin.coefficient_model.W, np.float32))
    for other in (make_aircraft("default"), make_aircraft("nn"), Quadrotor()):
        with pytest.raises(ValueError, match="CoefficientParameters"):
            autodiff.CoefficientParameters(other)
    with pytest.raises(ValueError):
        autodiff.MlpParameters(poly)  # (unchanged)
    x, u = torch.zeros(13, 2), torch.zeros(7, 2)
    with pytest.raises(TypeError, match="params"):
        autodiff.step(poly, x, u, 0.01, params=object())
    with pytest.raises(ValueError, match="another aircraft"):
        autodiff.step(lin, x, u, 0.01, params=p)


def test_cgrad_abi_is_exported():
    from aircraft_amd import _lib

    lib = _lib.load()
    for name in ("ac_coef_grad_floats", "ac_cgrad_workspace_floats", "ac_set_cgrad_grid", "ac_step_cgrad_f32", "ac_rollout_cgrad_f32"):
        assert getattr(lib, name) is not None
    n = C.c_size_t()
    assert lib.ac_coef_grad_floats(None, C.byref(n)) == -1
    assert lib.ac_cgrad_workspace_floats(None, 0, 1, 0, C.byref(n)) == -1
    assert lib.ac_set_cgrad_grid(None, 0) == -1
    assert lib.ac_step_cgrad_f32(None, None, None, C.c_float(0.01), None, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.ac_rollout_cgrad_f32(None, None, None, C.c_float(0.01), 1, 1, None, None, None, None, None, None, 0, None) == -1
