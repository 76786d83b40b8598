"""The recording airframe provider and the sub-step reverse sweep of the airframe gradient (aircraft_amd/csrc/ac_agrad.hpp)
compiled for the host with g++ (tests/host_agrad/agrad_host.cpp, -DAC_HOST_CHECK -ffp-contract=off) and checked against float64
central differences through the oracle (tests/agrad_ref.py): every sample added into ONE fp32 chain per parameter, the least
favourable order; the raw 22-vector goes through the autograd of AirframeParameters.derived() and is compared over the eight
physical numbers.  Also the checks of aircraft_amd.autodiff.AirframeParameters and of the ABI that need no device, and the
compiler's resource report of the new kernels.

Measured here (g++ -ffp-contract=off), worst group:
  summed, default / linear / poly (stall off and on) at one sub-step, poly at ten; n = 65, 130     <= 2.8e-7 (references agree to 7.9e-9)
  poly n = 4099                                                                                    7.7e-8
  poly rollout B = 65, H = 12, dt 0.01 (nodes: the oracle's, rounded)                              2.8e-7
  16 single units per case                                                                         <= 2.1e-5 (linear, mass)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import agrad_ref as R
from tests.helpers import f32_exact, make_aircraft

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_agrad")
SO = os.path.join(HERE, "libagrad_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc")
FP = C.POINTER(C.c_float)


def _lib():
    src = os.path.join(HERE, "agrad_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_dynamics.hpp", "ac_adjoint.hpp", "ac_vjp.hpp", "ac_cgrad.hpp",
                                                    "ac_agrad.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        # -ffp-contract=off: the bars then hold for the least favourable (unfused) rounding
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SO, src], check=True)
    L = C.CDLL(SO)
    L.host_step_agrad.restype = C.c_int
    L.host_step_agrad.argtypes = [C.c_void_p, FP, FP, FP, FP, FP, FP, C.c_int, FP, C.c_long, FP, FP, FP, FP]
    L.host_rollout_agrad.restype = C.c_int
    L.host_rollout_agrad.argtypes = [C.c_void_p, FP, FP, FP, FP, FP, C.c_float, C.c_long, C.c_long, FP, FP, FP, FP, FP]
    return L


def _model_ptrs(ac):
    m = ac.coefficient_model
    keep = [np.ascontiguousarray(getattr(m, k), dtype=np.float32) if k in R.TENSORS.get(ac.model_kind, ()) else None
            for k in ("W", "coef", "intercept")]
    return keep, [a.ctypes.data_as(FP) if a is not None else None for a in keep]


def _f32(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]


def host_step(ac, X, U, dt, lam, rc_only=False):
    """-> (raw gradient (22,), Xbar, Ubar, dtbar)"""
    n = X.shape[1]
    p = ac._param_struct()
    keep, ptr = _model_ptrs(ac)
    Xf, Uf, Lf, Df = _f32(X, U, lam, np.atleast_1d(dt))
    Xb, Ub, db = np.zeros((13, n), np.float32), np.zeros((7, n), np.float32), np.zeros(n, np.float32)
    phi = np.zeros(22, np.float32)
    rc = _lib().host_step_agrad(C.byref(p), *ptr, Xf.ctypes.data_as(FP), Uf.ctypes.data_as(FP), Df.ctypes.data_as(FP),
                                int(np.ndim(dt) > 0), Lf.ctypes.data_as(FP), n, Xb.ctypes.data_as(FP), Ub.ctypes.data_as(FP),
                                db.ctypes.data_as(FP), phi.ctypes.data_as(FP))
    if rc_only:
        return rc
    assert rc == 0, rc
    return phi, Xb, Ub, db


def host_rollout(ac, Xtraj, U, dt, G):
    H, _, B = U.shape
    p = ac._param_struct()
    keep, ptr = _model_ptrs(ac)
    Xf, Uf, Gf = _f32(Xtraj, U, G)
    X0b, Ub, db = np.zeros((13, B), np.float32), np.zeros((H, 7, B), np.float32), np.zeros(B, np.float32)
    phi = np.zeros(22, np.float32)
    rc = _lib().host_rollout_agrad(C.byref(p), *ptr, Xf.ctypes.data_as(FP), Uf.ctypes.data_as(FP), float(dt), B, H,
                                   Gf.ctypes.data_as(FP), X0b.ctypes.data_as(FP), Ub.ctypes.data_as(FP), db.ctypes.data_as(FP),
                                   phi.ctypes.data_as(FP))
    assert rc == 0, rc
    return phi


CASES = {  # name -> (model, sub-steps, dt, stall)
    "default": ("default", 1, 0.01, False),
    "linear": ("linear", 1, 0.01, False),
    "poly": ("poly", 1, 0.01, False),
    "poly_stall": ("poly", 1, 0.01, True),
    "poly_sub10": ("poly", 10, 0.1, False),
}
_REF = {}


def _reference(case, pool, seed):
    """(aircraft, units, dt, per-unit references), computed once per (case, pool)"""
    key = (case, pool, seed)
    if key not in _REF:
        model, ns, dt, stall = CASES[case]
        ac = R.aircraft(model, substeps=ns, stall_scaling=stall)
        X, U, lam = R.units(pool, seed)
        _REF[key] = (ac, X, U, lam, dt, R.step_reference(ac, X, U, dt, lam))
    return _REF[key]


@pytest.mark.parametrize("n,seed", [(65, 5), (130, 7)])
@pytest.mark.parametrize("case", list(CASES))
def test_step_airframe_grad_on_host(case, n, seed):
    ac, X, U, lam, dt, refs = _reference(case, n, seed)
    ref, agree = R.check_reference(refs)
    phi, Xb, Ub, db = host_step(ac, X, U, dt, lam)
    errs = R.summed_errors(R.chain(ac, phi), ref)
    print(f"[host agrad] {case} n={n} errs {errs} reference agreement {agree}")
    assert max(errs.values()) <= R.BAR_SUM, errs
    # the other outputs of the recording sweep are those of the plain one
    from tests.test_host_vjp import _run as plain_vjp

    Xp, Up, dp = plain_vjp(ac, 0, X, U, dt, lam)
    assert np.array_equal(Xb, Xp) and np.array_equal(Ub, Up) and np.array_equal(db, dp)


def test_step_airframe_grad_poly_4099_on_host():
    ac = R.aircraft("poly")
    X, U, lam = R.units(4099, 11)
    ref, agree = R.check_reference(R.step_reference(ac, X, U, 0.01, lam))
    errs = R.summed_errors(R.chain(ac, host_step(ac, X, U, 0.01, lam)[0]), ref)
    print(f"[host agrad] poly n=4099 errs {errs} reference agreement {agree}")
    assert max(errs.values()) <= R.BAR_SUM, errs


@pytest.mark.parametrize("case", list(CASES))
def test_single_units_on_host(case):
    """the first 16 units of the seed-5 pool, each as a call of its own: no cancellation across units"""
    ac, X, U, lam, dt, refs = _reference(case, 65, 5)
    worst = {}
    for k in range(16):
        ref, agree = R.check_reference([r[:, k:k + 1] for r in refs], bar=R.H_AGREE_UNIT)
        phi = host_step(ac, X[:, k:k + 1], U[:, k:k + 1], dt, lam[:, k:k + 1])[0]
        errs = R.unit_errors(R.chain(ac, phi), ref[:, 0])
        worst = {g: max(e, worst.get(g, 0.0)) for g, e in errs.items()}
        assert max(errs.values()) < R.BAR_UNIT, (k, errs)
    print(f"[host agrad] {case} 16 single units, worst {worst}")


def test_rollout_airframe_grad_on_host():
    ac = R.aircraft("poly")
    B, H, dt = 65, 12, 0.01
    X0, U, G = R.rollout_problem(B, H)
    ref, agree = R.check_reference(R.rollout_reference(ac, X0, U, dt, G))
    Xtraj = f32_exact(R.oracle_with(ac, R.eight_of(ac)).rollout(X0, U, dt))  # the saved nodes, as an fp32 rollout stores them
    errs = R.summed_errors(R.chain(ac, host_rollout(ac, Xtraj, U, dt, G)), ref)
    print(f"[host agrad] poly rollout B={B} H={H} errs {errs} reference agreement {agree}")
    assert max(errs.values()) <= R.BAR_SUM, errs


def test_host_sweep_substep_limit_and_other_models():
    X, U, lam = R.units(2, 5)
    assert host_step(make_aircraft("poly", substeps=41), X, U, 0.1, lam, rc_only=True) == -1
    assert host_step(make_aircraft("poly", normalise=True, substeps=40), X, U, 0.1, lam)[0].shape == (22,)
    assert host_step(make_aircraft("nn"), X, U, 0.01, lam, rc_only=True) == -2


# ---- aircraft_amd.autodiff.AirframeParameters: the checks that come before any device work ---------------------------------------
def test_derived_restates_the_aircraft_constants():
    import torch

    from aircraft_amd import autodiff
    from aircraft_amd.dynamics.aircraft import inertia_about_com

    ac = R.aircraft("poly")
    p = autodiff.AirframeParameters(ac)
    assert tuple(p.mass.shape) == () and tuple(p.inertia.shape) == (4,) and tuple(p.com.shape) == (3,)
    assert all(q.dtype == torch.float32 for q in p.parameters()) and len(list(p.parameters())) == 3
    eight = np.concatenate([q.detach().numpy().reshape(-1) for q in (p.mass, p.inertia, p.com)]).astype(np.float64)
    assert np.array_equal(eight, R.eight_of(ac))
    d = p.derived().detach().numpy()
    assert d.shape == (22,) and d.dtype == np.float64
    I = inertia_about_com(*eight[1:5], eight[0], eight[5:8])
    want = np.concatenate([eight[:1], I.ravel(), np.linalg.inv(I).ravel(), eight[5:8]])
    assert np.abs(d - want).max() <= 1e-12 * np.abs(want).max()
    s = ac._param_struct()
    sent = np.array([s.mass, *s.inertia, *s.inertia_inv, *s.com], dtype=np.float32)
    np.testing.assert_allclose(d.astype(np.float32), sent, rtol=2.5e-7, atol=1e-12)  # (two float64 inverses, rounded: one ulp)


def test_airframe_parameters_refusals():
    import torch

    from aircraft_amd import Quadrotor, autodiff

    for other in (make_aircraft("nn"), Quadrotor()):
        with pytest.raises(ValueError, match="AirframeParameters"):
            autodiff.AirframeParameters(other)
    poly, lin = make_aircraft("poly"), make_aircraft("linear")
    p = autodiff.AirframeParameters(poly)
    x, u = torch.zeros(13, 2), torch.zeros(7, 2)
    with pytest.raises(ValueError, match="another aircraft"):
        autodiff.step(lin, x, u, 0.01, params=p)
    with pytest.raises(ValueError, match="another aircraft"):
        autodiff.step(poly, x, u, 0.01, params=(autodiff.CoefficientParameters(lin), p))
    for bad in (object(), (p, autodiff.CoefficientParameters(poly)), (p,), (p, p), [autodiff.CoefficientParameters(poly), p]):
        with pytest.raises(TypeError, match="params"):
            autodiff.step(poly, x, u, 0.01, params=bad)
    # values no aircraft can fly are refused before anything is sent
    mass0 = float(poly.mass)
    with torch.no_grad():
        p.mass.fill_(-1.0)
    with pytest.raises(ValueError, match="mass"):
        p.sync()
    with torch.no_grad():
        p.mass.fill_(mass0)
        p.inertia[0] = -5.0
    with pytest.raises(ValueError, match="positive definite"):
        p.sync()
    assert float(poly.mass) == mass0 and poly.Ixx > 0  # (the aircraft kept its numbers)


def test_agrad_abi_is_exported():
    from aircraft_amd import _lib

    lib = _lib.load()
    for name in ("ac_agrad_workspace_floats", "ac_step_agrad_f32", "ac_rollout_agrad_f32"):
        assert getattr(lib, name) is not None
    n = C.c_size_t()
    assert _lib.AIRFRAME_GRAD_FLOATS == 22
    assert lib.ac_agrad_workspace_floats(None, 0, 1, 0, C.byref(n)) == -1
    assert lib.ac_step_agrad_f32(None, None, None, C.c_float(0.01), None, 1, None, None, None, None, None, None, 0, None) == -1
    assert lib.ac_rollout_agrad_f32(None, None, None, C.c_float(0.01), 1, 1, None, None, None, None, None, None, 0, None) == -1


def test_agrad_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "an_inst_agrad.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("an_inst_agrad", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "agrad.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        m = re.match(r"_ZN2ac\d+(k_step_agrad|k_rollout_agrad)ILi(\d)E", name)
        if m:
            seen[m.groups()] = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    assert len(seen) == 6, seen  # two kernels, three models
    assert not any(seen.values()), seen
