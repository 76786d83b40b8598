"""The fused reverse-mode code (aircraft_amd/csrc/ac_vjp.hpp) compiled for the host with g++ (tests/host_vjp/vjp_host.cpp,
-DAC_HOST_CHECK) and checked against the float64 oracle's EXACT Jacobians: [A | B | c]' lambda of the whole state_update —
sub-steps composed in reverse order, the quaternion normalisation adjoint applied once, after the last sub-step — and
(df/dx, df/du)' w of f.  Also the argument checking of aircraft_amd.autodiff that runs before any device is touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import f32_exact, make_aircraft, make_oracle, synthetic_units, unit_max_rel

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_vjp")
SO = os.path.join(HERE, "libvjp_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc")


def _lib():
    src = os.path.join(HERE, "vjp_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_dynamics.hpp", "ac_adjoint.hpp", "ac_vjp.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        # -ffp-contract=off: the tolerance below then holds for the least favourable (unfused) rounding
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", SO, src], check=True)
    L = C.CDLL(SO)
    fp = C.POINTER(C.c_float)
    L.host_vjp.restype = C.c_int
    L.host_vjp.argtypes = [C.c_void_p, fp, fp, fp, C.c_int, fp, fp, fp, C.c_int, fp, C.c_long, fp, fp, fp]
    return L


def _run(ac, what, X, U, dt, lam):
    L = _lib()
    fp = C.POINTER(C.c_float)
    n = X.shape[1]
    p = ac._param_struct()
    d = ac.coefficient_model.oracle_data() or {}
    keep = [np.ascontiguousarray(d[k], dtype=np.float32) if k in d else None for k in ("W", "coef", "intercept")]
    ptr = [a.ctypes.data_as(fp) if a is not None else None for a in keep]
    per_unit = np.ndim(dt) > 0
    Xf, Uf, Lf, Df = (np.ascontiguousarray(a, dtype=np.float32) for a in (X, U, lam, np.atleast_1d(dt)))
    Xb, Ub, db = np.zeros((13, n), np.float32), np.zeros((7, n), np.float32), np.zeros(n, np.float32)
    rc = L.host_vjp(C.byref(p), ptr[0], ptr[1], ptr[2], what, Xf.ctypes.data_as(fp), Uf.ctypes.data_as(fp), Df.ctypes.data_as(fp),
                    int(per_unit), Lf.ctypes.data_as(fp), n, Xb.ctypes.data_as(fp), Ub.ctypes.data_as(fp), db.ctypes.data_as(fp))
    assert rc == 0, rc
    return Xb, Ub, db


def _units(n, seed):
    X, U = synthetic_units(n, seed=seed, flaps=True)
    lam = np.random.default_rng(seed + 7).normal(size=(13, n))
    return f32_exact(X), f32_exact(U), f32_exact(lam)


@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("normalise", [True, False])
@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_step_vjp_substeps_and_single_normalisation_on_host(model, normalise, substeps):
    ac = make_aircraft(model, normalise=normalise, substeps=substeps, stall_scaling=(model == "default" and not normalise))
    X, U, lam = _units(48, seed=51)
    Xb, Ub, db = _run(ac, 0, X, U, 0.01, lam)
    _, A, B, c = make_oracle(ac).step_sens(X, U, 0.01)
    want = np.einsum("in,izn->zn", lam, np.concatenate([A, B, c[:, None, :]], axis=1))
    got = np.concatenate([Xb, Ub, db[None]], axis=0)
    assert unit_max_rel(got, want).max() < 2e-5
    assert np.array_equal(Xb[:3], lam[:3].astype(np.float32))  # p never enters f: x_bar[0..2] = lam[0..2] exactly
    assert not Ub[3:6].any()


def test_step_vjp_normalises_once_not_per_substep_on_host():
    """The adjoint of a normalisation after EVERY sub-step would be a different map: with the quaternion off the unit sphere
    the two differ, and only the reference's (once, at the end) matches the oracle."""
    ac = make_aircraft("default", normalise=True, substeps=10)
    X, U, lam = _units(24, seed=52)
    X[6:10] *= 1.3  # |q| = 1.3: each sub-step's normalisation would rescale
    X = f32_exact(X)
    Xb, Ub, db = _run(ac, 0, X, U, 0.01, lam)
    _, A, B, c = make_oracle(ac).step_sens(X, U, 0.01)
    want = np.einsum("in,izn->zn", lam, np.concatenate([A, B, c[:, None, :]], axis=1))
    assert unit_max_rel(np.concatenate([Xb, Ub, db[None]]), want).max() < 2e-5


def test_step_vjp_per_unit_dt_on_host():
    ac = make_aircraft("poly", normalise=True, substeps=3)
    X, U, lam = _units(40, seed=53)
    dts = f32_exact(np.random.default_rng(4).uniform(0.005, 0.02, 40))
    Xb, Ub, db = _run(ac, 0, X, U, dts, lam)
    _, A, B, c = make_oracle(ac).step_sens(X, U, dts)
    want = np.einsum("in,izn->zn", lam, np.concatenate([A, B, c[:, None, :]], axis=1))
    assert unit_max_rel(np.concatenate([Xb, Ub, db[None]]), want).max() < 2e-5


@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_state_derivative_vjp_on_host(model):
    ac = make_aircraft(model, stall_scaling=(model != "poly"))
    X, U, w = _units(48, seed=54)
    Xb, Ub, _ = _run(ac, 1, X, U, 0.0, w)
    _, Fx, Fu = make_oracle(ac).state_derivative_sens(X, U)
    want = np.einsum("in,izn->zn", w, np.concatenate([Fx, Fu], axis=1))
    assert unit_max_rel(np.concatenate([Xb, Ub]), want).max() < 2e-5
    assert not Xb[:3].any()


# ---- aircraft_amd.autodiff: the checks that come before any device work --------------------------------------------------------
def test_autodiff_refuses_numpy_and_bad_shapes():
    import torch

    from aircraft_amd import autodiff

    ac = make_aircraft("poly")
    x, u = np.zeros((13, 4)), np.zeros((7, 4))
    for fn, args in ((autodiff.step, (x, u, 0.01)), (autodiff.state_derivative, (x, u)),
                     (autodiff.rollout, (x, np.zeros((3, 7, 4)), 0.01))):
        with pytest.raises(TypeError, match="torch.Tensor"):
            fn(ac, *args)
    xt, ut = torch.zeros(13, 4), torch.zeros(7, 4)
    with pytest.raises(ValueError, match="x:"):
        autodiff.step(ac, torch.zeros(12, 4), ut, 0.01)
    with pytest.raises(ValueError, match="u:"):
        autodiff.step(ac, xt, torch.zeros(7, 5), 0.01)
    with pytest.raises(ValueError, match="dt"):
        autodiff.step(ac, xt, ut, torch.full((3,), 0.01))
    with pytest.raises(TypeError, match="dt"):
        autodiff.step(ac, xt, ut, np.full(4, 0.01))
    with pytest.raises(ValueError, match="U:"):
        autodiff.rollout(ac, xt, torch.zeros(3, 7, 5), 0.01)
    with pytest.raises(ValueError, match="scalar"):
        autodiff.rollout(ac, xt, torch.zeros(3, 7, 4), torch.full((4,), 0.01))
    with pytest.raises(ValueError, match="u:"):
        autodiff.state_derivative(ac, xt, torch.zeros(6, 4))


def test_vjp_abi_is_exported():
    from aircraft_amd import _lib

    lib = _lib.load()
    for name in ("ac_step_vjp_f32", "ac_rollout_vjp_f32", "ac_state_derivative_vjp_f32", "ac_vjp_workspace_floats",
                 "ac_set_vjp_route"):
        assert getattr(lib, name) is not None
    assert lib.ac_set_vjp_route(None, 0) == -1
    n = C.c_size_t()
    assert lib.ac_vjp_workspace_floats(None, 0, 1, 0, C.byref(n)) == -1
