"""The trim's per-unit code (aircraft_amd/csrc/ac_trim.hpp) compiled for the host with g++ (tests/host_trim/trim_host.cpp,
-DAC_HOST_CHECK) with the analytic models' own state_derivative, checked against a float64 restatement (tests/trim_ref.py)
and the float64 oracle: the assembly z -> (x, u), the Jacobian J_z, and the whole LM loop.  Also the argument checks of
Aircraft.trim that run before any device is touched, and the register budget of the two new kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import trim_ref as T
from tests.helpers import make_aircraft, make_oracle, unit_max_rel
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_trim")
SO = os.path.join(HERE, "libtrim_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc")
FP = C.POINTER(C.c_float)


def _lib_host():
    src = os.path.join(HERE, "trim_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_dynamics.hpp", "ac_trim.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", SO, src],
                       check=True)
    L = C.CDLL(SO)
    L.host_trim_assemble.argtypes = [C.c_int, FP, FP, FP, C.c_long, FP, FP]
    L.host_trim_jacobian.argtypes = [C.c_void_p, FP, FP, FP, C.c_int, FP, FP, FP, C.c_long, FP, FP]
    L.host_trim.argtypes = [C.c_void_p, FP, FP, FP, C.c_void_p, FP, FP, FP, C.c_int, C.c_long, FP, FP, FP, FP, C.POINTER(C.c_int)]
    IP = C.POINTER(C.c_int)
    L.host_trim_trace.argtypes = L.host_trim.argtypes + [FP] * 6
    L.host_trim_chain.argtypes = [C.c_int, FP, FP, FP, FP, FP, C.c_long, FP, FP]
    L.host_trim_step.argtypes = [C.c_void_p, FP, FP, FP, FP, C.c_long, FP]
    L.host_trim_final_status.argtypes = [C.c_void_p, FP, FP, FP, C.c_long, IP]
    for f in (L.host_trim_assemble, L.host_trim_jacobian, L.host_trim, L.host_trim_trace, L.host_trim_chain, L.host_trim_step,
              L.host_trim_final_status):
        f.restype = C.c_int
    return L


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _model_args(ac):
    d = ac.coefficient_model.oracle_data() or {}
    keep = [f32(d[k]) if k in d else None for k in ("W", "coef", "intercept")]
    return keep, [a.ctypes.data_as(FP) if a is not None else None for a in keep]


def synthetic_problem(n, lateral, seed):
    """random targets and z inside the bounds (f32-exact)"""
    rng = np.random.default_rng(seed)
    tg = np.zeros((7, n))
    tg[0:3] = rng.uniform(-100, 100, (3, n))
    tg[3] = rng.uniform(25, 70, n)
    tg[4] = rng.uniform(-np.pi, np.pi, n)
    tg[5] = rng.uniform(-0.2, 0.2, n)
    tg[6] = rng.uniform(-5, 5, n) if lateral else rng.uniform(-3, 3, n) * T.DEG
    uh = np.zeros((7, n))
    uh[6] = rng.uniform(0, 1, n)
    z = np.stack([rng.uniform(-8, 8, n) * T.DEG, rng.uniform(-30, 20, n) * T.DEG, rng.uniform(-40, 40, n) * T.DEG,
                  rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-3, 3, n) * (T.DEG if lateral else 1.0)])
    return f32(tg).astype(np.float64), f32(uh).astype(np.float64), f32(z).astype(np.float64)


def host_solve(ac, target, uhold, z0, lateral, iters=30, tol=(1e-4, 1e-4), bounds=None):
    L = _lib_host()
    n = target.shape[1]
    keep, ptr = _model_args(ac)
    o = _lib.TrimOpts()
    o.lateral = lateral
    o.tol_v, o.tol_w = tol
    lo, hi = ac.trim_bounds(lateral) if bounds is None else bounds
    o.lo[:] = [float(v) for v in lo]
    o.hi[:] = [float(v) for v in hi]
    t, u, z = f32(target), f32(uhold), f32(z0)
    X, U = np.zeros((13, n), np.float32), np.zeros((7, n), np.float32)
    Z, R, S = np.zeros((6, n), np.float32), np.zeros((6, n), np.float32), np.zeros(n, np.int32)
    rc = L.host_trim(C.byref(ac._param_struct()), *ptr, C.byref(o), t.ctypes.data_as(FP), u.ctypes.data_as(FP),
                     z.ctypes.data_as(FP), iters, n, X.ctypes.data_as(FP), U.ctypes.data_as(FP), Z.ctypes.data_as(FP),
                     R.ctypes.data_as(FP), S.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return X.astype(np.float64), U.astype(np.float64), Z.astype(np.float64), R.astype(np.float64), S


# ---- 1. assembly --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lateral", [0, 1])
def test_assembly_matches_float64(lateral):
    L = _lib_host()
    n = 200
    tg, uh, z = synthetic_problem(n, lateral, seed=1)
    X, U = np.zeros((13, n), np.float32), np.zeros((7, n), np.float32)
    assert L.host_trim_assemble(lateral, f32(tg).ctypes.data_as(FP), f32(uh).ctypes.data_as(FP), f32(z).ctypes.data_as(FP), n,
                                X.ctypes.data_as(FP), U.ctypes.data_as(FP)) == 0
    x, u = T.assemble(z, tg, uh, lateral)
    assert np.abs(X[0:3] - x[0:3]).max() <= 1e-7 * np.abs(x[0:3]).max()
    assert np.abs(X[3:6] - x[3:6]).max() < 1e-5 * 70  # |v| = V <= 70 m/s: fp32 rounding of the trig and rotation
    assert np.abs(X[6:10] - x[6:10]).max() < 1e-6
    assert np.abs(X[10:13] - x[10:13]).max() < 1e-7
    assert np.array_equal(U, f32(u))  # copied, not computed
    # the attitude is the Euler-to-quaternion map that euler_angles() inverts
    qx, qy, qz, qw = x[6:10]
    phi = np.arctan2(2 * (qw * qx + qy * qz), 1 - 2 * (qx * qx + qy * qy))
    theta = np.arcsin(2 * (qw * qy - qz * qx))
    assert np.abs(phi - z[2]).max() < 1e-12 and np.abs(theta - z[1]).max() < 1e-12


# ---- 2. Jacobian ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lateral", [0, 1])
@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_jacobian_matches_float64_chain(model, lateral):
    ac = make_aircraft(model)
    orc = make_oracle(ac)
    L = _lib_host()
    n = 96
    tg, uh, z = synthetic_problem(n, lateral, seed=2)
    keep, ptr = _model_args(ac)
    R, J = np.zeros((6, n), np.float32), np.zeros((36, n), np.float32)
    assert L.host_trim_jacobian(C.byref(ac._param_struct()), *ptr, lateral, f32(tg).ctypes.data_as(FP), f32(uh).ctypes.data_as(FP),
                                f32(z).ctypes.data_as(FP), n, R.ctypes.data_as(FP), J.ctypes.data_as(FP)) == 0
    r64, J64 = T.jacobian(orc, z, tg, uh, lateral)
    assert unit_max_rel(J.reshape(6, 6, n), J64).max() <= 1e-5
    assert unit_max_rel(R, r64).max() <= 1e-5


# ---- 3. the whole loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_host_loop_converged_trims_satisfy_oracle(model):
    ac = make_aircraft(model)
    orc = make_oracle(ac)
    g = T.grid(seed=3)
    for lateral in (0, 1):
        cases = [c for c in g if (c[1] == 0.0 or (model == "linear") == (lateral == 1))] if lateral == 0 else \
            [c for c in g if model == "linear" and c[1] != 0.0]
        if not cases:
            continue
        n = len(cases)
        tg = np.zeros((7, n))
        uh = np.zeros((7, n))
        for i, (V, psid, beta, fl, psi) in enumerate(cases):
            tg[:, i] = [0.0, 0.0, -200.0, V, psi, psid, 0.0 if lateral else beta]
            uh[6, i] = fl
        tg, uh = f32(tg).astype(np.float64), f32(uh).astype(np.float64)
        z0 = T.default_guess(tg[3], tg[5], ac.opts.aircraft_config.glide_ratio)
        X, U, Z, R, S = host_solve(ac, tg, uh, z0, lateral)
        ok = S == 0
        assert ok.sum() >= n // 2, (model, lateral, np.bincount(S, minlength=4))
        r = T.residual_at(orc, X[:, ok], U[:, ok], Z[:, ok], tg[:, ok], lateral)
        assert np.abs(r[:3]).max() <= 1e-3 and np.abs(r[3:]).max() <= 1e-3, np.abs(r).max()
        # the straight glides without flaps up to 50 m/s all trim (at 70 m/s the linear model needs theta below -60 deg)
        straight = np.array([c[1] == 0.0 and c[3] == 0.0 and c[0] <= 50.0 for c in cases])
        if lateral == 0:
            assert ok[straight].all(), (model, S[straight])
        # the kernel's own stored residual is the one it reports
        assert np.abs(R[:, ok]).max() <= 1e-4


def test_host_loop_frozen_and_nonfinite():
    ac = make_aircraft("poly")
    tg = np.zeros((7, 4))
    tg[2] = -200.0
    tg[3] = [40.0, 40.0, 0.0, np.nan]  # V = 0 and NaN: status 3
    uh = np.zeros((7, 4))
    z0 = T.default_guess(tg[3], tg[5], 3.0)
    z0 = np.nan_to_num(z0)
    a = host_solve(ac, tg, uh, z0, 0, iters=30)
    b = host_solve(ac, tg, uh, z0, 0, iters=60)
    assert list(a[4][:2]) == [0, 0] and list(a[4][2:]) == [3, 3]
    for p, q in zip(a, b):
        assert np.array_equal(p[..., :2], q[..., :2])  # frozen after convergence: bit-identical at 30 and 60 iterations


def test_host_loop_reports_bound():
    """A 70 m/s glide with full flaps would need theta below the default -60 deg: status 2, theta on its bound."""
    ac = make_aircraft("poly")
    tg = np.array([[0.0], [0.0], [-200.0], [70.0], [0.0], [0.0], [0.0]])
    uh = np.zeros((7, 1))
    uh[6] = 1.0
    X, U, Z, R, S = host_solve(ac, tg, uh, T.default_guess(70.0, 0.0, 3.0), 0, iters=40)
    assert S[0] == 2 and abs(Z[1, 0] + np.deg2rad(60)) < 1e-6


# ---- 4. Python argument checks (before any device call) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(iters=0), dict(iters=2.5), dict(tol=(0.0, 1e-4)), dict(tol=(1e-4,)), dict(rudder=1.0, beta=0.1),
    dict(bounds=(np.ones(6), -np.ones(6))), dict(bounds=(np.zeros(5), np.ones(5))), dict(position=np.zeros(4)),
    dict(guess=np.zeros(5)), dict(psi=np.zeros(3)), dict(thrust=np.zeros((2, 4))), dict(ws=np.zeros(10, np.float32)),
])
def test_trim_argument_checks(kw):
    ac = make_aircraft("poly")
    with pytest.raises(ValueError):
        ac.trim(np.array([30.0, 40.0, 50.0, 60.0]), **kw)
    assert not ac._handle  # nothing reached the library


def test_trim_bounds_default():
    ac = make_aircraft("default")
    lo, hi = ac.trim_bounds(0)
    assert np.allclose(hi, [np.deg2rad(20), np.deg2rad(60), np.deg2rad(80), 10, 10, 10]) and np.array_equal(lo, -hi)
    assert np.isclose(ac.trim_bounds(1)[1][5], np.deg2rad(10))


# ---- 5. resources --------------------------------------------------------------------------------------------------------------------------
def test_trim_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "an_inst_trim.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("an_inst_trim", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "trim.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("k_trim_assemble", "k_trim_update"):
        assert scratch_bytes(r.stderr, k) == 0, k
