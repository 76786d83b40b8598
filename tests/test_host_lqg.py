"""The per-lane code of the loop closed through the estimator (aircraft_amd/csrc/ac_lqg.hpp) compiled for the host with g++
(tests/host_lqg/lqg_host.cpp, -DAC_HOST_CHECK -ffp-contract=off) against tests/lqg_ref.py: Philox, the schedule and the dropout
bit for bit; the control law bit for bit against the float32 fmaf chain; sense, disturb and the score against float64; mutated
copies of the header that these checks must catch; the argument checks of the new Python methods that run before any device
is touched; the resources of the kernels from the compiler's remarks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests import lqg_ref as R
from tests import mppi_ref as M
from tests.helpers import make_aircraft
from tests.test_host_mppi import sample_tolerance

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_lqg")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_lqg.hpp")
FP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint)
_LIBS = {}

# the sensors of these tests: GPS every 5th step from step 2, the air data dropped 3 times in 10, instances offset past 2^32
SENS = R.Sensors(seed=0x123456789ABCDEF, instance_offset=(1 << 32) + 5, period=(5, 5, 1, 1, 2), phase=(2, 2, 0, 0, 1),
                 dropout=(0.0, 0.0, 0.0, 0.3, 0.0))
# h's own float32 error on rows 9-14: the e32 ekf_ref records for h (the magnetometer rows' relative error), applied to every row
# formed from a rotated vector
H_TOL = E.E32_WORST["mag"]


def lib_host(header=None):
    """the host build of ac_lqg.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "lqg_host.cpp")
    so = os.path.join(HERE, "liblqg_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp", "ac_ekf.hpp", "ac_rts.hpp", "ac_mppi.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_LQG_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_lqg_philox.argtypes = [UP, UP, C.c_long, UP]
    lib.host_lqg_schedule.argtypes = [C.c_void_p, C.c_int, C.c_long, C.c_long, IP]
    lib.host_lqg_sense.argtypes = [C.c_void_p, C.c_float, C.c_int, FP, FP, C.c_long, FP, IP]
    lib.host_lqg_disturb.argtypes = [C.c_void_p, C.c_int, FP, FP, C.c_long, FP]
    lib.host_lqg_policy.argtypes = [FP, FP, FP, FP, FP, FP, C.c_long, FP]
    lib.host_lqg_score.argtypes = [FP, FP, FP, C.c_long, FP, FP, IP]
    for f in ("philox", "schedule", "sense", "disturb", "policy", "score"):
        getattr(lib, "host_lqg_" + f).restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the checks (the mutated headers must fail at least one) -------------------------------------------------------------------------
def check_philox(header=None):
    c = np.array([k[0] for k in M.KNOWN_ANSWERS], dtype=np.uint32).T.copy()
    k = np.array([k[1] for k in M.KNOWN_ANSWERS], dtype=np.uint32).T.copy()
    out = np.zeros((4, c.shape[1]), np.uint32)
    assert lib_host(header).host_lqg_philox(c.ctypes.data_as(UP), k.ctypes.data_as(UP), c.shape[1], out.ctypes.data_as(UP)) == 0
    assert [tuple(int(v) for v in out[:, i]) for i in range(c.shape[1])] == [k[2] for k in M.KNOWN_ANSWERS]


def check_schedule(header=None, n=257, T=23, step=-3):
    """every step of a window that starts before the phases, bit for bit: the comparison is integer and an exact 2^-24 product"""
    host = R.host_schedule(SENS, step, T, n, header)
    ref = np.stack([R.report_mask(SENS, n, step + t) for t in range(T)])
    assert np.array_equal(host, ref)
    gps = (host & 0x3F) != 0
    assert [t for t in range(T) if gps[t].any()] == [t for t in range(T) if (step + t - 2) % 5 == 0] and gps[5].all()
    air = ((host >> 9) & 7) == 7
    assert 0.6 < air.mean() < 0.8 and (((host >> 6) & 7) == 7).all()  # dropout 0.3 on the air data, none on the gyro


def sense_tolerance(Z, rad, hx, sigma=E.SIG_R):
    """|Z - Z64| allowed: test_host_mppi's bound on the noise term (sigma (15,)), plus h's own float32 error on rows 9-14"""
    tol = sample_tolerance(Z[None], rad[None], sigma)[0]
    tol[9:15] += H_TOL * np.maximum(1.0, np.abs(hx[9:15]))
    return tol


def disturb_tolerance(Xr, rad, sigma=E.SIG_Q):
    """|Xo - Xo64| allowed, the same bound through [+]: the position, velocity and rate rows add d; a component of
    q (x) (d/2, 1) / |.| moves by at most half of each rotation coordinate's error (|dq / dtheta_j| <= 1/2)"""
    sq = np.concatenate([sigma[0:6], np.repeat(0.5 * sigma[6:9].sum(), 4), sigma[9:12]])
    radx = np.concatenate([rad[0:6], np.repeat(rad[6:9].max(axis=0)[None], 4, axis=0), rad[9:12]])
    tol = sample_tolerance(Xr[None], radx[None], sq)[0]
    # the float32 roundings behind one component of a unit quaternion: its product (4), the norm (4, halved by the square root),
    # the square root, the reciprocal and the scaling: ten at the most, each of at most half an ulp of 1
    tol[6:10] += 10 * 2.0 ** -25
    return tol


DISTURB_BLOCKS = (("p", slice(0, 3)), ("v", slice(3, 6)), ("q", slice(6, 10)), ("w", slice(10, 13)))


def disturb_ratios(err, tol):
    """how much of the allowance every row block uses"""
    return ", ".join(f"{k} {(err[sl] / tol[sl]).max():.3f}" for k, sl in DISTURB_BLOCKS)


def sense_case(name):
    d = E.inputs(name)
    return E.measure_states(name), d["eps"]


def check_sense(name="poly", header=None):
    x, eps = sense_case(name)
    x = E.cycle(x, 40)
    for step in (9, 12):  # 9: the magnetometer and no GPS; 12: the GPS and no magnetometer; the gyro always, some air data
        Zh, mh = R.host_sense(x, E.SIG_R, SENS, step, eps, header)
        Z, mask, hx, rad = R.sense(x, E.SIG_R, SENS, step, eps)
        assert np.array_equal(mh, mask) and np.array_equal(np.isnan(Zh), np.isnan(Z))
        rep = ~np.isnan(Z)
        assert rep[6:9].all() and rep[0:6].all() == (step == 12) and rep[12:15].all() == (step == 9) and 0 < rep[9].sum() < rep.shape[1]
        assert rep[0:6].any() == (step == 12) and rep[12:15].any() == (step == 9)
        tol = sense_tolerance(Z, rad, hx)
        err = np.abs(Zh.astype(np.float64) - Z)
        print(f"[lqg sense] {name} step {step}: worst |dZ| / tol {np.nanmax(err / tol):.3f}")
        assert (err[rep] <= tol[rep]).all()
    step = 9
    # without noise the rows are the measurement kernel's, bit for bit
    Z0, m0 = R.host_sense(x, np.zeros(15), R.Sensors(mag=SENS.mag), step, eps, header)
    assert (m0 == E.ALL).all() and np.array_equal(Z0.astype(np.float64), E.host_measure(x, E.MAG, eps))


def check_disturb(name="poly", header=None, step=7):
    x = E.cycle(E.inputs(name)["x"], 40)
    Xh = R.host_disturb(x, E.SIG_Q, SENS, step, header)
    Xr, d, rad = R.disturb(x, E.SIG_Q, SENS, step)
    tol = disturb_tolerance(Xr, rad)
    err = np.abs(Xh.astype(np.float64) - Xr)
    print(f"[lqg disturb] {name}: worst |dX| / tol " + disturb_ratios(err, tol))
    assert (err <= tol).all() and np.abs(d).max() > 0


def policy_case(n=40, seed=5):
    rng = np.random.default_rng(seed)
    d = E.inputs("poly")
    xn, un = E.cycle(d["x"], n), E.cycle(d["u"], n)
    fb = E.f32x(E.boxplus(xn, E.SIG_P0[:, None] * rng.standard_normal((12, n))))
    Kx = E.f32x(rng.standard_normal((7, 13, n)) * 3.0)
    lo, hi = np.array([-5.0, -5, -5, -np.inf, 0, 0, 0]), np.array([5.0, 5, 5, np.inf, 0, 0, 1])
    return fb, xn, un, Kx, lo, hi


def check_policy(header=None):
    fb, xn, un, Kx, lo, hi = policy_case()
    U = R.host_policy(fb, xn, un, Kx, lo, hi, header)
    U32 = R.policy32(fb, xn, un, Kx, lo, hi)
    assert np.array_equal(U, U32)
    assert (U[0:3] == 5).any() and (U[0:3] == -5).any() and (np.abs(U[0:3]) < 5).any() and (U[4:6] == 0).all()
    ref = R.policy(fb, xn, un, Kx, lo, hi)
    assert np.abs(U - ref).max() <= 1e-3  # (float64: the same law, not the same rounding)


def score_errors(name, header=None):
    d = E.inputs(name)
    e, nees, st = R.host_score(d["truth"], d["x"], d["P"], header)
    er, nr, sr = R.score(E.f32x(d["truth"]), d["x"], d["P"])
    assert not st.any() and not sr.any()
    return {"e": R.err_e(e.astype(np.float64), er, d["P"]), "nees": E.err_scalar(nees.astype(np.float64), nr)}


def check_score(name="poly", header=None):
    m = score_errors(name, header)
    print(f"[lqg e32] {name}: " + ", ".join(f"{k} {v.max():.2e}" for k, v in m.items()))
    for k, bar in R.E32_WORST.items():
        assert m[k].max() <= bar, (k, m[k].max(), bar)


CHECKS = {"philox": check_philox, "schedule": check_schedule, "sense": check_sense, "disturb": check_disturb, "policy": check_policy,
          "score": check_score}


def test_philox_known_answers():
    check_philox()


def test_schedule_and_dropout_bit_equal():
    check_schedule()


def test_schedule_at_the_ends_of_the_step_range():
    """step - phase is taken in 64-bit: the largest step with the most negative phase (and the reverse) is no overflow"""
    big = 2 ** 31 - 1
    for step, phase in ((big - 3, -big), (-big, big), (big - 3, big), (-big, -big)):
        s = R.Sensors(seed=3, period=(7, 5, 3, 2, 1), phase=(phase,) * 5, dropout=(0.0, 0.0, 0.0, 0.3, 0.0))
        host = R.host_schedule(s, step, 4, 9)
        assert np.array_equal(host, np.stack([R.report_mask(s, 9, step + t) for t in range(4)])), (step, phase)


def test_policy_is_the_stated_fma_chain():
    check_policy()


@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_sense_and_disturb_against_float64(name):
    check_sense(name)
    check_disturb(name)


@pytest.mark.parametrize("name", E.MODELS)
def test_score_e32_within_recorded_worst(name):
    check_score(name)


def test_recorded_worst_is_measured_plus_ten_percent():
    for key, bar in R.E32_WORST.items():
        w = max(float(score_errors(n)[key].max()) for n in E.MODELS)
        assert w <= bar <= 1.25 * w, (key, w, bar)


def test_score_status_and_nan():
    d = E.inputs("poly")
    x, xh, P = E.f32x(d["truth"][:, :4]), d["x"][:, :4], d["P"][:, :, :4].copy()
    P[3, 3, 1] = -1.0                      # a negative pivot
    P[:, :, 2] = np.nan                    # not finite
    e, nees, st = R.host_score(x, xh, P)
    er, nr, sr = R.score(x, xh, P)
    assert list(st) == [0, 1, 1, 0] and list(sr) == [0, 1, 1, 0]
    assert np.isnan(nees[[1, 2]]).all() and np.isfinite(nees[[0, 3]]).all() and np.isfinite(e).all()
    # the truth scored against itself: e = 0 exactly (a unit attitude up to its float32 norm), nees = 0
    e, nees, st = R.host_score(xh, xh, P[:, :, [0, 0, 3, 3]])
    assert np.abs(e).max() <= 1e-6 and (e[[0, 1, 2, 3, 4, 5, 9, 10, 11]] == 0).all() and nees.max() <= 1e-6 and not st.any()


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "counter_words_swapped": ("(unsigned)(g >> 32), step, purpose, o.seed_lo", "(unsigned)(g >> 32), purpose, step, o.seed_lo", ("sense", "disturb")),
    "phase_off_by_one": ("((long long)step - o.phase[j]) % o.period[j] == 0", "((long long)step - o.phase[j] + 1) % o.period[j] == 0", ("schedule",)),
    "error_sign_flipped": ("rts_minus(x, xh, e);", "rts_minus(xh, x, e);", ("score",)),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new, checks = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, (which, old)
    path = str(tmp_path / f"ac_lqg_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_mppi.hpp"', f'#include "{CSRC}/ac_mppi.hpp"')
                .replace('#include "ac_rts.hpp"', f'#include "{CSRC}/ac_rts.hpp"'))
    for c in checks:
        with pytest.raises(AssertionError):
            CHECKS[c](header=path)


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(sigma=np.ones(14)), dict(sigma=-np.ones(15)), dict(sigma=np.full(15, np.nan)), dict(sigma=np.ones((15, 2, 2))),
    dict(period=(1, 1, 1, 1)), dict(period=(0, 1, 1, 1, 1)), dict(period=(1.5, 1, 1, 1, 1)), dict(phase=(0, 0, 0)),
    dict(dropout=(0, 0, 0, 0, 1.0)), dict(dropout=(-0.1, 0, 0, 0, 0)), dict(dropout=(0, 0)), dict(seed=-1), dict(seed=1.5),
    dict(seed=2 ** 64), dict(mag_ned=(1.0, 0.0)), dict(instance_offset=-1),
])
def test_sensor_model_argument_checks(kw):
    import torch

    from aircraft_amd import SensorModel

    with pytest.raises(ValueError):  # values of host tensors are checked too
        SensorModel(sigma=-torch.ones(15))

    args = dict(sigma=E.SIG_R)
    args.update(kw)
    with pytest.raises(ValueError):
        SensorModel(**args)


def _bank(ac, n=4):
    """an EKF bank without a device: what the checks read of it"""
    from aircraft_amd import EKF

    class Shape:
        shape = (13, n)

    return EKF(ac, Shape(), None, None, None, E.MAG, None, True, False)


def _good(n=4, T=3):
    from aircraft_amd import SensorModel

    return dict(x0=np.zeros((13, n)), Xnom=np.zeros((T + 1, 13, n)), Unom=np.zeros((T, 7, n)), Kx=np.zeros((T, 7, 13, n)), dt=0.01,
                sensors=SensorModel(sigma=E.SIG_R))


@pytest.mark.parametrize("kw", [
    dict(x0=np.zeros((12, 4))), dict(x0=np.zeros((13, 3))), dict(Xnom=np.zeros((4, 13, 3))), dict(Xnom=np.zeros((13, 4))),
    dict(Unom=np.zeros((4, 7, 4))), dict(Kx=np.zeros((3, 7, 12, 4))), dict(dt=0.0), dict(dt=float("nan")), dict(sensors=None),
    dict(process_sigma=np.ones(11)), dict(process_sigma=-np.ones(12)), dict(process_sigma=np.ones((12, 3))),
    dict(limits=(np.zeros(7), -np.ones(7))), dict(limits=(np.zeros(6), np.ones(6))), dict(feedback="both"), dict(record=("Q",)),
    dict(step0=1.5), dict(step0=2 ** 31 - 3), dict(ws=np.zeros(10, np.float32)), dict(est=None), dict(mag=(0.4, 0.0, 0.9)),
    dict(process_sigma="nan tensor"),
])
def test_rollout_output_feedback_argument_checks(kw):
    ac = make_aircraft("poly")
    import torch

    from aircraft_amd import SensorModel

    args = dict(est=_bank(ac), **_good())
    kw = dict(kw)
    if "mag" in kw:  # the sensors' field differs from the bank's
        args["sensors"] = SensorModel(sigma=E.SIG_R, mag_ned=kw.pop("mag"))
    if isinstance(kw.get("process_sigma"), str):  # values of host tensors are checked too
        kw["process_sigma"] = torch.full((12,), float("nan"))
    args.update(kw)
    est = args.pop("est")
    with pytest.raises(ValueError):
        ac.rollout_output_feedback(est, **args)
    assert not ac._handle  # nothing reached the library


def test_sigma_columns_and_foreign_bank_are_rejected():
    from aircraft_amd import LqrResult, SensorModel

    ac, other = make_aircraft("poly"), make_aircraft("poly")
    args = _good()
    with pytest.raises(ValueError):
        ac.rollout_output_feedback(_bank(other), **args)
    args["sensors"] = SensorModel(sigma=np.ones((15, 3)))
    with pytest.raises(ValueError):
        ac.rollout_output_feedback(_bank(ac), **args)
    with pytest.raises(ValueError):
        ac.sense(np.zeros((13, 4)), args["sensors"], 0)
    with pytest.raises(ValueError):
        ac.sense(np.zeros((12, 4)), SensorModel(sigma=E.SIG_R), 0)
    with pytest.raises(ValueError):
        ac.sense(np.zeros((13, 4)), SensorModel(sigma=E.SIG_R), 0.5)
    res = LqrResult(*([None] * 10))
    for bad in (dict(T=0), dict(T=2.0), dict(res=None), dict(x0=np.zeros((13, 3)))):
        a = dict(res=res, est=_bank(ac), x0=np.zeros((13, 4)), T=3, sensors=SensorModel(sigma=E.SIG_R), dt=0.01)
        a.update(bad)
        with pytest.raises(ValueError):
            ac.rollout_lqg(a.pop("res"), a.pop("est"), a.pop("x0"), a.pop("T"), a.pop("sensors"), **a)
    assert not ac._handle and not other._handle


# ---- resources -------------------------------------------------------------------------------------------------------------------------
# what DESIGN.md §4.19 states: VGPRs, LDS bytes per workgroup, waves per SIMD; scratch 0 B for all
RESOURCES = {"_ZN2ac11k_lqg_senseILb0": (60, 0, 8), "_ZN2ac11k_lqg_senseILb1": (70, 0, 7), "_ZN2ac13k_lqg_control": (60, 0, 8),
             "_ZN2ac11k_lqg_score": (111, 0, 4)}


def test_lqg_kernel_resources(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "lqg_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("lqg_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "lqg.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    for prefix, (vgprs, lds, occ) in RESOURCES.items():
        (b,) = [b for b in blocks if b.startswith(prefix)]
        got = tuple(int(re.search(p, b).group(1)) for p in (r" VGPRs: (\d+)", r"LDS Size \[bytes/block\]: (\d+)", r"Occupancy \[waves/SIMD\]: (\d+)"))
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, prefix
        assert got == (vgprs, lds, occ), (prefix, got)
