"""The EKF's per-lane code (aircraft_amd/csrc/ac_ekf.hpp) compiled for the host with g++ (tests/host_ekf/ekf_host.cpp,
-DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/ekf_ref.py) on identical float32-rounded
inputs, per instance and per output, over the grids of every model and the mask cases; the bitwise symmetry of P; mutated
copies of the header that these checks must catch; the argument checks of Aircraft.ekf that run before any device is
touched; the scratch budget of the kernels from the compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_ekf")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_ekf.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_ekf.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "ekf_host.cpp")
    so = os.path.join(HERE, "libekf_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_EKF_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_ekf_step.argtypes = [C.c_void_p, C.c_float, FP, FP, FP, FP, FP, IP, FP, FP, FP, C.c_long, FP, FP, FP, FP, FP, FP, IP, IP,
                                  FP, FP, FP]
    lib.host_ekf_measure.argtypes = [C.c_void_p, C.c_float, FP, C.c_long, FP]
    lib.host_ekf_step.restype = lib.host_ekf_measure.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
def measure(name, header=None, cases=None):
    """e32 of every output on the inputs of `name`, per mask case: {case: {measure: (m,)}}; x- and A from the oracle, rounded"""
    d = E.inputs(name)
    xp, A, _, _ = (E.f32x(a) for a in d["orc"].step_sens(d["x"], d["u"], E.DT))
    m = d["x"].shape[1]
    out = {}
    for case, mask in E.mask_cases(m).items():
        if cases is not None and case not in cases:
            continue
        args = (d["x"], d["P"], xp, A, d["z"], mask, d["Qd"], d["Rd"], E.MAG, d["eps"])
        ref, host = E.step(*args), E.host_step(*args, header=header)
        e = E.errors(host, ref)
        assert np.array_equal(host["P32"], host["P32"].transpose(1, 0, 2)), "P is not bitwise symmetric"
        assert np.array_equal(host["used"], ref["used"]) and np.array_equal(host["status"], ref["status"]) and (ref["status"] == 0).all()
        if case == "none":
            assert np.array_equal(host["X"], xp) and (host["nis"] == 0).all() and (host["ll"] == 0).all()
        out[case] = e
    if cases is None or "chain" in cases:
        c = E.chain_inputs(name)
        orc = c["orc"]
        args = (c["x"], c["P"], c["u"], c["Z"], c["masks"], c["Qd"], c["Rd"], E.MAG, c["eps"])
        ref = E.chain(E.step, orc.step_sens, *args)
        host = E.chain(lambda *a, **k: E.host_step(*a, header=header, **k), lambda *a: [E.f32x(v) for v in orc.step_sens(*a)], *args, host=True)
        assert (ref["status"] == 0).all() and np.array_equal(ref["used"], host["used"]) and np.array_equal(ref["used"], c["masks"])
        out["chain"] = E.chain_errors(host, ref)
    xs = E.measure_states(name)
    z64 = E.h(xs, E.MAG, d["eps"])
    zh = E.host_measure(xs, E.MAG, d["eps"], header)
    assert np.array_equal(zh[0:6], xs[0:6]) and np.array_equal(zh[6:9], xs[10:13])
    out["measure"] = {"mag": E.L.unit_max_rel(zh[12:15], z64[12:15])}
    return out


_MEASURED = {}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = measure(name)
    return _MEASURED[name]


def worst(m, key):
    return max(float(e[key].max()) for e in m.values() if key in e)


def check(m):
    """the assertions a measurement has to meet (the mutated headers must fail at least one)"""
    for key, bar in E.E32_WORST.items():
        assert worst(m, key) <= bar, (key, worst(m, key), bar)


@pytest.mark.parametrize("name", E.MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (ekf_ref.E32_WORST) hold on every model's grid and every mask case, so the
    GPU tests' condition e32 <= 2 x worst leaves out no instance of these inputs (the cap is 5 %)."""
    m = measured(name)
    print(f"[ekf e32] {name}: " + ", ".join(f"{k} {worst(m, k):.2e}" for k in E.E32_WORST))
    check(m)
    for case, e in m.items():
        if case != "measure":
            assert E.checked(e).all(), case


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst over the models, not a loose bound: each entry is within 3 x of what is measured."""
    for key, bar in E.E32_WORST.items():
        w = max(worst(measured(n), key) for n in E.MODELS)
        assert bar <= 3 * w, (key, w, bar)


def test_update_only_and_nan_rows_host():
    """predict = 0 against the update-only restatement; a NaN z row is a cleared mask bit, bit for bit"""
    d = E.inputs("poly")
    m = d["x"].shape[1]
    args = (d["x"], d["P"], None, None, d["z"], None, d["Qd"], d["Rd"], E.MAG, d["eps"])
    ref, host = E.step(*args, predict_=False), E.host_step(*args, predict_=False)
    e = E.errors(host, ref)
    print("[ekf e32] update only: " + ", ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    assert E.checked(e).all() and np.array_equal(host["Xpred"], d["x"])
    assert np.array_equal(host["Abar"], np.repeat(np.eye(12)[:, :, None], m, axis=2))
    z = d["z"].copy()
    z[10, ::2] = np.nan
    mask = np.full(m, E.ALL, np.int32)
    mask[::2] &= ~(1 << 10)
    a = E.host_step(d["x"], d["P"], None, None, z, None, d["Qd"], d["Rd"], E.MAG, d["eps"], predict_=False)
    b = E.host_step(d["x"], d["P"], None, None, d["z"], mask, d["Qd"], d["Rd"], E.MAG, d["eps"], predict_=False)
    for k in ("X32", "P32", "nu", "S", "nis", "ll32", "used", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["used"][::2] == (E.ALL & ~(1 << 10))).all() and (a["used"][1::2] == E.ALL).all()


def test_status_paths_host():
    d = E.inputs("poly")
    x, P, Rd, xp = d["x"][:, :4], d["P"][:, :, :4].copy(), d["Rd"][:, :4].copy(), d["x"][:, :4].copy()
    A = np.repeat(np.eye(13)[:, :, None], 4, axis=2)
    # a measurement without noise of a coordinate without variance: s = 0 exactly
    P[0, :, 1] = P[:, 0, 1] = 0.0
    Rd[0, 1] = 0.0
    xp[4, 2] = np.nan
    host = E.host_step(x, P, xp, A, d["z"][:, :4], None, np.zeros((12, 4)), Rd, E.MAG, d["eps"])
    assert list(host["status"]) == [0, 1, 2, 0]
    assert host["S"][0, 1] == 0 and host["used"][1] == E.ALL and host["used"][2] == 0
    assert (host["nu"][:, 2] == 0).all() and host["nis"][2] == 0 and host["ll"][2] == 0 and np.isnan(host["X"][4, 2])
    assert np.isfinite(host["X"][:, [0, 1, 3]]).all() and np.isfinite(host["P"][:, :, [0, 1, 3]]).all()


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "sign_flip_in_vb_cross": ("ekf_skew(vb, Sv);", "ekf_skew(vb, Sv); for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Sv[i][j] = -Sv[i][j];"),
    "dropped_Q": ("if (PREDICT && j == r) v += io.Qd[j * n + i];", ""),
    "nu_not_reduced": ("const float rho = L.nu[z] - ekf_hdot(L, L.d, z);", "const float rho = L.nu[z];"),
    "transposed_Abar": ("acc = fmaf(mr[k], s.m[1][j][k], acc);", "acc = fmaf(mr[k], s.m[1][k][j], acc);"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_ekf_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_dynamics.hpp"', f'#include "{CSRC}/ac_dynamics.hpp"')
                .replace('#include "ac_group.hpp"', f'#include "{CSRC}/ac_group.hpp"'))
    with pytest.raises(AssertionError):
        check(measure("poly", path, cases=("all", "no_gps")))


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
def _good(n=4):
    x = np.zeros((13, n))
    x[3], x[9] = 30.0, 1.0
    P = np.repeat(np.diag(E.SIG_P0 ** 2)[:, :, None], n, axis=2)
    return dict(x0=x, P0=P, q=E.SIG_Q ** 2, r=E.SIG_R ** 2)


def _asym():
    P = _good()["P0"]
    P[0, 1, 2] = 0.1
    return P


def _negdiag():
    P = _good()["P0"]
    P[5, 5, 0] = 0.0
    return P


@pytest.mark.parametrize("kw", [
    dict(x0=np.zeros((12, 4))), dict(P0=np.zeros((12, 12, 3))), dict(P0=np.zeros((12, 12))), dict(P0=_asym()), dict(P0=_negdiag()),
    dict(q=np.ones(11)), dict(q=np.ones((12, 3))), dict(q=-np.ones(12)), dict(r=np.ones(14)), dict(r=np.zeros(15)),
    dict(r=-np.ones((15, 4))), dict(r=np.full(15, np.nan)), dict(mag_ned=(1.0, 0.0)), dict(ws=np.zeros(10, np.float32)),
])
def test_ekf_argument_checks(kw):
    ac = make_aircraft("poly")
    args = _good()
    args.update(kw)
    x0, P0 = args.pop("x0"), args.pop("P0")
    with pytest.raises(ValueError):
        ac.ekf(x0, P0, **args)
    assert not ac._handle  # nothing reached the library


# ---- resources -------------------------------------------------------------------------------------------------------------------------
def test_ekf_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "ekf_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("ekf_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "ekf.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert scratch_bytes(r.stderr, "k_ekf_measure") == 0
    # both instantiations of k_ekf_step (with and without the time update)
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:] if b.startswith("_ZN2ac10k_ekf_stepILb")]
    assert len(blocks) == 2
    for b in blocks:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split("\n")[0]
        assert int(re.search(r" VGPRs: (\d+)", b).group(1)) <= 256 and int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)) <= 48 * 1024  # (three workgroups per CU)
