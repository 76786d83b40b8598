"""The RTS smoother's per-lane code (aircraft_amd/csrc/ac_rts.hpp) compiled for the host with g++ (tests/host_rts/rts_host.cpp,
-DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/rts_ref.py) on identical float32-rounded
records, per instance and per measure, over the filter chains of every model, with and without the initial node; the bitwise
symmetry of P^s, the bit-for-bit copy of the last node and the status; mutated copies of the header that these checks must
catch; the argument checks of EKF.smooth that run before any device is touched; the scratch budget of the kernel from the
compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests import rts_ref as R
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_rts")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_rts.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_rts.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "rts_host.cpp")
    so = os.path.join(HERE, "librts_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp", "ac_ekf.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_RTS_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_rts_smooth.argtypes = [FP] * 7 + [C.c_long, C.c_long] + [FP] * 5 + [IP]
    lib.host_rts_smooth.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
def measure(name, header=None, cases=(True, False)):
    """e32 of every measure on the records of the float64 filter chain of `name`: {initial: {measure: (m,)}}"""
    rec = R.chain_records(name)
    out = {}
    for initial in cases:
        args = [rec[k] for k in ("X", "P", "Xpred", "Ppred", "Abar")] + ([rec["X0"], rec["P0"]] if initial else [])
        ref, host = R.smooth(*args), R.host_smooth(*args, header=header)
        assert np.array_equal(host["P32"], host["P32"].transpose(0, 2, 1, 3)), "P^s is not bitwise symmetric"
        if initial:
            assert np.array_equal(host["P032"], host["P032"].transpose(1, 0, 2)), "P^s of node -1 is not bitwise symmetric"
        else:
            assert host["X0"] is None and (host["C"][0] == 0).all()
        assert np.array_equal(host["X"][-1], rec["X"][-1]) and np.array_equal(host["P"][-1], rec["P"][-1]), "node T-1 is the filtered one"
        assert np.array_equal(host["status"], ref["status"]) and (ref["status"] == 0).all()
        out[initial] = R.errors(host, ref, rec, initial)
    return out


_MEASURED = {}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = measure(name)
    return _MEASURED[name]


def worst(m, key):
    return max(float(e[key].max()) for e in m.values())


def check(m):
    """the assertions a measurement has to meet (the mutated headers must fail at least one)"""
    for key, bar in R.E32_WORST.items():
        assert worst(m, key) <= bar, (key, worst(m, key), bar)


@pytest.mark.parametrize("name", E.MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (rts_ref.E32_WORST) hold on every model's chain, with and without the initial
    node, and every instance is inside 2 x them: the reference itself does not need the GPU tests' 5 % allowance."""
    m = measured(name)
    print(f"[rts e32] {name}: " + ", ".join(f"{k} {worst(m, k):.2e}" for k in R.E32_WORST))
    check(m)
    for e in m.values():
        assert R.checked(e).all()


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst over the models, not a loose bound: each entry is within 3 x of what is measured."""
    for key, bar in R.E32_WORST.items():
        w = max(worst(measured(n), key) for n in E.MODELS)
        assert bar <= 3 * w, (key, w, bar)


def test_gains_are_optional_host():
    rec = R.chain_records("poly")
    args = [rec[k] for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")]
    a, b = R.host_smooth(*args), R.host_smooth(*args, gains=False)
    assert b["C"] is None
    for k in ("X", "P", "X0", "P0", "status"):
        assert np.array_equal(a[k], b[k]), k


def test_short_traces_host():
    """T = 1 is a copy (and one link with the initial node); T = 2 is one link"""
    rec = R.chain_records("poly")
    for T_ in (1, 2):
        for initial in (False, True):
            args = [rec[k][:T_] for k in ("X", "P", "Xpred", "Ppred", "Abar")] + ([rec["X0"], rec["P0"]] if initial else [])
            ref, host = R.smooth(*args), R.host_smooth(*args)
            assert np.array_equal(host["X"][-1], rec["X"][T_ - 1]) and np.array_equal(host["P"][-1], rec["P"][T_ - 1])
            assert np.array_equal(host["status"], ref["status"]) and (host["status"] == 0).all()
            assert R.checked(R.errors(host, ref, rec, initial)).all(), (T_, initial)


def test_status_paths_host():
    """a non-PD P- at one link, a NaN record at one link: the bits are set, the gain is zero, the node before is the filtered one
    bit for bit, the nodes further back are smoothed again from it, and the host build agrees with the restatement"""
    rec = {k: v[..., :4].copy() for k, v in R.chain_records("poly").items()}
    T_ = rec["X"].shape[0]
    rec["Ppred"][12][:, :, 1] *= -1.0        # not positive definite
    rec["Abar"][7][3, 4, 2] = np.nan          # an operand that is not finite
    rec["Xpred"][15][8, 3] = np.inf
    rec["Ppred"][5][2, 2, 3] = 0.0            # a zero pivot
    args = [rec[k] for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")]
    ref, host = R.smooth(*args), R.host_smooth(*args)
    want = np.zeros((T_, 4), np.int32)
    want[12, 1], want[7, 2], want[15, 3], want[5, 3] = R.NOT_PD, R.NONFINITE, R.NONFINITE, R.NOT_PD
    assert np.array_equal(ref["status"], want) and np.array_equal(host["status"], want)
    for k, i in ((12, 1), (7, 2), (15, 3), (5, 3)):
        assert np.array_equal(host["X"][k - 1][:, i], rec["X"][k - 1][:, i]) and np.array_equal(host["P"][k - 1][:, :, i], rec["P"][k - 1][:, :, i])
        assert (host["C"][k][:, :, i] == 0).all() and (host["C"][k - 1][:, :, i] != 0).any()
        assert not np.array_equal(host["P"][k - 2][:, :, i], rec["P"][k - 2][:, :, i])  # smoothed again further back
    assert np.isfinite(host["X"]).all() and np.isfinite(host["P"]).all() and np.isfinite(host["C"]).all()
    clean = R.host_smooth(*[R.chain_records("poly")[k][..., :4] for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")])
    for k in ("X", "P", "C", "status", "X0", "P0"):
        assert np.array_equal(host[k][..., 0], clean[k][..., 0]), k  # the untouched instance
    # (the gain measure scales by the crafted links' own P-, which has no square root: x and P^s alone)
    assert R.checked(R.errors({k: host[k] for k in ("X", "P", "X0", "P0")}, ref, rec, True)).all()


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "Abar_untransposed": ("acc = fmaf(L.cur.p[c], s.m[1][q][c], acc);", "acc = fmaf(L.cur.p[c], s.m[1][c][q], acc);"),
    "P_for_Ppred_in_the_solve": ("const float ch = L.cur.pm[j];", "const float ch = io.Pf[((size_t)k * 144 + (r < kEkfN ? r : 0) * 12 + j) * n + i];"),
    "symmetrisation_dropped": ("const float v = 0.5f * (L.x[j] + s.m[0][j][rc]);", "const float v = L.x[j];"),
    "difference_sign_flipped": ("s.m[2][r][j] = L.ps[j] - L.cur.pm[j];", "s.m[2][r][j] = L.cur.pm[j] - L.ps[j];"),
    "minus_against_the_filtered_state": ("for (int c = 0; c < 13; ++c) xm[c] = s.xm[c];", "for (int c = 0; c < 13; ++c) xm[c] = io.Xf[((size_t)k * 13 + c) * n + i];"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_rts_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_ekf.hpp"', f'#include "{CSRC}/ac_ekf.hpp"'))
    with pytest.raises(AssertionError):
        check(measure("poly", path, cases=(False,)))


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
def _bank(n=4):
    import torch

    from aircraft_amd import EKF

    ac = make_aircraft("poly")
    z = lambda *s: torch.zeros(s)  # noqa: E731
    return ac, EKF(ac, z(13, n), z(12, 12, n), z(12, n), z(15, n), E.MAG, z(8), True, False)


def _trace(n=4, T_=3, **kw):
    from aircraft_amd import EkfTrace

    z = lambda *s: np.zeros(s)  # noqa: E731
    f = dict(X=z(T_, 13, n), P=z(T_, 12, 12, n), nu=z(T_, 15, n), S=z(T_, 15, n), nis=z(T_, n), ll=z(n), used=z(T_, n), status=z(T_, n),
             Xpred=z(T_, 13, n), Ppred=z(T_, 12, 12, n), Abar=z(T_, 12, 12, n), X0=z(13, n), P0=z(12, 12, n))
    f.update(kw)
    return EkfTrace(**f)


@pytest.mark.parametrize("kw", [
    dict(Xpred=None), dict(Ppred=None), dict(Abar=None), dict(X0=None), dict(P0=None), dict(X=np.zeros((3, 12, 4))),
    dict(P=np.zeros((3, 12, 12, 5))), dict(Xpred=np.zeros((2, 13, 4))), dict(Ppred=np.zeros((3, 12, 4))), dict(Abar=np.zeros((3, 12, 12))),
    dict(X0=np.zeros((13, 3))), dict(P0=np.zeros((12, 4))), dict(X=np.zeros((13, 4))),
])
def test_smooth_argument_checks(kw):
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.smooth(_trace(**kw))
    assert not ac._handle  # nothing reached the library


def test_trace_fields_keep_their_positions():
    from aircraft_amd import EkfSmooth, EkfTrace

    t = EkfTrace(1, 2, 3, 4, 5, 6, 7, 8)
    assert (t.X, t.P, t.nu, t.S, t.nis, t.ll, t.used, t.status) == (1, 2, 3, 4, 5, 6, 7, 8)
    assert t.Xpred is None and t.Ppred is None and t.Abar is None and t.X0 is None and t.P0 is None
    assert [f for f in EkfSmooth.__dataclass_fields__] == ["X", "P", "X0", "P0", "C", "status"]
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.smooth(t)  # a trace without records
    assert not ac._handle


# ---- resources -------------------------------------------------------------------------------------------------------------------------
def test_smoother_kernel_uses_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "rts_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("rts_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "rts.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert scratch_bytes(r.stderr, "k_ekf_smooth") == 0
    b = [b for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:] if "k_ekf_smooth" in b.split("\n")[0]]
    assert len(b) == 1
    assert int(re.search(r" VGPRs: (\d+)", b[0]).group(1)) <= 256 and int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b[0]).group(1)) <= 48 * 1024  # (three workgroups per CU)
