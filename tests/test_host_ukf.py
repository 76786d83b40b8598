"""The UKF's per-lane code (aircraft_amd/csrc/ac_ukf.hpp) compiled for the host with g++ (tests/host_ukf/ukf_host.cpp,
-DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/ukf_ref.py) on identical float32-rounded
inputs (the images of the host build's own sigma points come from the oracle, rounded), per instance and per output, over the
grids of every model, the mask cases, kappa in {0, 3} and a 20-step chain; the bitwise symmetry of P and P-; the status paths;
mutated copies of the header that these checks must catch; the argument checks of Aircraft.ukf that run before any device is
touched; the resources of the kernels from the compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests import ukf_ref as U
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_ukf")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_ukf.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
KAPPAS = (0.0, 3.0)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_ukf.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "ukf_host.cpp")
    so = os.path.join(HERE, "libukf_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp", "ac_ekf.hpp", "ac_rts.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_UKF_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_ukf_sigma.argtypes = [C.c_void_p, FP, FP, FP, C.c_long, FP, FP, FP, IP]
    lib.host_ukf_update.argtypes = [C.c_void_p, C.c_float, FP, FP, FP, FP, IP, FP, IP, FP, FP, FP, C.c_long, FP, FP, FP, FP, FP, FP, IP,
                                    IP, FP, FP, FP]
    lib.host_ukf_sigma.restype = lib.host_ukf_update.restype = C.c_int
    _LIBS[key] = lib
    return lib


def symmetric(host):
    assert np.array_equal(host["P32"], host["P32"].transpose(1, 0, 2)), "P is not bitwise symmetric"
    assert np.array_equal(host["Ppred32"], host["Ppred32"].transpose(1, 0, 2)), "P- is not bitwise symmetric"


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
def measure(name, header=None, cases=None, kappas=KAPPAS):
    """e32 of every output on the inputs of `name`, per kappa and mask case: {case: {measure: (m,)}}"""
    d = E.inputs(name)
    orc, x, P, u = d["orc"], d["x"], d["P"], d["u"]
    m = x.shape[1]
    out = {}
    for kappa in kappas:
        hs, rs = U.host_sigma(x, P, u, kappa, header), U.sigma(x, P, kappa)
        assert not hs["flag"].any() and rs["ok"].all()
        assert np.array_equal(hs["U32"], np.tile(U.c32(u), U.PTS)) and (hs["pts32"].reshape(13, U.PTS, m)[0:3, 0] == 0).all()
        out[f"sigma k{kappa:g}"] = {"sig": U.err_sig(hs["pts"], rs["pts"])}
        F = U.f32x(U.propagate(orc.state_update, hs["pts"], u))
        for case, mask in U.mask_cases(m).items():
            if cases is not None and case not in cases:
                continue
            ref = U.update(x, P, rs["L"], rs["ok"], F, d["z"], mask, d["Qd"], d["Rd"], kappa, E.MAG, d["eps"])
            host = U.host_update(x, P, hs["L32"], hs["flag"], F, d["z"], mask, d["Qd"], d["Rd"], kappa, E.MAG, d["eps"], header=header)
            symmetric(host)
            assert np.array_equal(host["used"], ref["used"]) and np.array_equal(host["status"], ref["status"]) and (ref["status"] == 0).all()
            if case == "none":
                assert np.array_equal(host["X"], host["Xpred"]) and (host["nis"] == 0).all() and (host["ll"] == 0).all()
                assert np.array_equal(host["P32"], host["Ppred32"])
            out[f"{case} k{kappa:g}"] = E.errors(host, ref)
    if cases is None or "chain" in cases:
        c = E.chain_inputs(name)
        args = (c["x"], c["P"], c["u"], c["Z"], c["masks"])

        def ref_one(x_, P_, u_, z_, mask_, ll_):
            return U.step(orc.state_update, x_, P_, u_, z_, mask_, c["Qd"], c["Rd"], 0.0, E.MAG, c["eps"])

        def host_one(x_, P_, u_, z_, mask_, ll_):
            s = U.host_sigma(x_, P_, u_, 0.0, header)
            F_ = U.f32x(U.propagate(orc.state_update, s["pts"], u_))
            return U.host_update(x_, P_, s["L32"], s["flag"], F_, z_, mask_, c["Qd"], c["Rd"], 0.0, E.MAG, c["eps"], ll_in=ll_, header=header)

        ref, host = U.chain(ref_one, *args), U.chain(host_one, *args, host=True)
        assert (ref["status"] == 0).all() and np.array_equal(ref["used"], host["used"]) and np.array_equal(ref["used"], c["masks"])
        out["chain"] = E.chain_errors(host, ref)
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
    for key, bar in U.E32_WORST.items():
        assert worst(m, key) <= bar, (key, worst(m, key), bar)


@pytest.mark.parametrize("name", E.MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (ukf_ref.E32_WORST) hold on every model's grid, every mask case, both kappas
    and the chain, so the GPU tests' condition e32 <= 2 x worst leaves out no instance of these inputs (the cap is 5 %)."""
    m = measured(name)
    print(f"[ukf e32] {name}: " + ", ".join(f"{k} {worst(m, k):.2e}" for k in U.E32_WORST))
    check(m)
    for e in m.values():
        assert U.checked(e).all()


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst over the models, not a loose bound: each entry is within 3 x of what is measured."""
    for key, bar in U.E32_WORST.items():
        w = max(worst(measured(n), key) for n in E.MODELS)
        assert bar <= 3 * w, (key, w, bar)


def test_update_only_and_nan_rows_host():
    """predict = 0 against the update-only restatement; a NaN z row is a cleared mask bit, bit for bit"""
    d = E.inputs("poly")
    m = d["x"].shape[1]
    args = (d["x"], d["P"], None, None, None, d["z"], None, d["Qd"], d["Rd"], 0.0, E.MAG, d["eps"])
    ref, host = U.update(*args, predict_=False), U.host_update(*args, predict_=False)
    e = E.errors(host, ref)
    print("[ukf e32] update only: " + ", ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    assert U.checked(e).all() and np.array_equal(host["Xpred"], d["x"]) and np.array_equal(host["Ppred"], d["P"])
    assert np.array_equal(host["Abar"], np.repeat(np.eye(12)[:, :, None], m, axis=2))
    symmetric(host)
    z = d["z"].copy()
    z[10, ::2] = np.nan
    mask = np.full(m, E.ALL, np.int32)
    mask[::2] &= ~(1 << 10)
    a = U.host_update(d["x"], d["P"], None, None, None, z, None, d["Qd"], d["Rd"], 0.0, E.MAG, d["eps"], predict_=False)
    b = U.host_update(d["x"], d["P"], None, None, None, d["z"], mask, d["Qd"], d["Rd"], 0.0, E.MAG, d["eps"], predict_=False)
    for k in ("X32", "P32", "nu", "S", "nis", "ll32", "used", "status"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["used"][::2] == (E.ALL & ~(1 << 10))).all() and (a["used"][1::2] == E.ALL).all()
    assert np.isfinite(a["X"]).all() and np.isfinite(a["P"]).all()


def status_inputs(n=4):
    """instance 1: a velocity coordinate with a variance of 1e-36, uncorrelated, measured without noise: the sigma points do not
    move it in float32 (nor in float64 next to 30 m/s), its pivot of Pzz is exactly 0 -> value 1 (a row of P that is exactly zero
    has no Cholesky factor: that is value 4, instance 3); instance 2: a NaN state -> value 2"""
    d = E.inputs("poly")
    x, P, Rd = d["x"][:, :n].copy(), d["P"][:, :, :n].copy(), d["Rd"][:, :n].copy()
    assert abs(x[3, 1]) > 1.0
    P[3, :, 1] = P[:, 3, 1] = 0.0
    P[3, 3, 1] = 1e-36
    Rd[3, 1] = 0.0
    x[4, 2] = np.nan
    P[5, :, 3] = P[:, 5, 3] = 0.0
    return d, x, E.f32x(P), Rd


def test_status_paths_host():
    d, x, P, Rd = status_inputs()
    z, Qd = d["z"][:, :4], d["Qd"][:, :4]
    host = U.host_update(x, P, None, None, None, z, None, Qd, Rd, 0.0, E.MAG, d["eps"], predict_=False)
    ref = U.update(x, P, None, None, None, z, None, Qd, Rd, 0.0, E.MAG, d["eps"], predict_=False)
    assert list(host["status"]) == [0, 1, 2, 4] and list(ref["status"]) == [0, 1, 2, 4]
    assert host["S"][3, 1] == 0 and host["used"][1] == E.ALL and host["used"][2] == 0 and host["used"][3] == 0
    for k in (2, 3):
        assert (host["nu"][:, k] == 0).all() and (host["S"][:, k] == 0).all() and host["nis"][k] == 0 and host["ll"][k] == 0
    assert np.isnan(host["X"][4, 2]) and np.array_equal(host["X32"][:, 3], U.c32(x)[:, 3]) and np.array_equal(host["P"][:, :, 3], P[:, :, 3])
    assert np.isfinite(host["X"][:, [0, 1, 3]]).all() and np.isfinite(host["P"][:, :, [0, 1, 3]]).all()
    # with the time update: a P without a factor gives 25 copies of x^ and comes back unchanged; a NaN state gives value 2
    u = d["u"][:, :4]
    s = U.host_sigma(x, P, u)
    assert list(s["flag"]) == [0, 0, 0, 1]
    pts = s["pts32"].reshape(13, U.PTS, 4)
    centre = U.c32(x)[:, 3].copy()
    centre[0:3] = 0.0
    assert all(np.array_equal(pts[:, j, 3], centre) for j in range(U.PTS))
    with np.errstate(all="ignore"):
        F = U.f32x(U.propagate(d["orc"].state_update, s["pts"], u))
    host = U.host_update(x, P, s["L32"], s["flag"], F, z, None, Qd, Rd, 0.0, E.MAG, d["eps"])
    assert host["status"][2] == 2 and host["status"][3] == 4 and host["status"][0] == 0
    assert np.array_equal(host["X32"][:, 3], U.c32(x)[:, 3]) and np.array_equal(host["P"][:, :, 3], P[:, :, 3])
    assert np.array_equal(host["Abar"][:, :, 3], np.eye(12)) and host["used"][3] == 0 and host["nis"][3] == 0


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    # (zbar = w0 z_0 + w1 sum z_j without its first term, in the centred form the header uses)
    "w0_dropped_from_the_mean": [("const float zb = z0 + w.w1 * sum;", "const float zb = (1.0f - w.w0) * z0 + w.w1 * sum;")],
    "dbar_not_subtracted": [("s.a.e[j][r] = s.a.e[j][r] - db;", "s.a.e[j][r] = s.a.e[j][r];")],
    "measurement_points_from_P": [("s.b.m[r][c] = L.pm[c];", "s.b.m[r][c] = io.P[(rr * 12 + c) * n + i];")],
    # (an unused row is replaced by a unit row whatever was added to it before, so "Rd added before the mask replaces a row" changes
    # no bit of this implementation; the Rd mutation that can be caught is the one that leaves it out)
    "rd_not_added": [("if (c == r) v += L.rd;", "")],
    "abar_with_L_transposed": [("for (int c = 11; c > j; --c) t = fmaf(-ab[c], s.b.m[c][j], t);",
                                "t = 0.f; for (int c = 0; c < 12; ++c) t = fmaf(D[c], s.b.m[j][c], t);"),
                               ("ab[j] = t / s.b.m[j][j];", "ab[j] = t;")],
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    text = open(HEADER).read()
    for old, new in MUTATIONS[which]:
        assert text.count(old) == 1, (which, old)
        text = text.replace(old, new)
    path = str(tmp_path / f"ac_ukf_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace('#include "ac_rts.hpp"', f'#include "{CSRC}/ac_rts.hpp"'))
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
    dict(kappa=-1.0), dict(kappa=float("nan")), dict(kappa=float("inf")), dict(kappa=np.ones(2)), dict(kappa=True),
])
def test_ukf_argument_checks(kw):
    ac = make_aircraft("poly")
    args = _good()
    args.update(kw)
    x0, P0 = args.pop("x0"), args.pop("P0")
    with pytest.raises(ValueError):
        ac.ukf(x0, P0, **args)
    assert not ac._handle  # nothing reached the library


# ---- resources -------------------------------------------------------------------------------------------------------------------------
# what DESIGN.md §4.18 states: VGPRs, LDS bytes per workgroup, waves per SIMD
RESOURCES = {"_ZN2ac11k_ukf_sigma": (52, 15360, 8), "_ZN2ac12k_ukf_updateILb1": (176, 44032, 2), "_ZN2ac12k_ukf_updateILb0": (160, 44032, 3)}


def test_ukf_kernel_resources(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "ukf_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("ukf_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "ukf.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert scratch_bytes(r.stderr, "k_ukf_sigma") == 0
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    for prefix, (vgprs, lds, occ) in RESOURCES.items():
        (b,) = [b for b in blocks if b.startswith(prefix)]
        got = tuple(int(re.search(p, b).group(1)) for p in (r" VGPRs: (\d+)", r"LDS Size \[bytes/block\]: (\d+)", r"Occupancy \[waves/SIMD\]: (\d+)"))
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, prefix
        assert got == (vgprs, lds, occ), (prefix, got)
