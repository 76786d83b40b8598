"""The iterated Kalman smoother's per-lane code (aircraft_amd/csrc/ac_ieks.hpp) compiled for the host with g++
(tests/host_ieks/ieks_host.cpp, -DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/ieks_ref.py) on
identical float32-rounded inputs, per instance and per output of the pass and of the cost, over the chains of every model; the
bitwise symmetry of Ps and Ppreds; the anchor against the EKF's host build (T = 1, nominal (x0, F(x0, u)): Ppred and Abar bit for
bit); the status and restart rule; the candidates and the accept decision; mutated copies of the header that the Gauss-Newton
property must catch; the argument checks of EKF.map_smooth that run before any device is touched; the register, LDS and scratch
figures of the kernels from the compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests import ieks_ref as I
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_ieks")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_ieks.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_ieks.hpp, or of the copy `header` (built next to that copy)"""
    from aircraft_amd import _lib

    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "ieks_host.cpp")
    so = os.path.join(HERE, "libieks_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp", "ac_ekf.hpp", "ac_rts.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_IEKS_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_ieks_pass.argtypes = [C.POINTER(_lib.EkfOpts), C.c_float] + [FP] * 6 + [IP, FP, FP, C.c_long, C.c_long] + [FP] * 6 + [IP, IP] + [FP] * 3
    lib.host_ieks_cost.argtypes = [C.POINTER(_lib.EkfOpts), C.c_float] + [FP] * 5 + [IP, FP, FP, C.c_long, C.c_long, C.c_long] + [FP] * 4 + [IP]
    lib.host_ieks_candidates.argtypes = [FP] * 5 + [C.c_int, C.c_long, C.c_long, FP, FP]
    lib.host_ieks_accept.argtypes = [FP, FP, IP, FP, FP, C.c_int, C.c_long, C.c_long, FP, FP, FP, IP]
    for f in (lib.host_ieks_pass, lib.host_ieks_cost, lib.host_ieks_candidates, lib.host_ieks_accept):
        f.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement (item 5) ------------------------------------------------------------------------------------------------
MEASURE_T = (1, 2, 5, I.DESCENT_T)  # the GPU tests' lengths and the descent's


def measure(name):
    """e32 of every output of the pass and of the cost about the EKF + RTS nominal of ieks_ref.inputs(name), worst over the
    lengths MEASURE_T -> {measure: (m,)}"""
    per = [measure_at(name, T_) for T_ in MEASURE_T]
    return {k: np.max([e[k] for e in per], axis=0) for k in per[0]}


def measure_at(name, T_):
    d = I.inputs(name, T_=T_)
    F, A = I.linearise(d["orc"], d["Xekf"], d["U"])
    F, A = I.f32x(F), I.f32x(A)
    a = (d["X0"], d["P"], d["Xekf"], F, A, d["Z"], d["masks"], d["Qd"], d["Rd"], E.MAG, d["eps"])
    ref, host = I.pass_(*a), I.host_pass(*a)
    assert np.array_equal(host["P32"], host["P32"].transpose(0, 2, 1, 3)), "Ps is not bitwise symmetric"
    assert np.array_equal(host["Ppred32"], host["Ppred32"].transpose(0, 2, 1, 3)), "Ppreds is not bitwise symmetric"
    assert np.array_equal(host["status"], ref["status"]) and (ref["status"] == 0).all()
    assert np.array_equal(host["used"], ref["used"]) and (ref["used"] == E.ALL).all()
    e = I.pass_errors(host, ref)
    # the cost of that nominal and of the ladder's candidates about it, in one batch
    Xc, Uc = I.candidates(d["Xekf"], I.nodes(I.smooth(ref)), d["U"])
    Xc = I.f32x(np.concatenate([d["Xekf"], Xc], axis=2)[:, :, :4 * d["X0"].shape[1]])
    Fc = I.f32x(I.images(d["orc"], Xc, np.concatenate([d["U"]] * 4, axis=2)))
    c = (d["X0"], d["P"], Xc, Fc, d["Z"], d["masks"], d["Qd"], d["Rd"], E.MAG, d["eps"])
    cref, chost = I.cost(*c), I.host_cost(*c)
    assert np.array_equal(chost["status"], cref["status"]) and (cref["status"] == 0).all()
    m = d["X0"].shape[1]
    e.update({k: v.reshape(4, m).max(0) for k, v in I.cost_errors(chost, cref).items()})
    return e


_MEASURED = {}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = measure(name)
    return _MEASURED[name]


@pytest.mark.parametrize("name", E.MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (ieks_ref.E32_WORST) hold on every model's chain and every instance is inside
    2 x them: the reference itself does not need the GPU tests' 5 % allowance."""
    e = measured(name)
    print(f"[ieks e32] {name}: " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in e.items()))
    for k, bar in I.E32_WORST.items():
        assert float(e[k].max()) <= bar, (k, float(e[k].max()), bar)
    assert I.checked(e).all()


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst over the models, not a loose bound: each entry is within 3 x of what is measured."""
    for k, bar in I.E32_WORST.items():
        w = max(float(measured(n)[k].max()) for n in E.MODELS)
        assert bar <= 3 * w, (k, w, bar)


# ---- the anchor (item 2) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_anchor_against_the_filter_step(name):
    """T = 1 about the nominal (x0, F(x0, u)): the pass is the EKF step.  Ppred and Abar equal the EKF host build's bit for bit; Xs,
    Ps, nu, S are within the e32 bars (the two differ only by the rounding of c_0 and of x0 [-] x0)."""
    d = E.inputs(name)
    xp, A = d["orc"].step_sens(d["x"], d["u"], E.DT)[:2]
    xp, A = I.f32x(xp), I.f32x(A)
    ekf = E.host_step(d["x"], d["P"], xp, A, d["z"], None, d["Qd"], d["Rd"], E.MAG, d["eps"])
    got = I.host_pass(d["x"], d["P"], np.stack([d["x"], xp]), xp[None], A[None], d["z"][None], None, d["Qd"], d["Rd"], E.MAG, d["eps"])
    assert np.array_equal(got["Ppred"][0], ekf["Ppred"]) and np.array_equal(got["Abar"][0], ekf["Abar"])
    assert np.array_equal(got["used"][0], ekf["used"]) and np.array_equal(got["status"][0], ekf["status"])
    e = E.errors({k: got[k][0] for k in ("X", "P", "nu", "S", "nis")} | {"ll": got["ll"]}, ekf)
    print(f"[ieks anchor] {name}: " + ", ".join(f"{k} {float(v.max()):.2e}" for k, v in e.items()))
    for k in ("x", "P", "nu", "S"):
        assert float(e[k].max()) <= I.E32_WORST[k], (k, float(e[k].max()))


# ---- status and the restart rule -----------------------------------------------------------------------------------------------------
def test_status_and_restart_rule_host():
    """A NaN z and a cleared mask bit leave the row out; a row with s <= 0 is rejected; a nominal node that is not finite sets bit 2
    at the two steps that read it, no row is applied there, Xs is the nominal node bit for bit and the recursion restarts from
    d = 0 and P = P- where all of P- is finite (the step that reads the node as Xbar[k+1] only), else P = P0 (the step whose Abar
    it enters, and a step whose F is not finite)."""
    d = I.inputs("poly")
    m = d["X0"].shape[1]
    assert m >= 4
    F, A = I.linearise(d["orc"], d["Xekf"], d["U"])
    F, A, Xb, Z, Rd = I.f32x(F), I.f32x(A), d["Xekf"].copy(), d["Z"].copy(), d["Rd"].copy()
    masks = d["masks"].copy()
    Z[2, 7, 0] = np.nan
    masks[3, 0] &= ~(1 << 4)
    Rd[9, 1] = -1.0e6                       # s <= 0 at row 9 of every step
    Xb[3, 7, 2] = np.nan                    # the attitude of node 2 of instance 2: read by steps 2 (as Xbar[k+1]) and 3 (as Xbar[k])
    F[4, 8, 3] = np.inf                     # the attitude of F_4 of instance 3
    a = (d["X0"], d["P"], Xb, F, A, Z, masks, d["Qd"], Rd, E.MAG, d["eps"])
    ref, host = I.pass_(*a), I.host_pass(*a)
    want = np.zeros_like(ref["status"])
    want[:, 1] = 1
    want[2, 2] = want[3, 2] = want[4, 3] = 2
    assert np.array_equal(ref["status"], want) and np.array_equal(host["status"], want)
    used = np.full_like(ref["used"], E.ALL)
    used[2, 0] &= ~(1 << 7)
    used[3, 0] &= ~(1 << 4)
    used[2, 2] = used[3, 2] = used[4, 3] = 0
    assert np.array_equal(ref["used"], used) and np.array_equal(host["used"], used)
    assert host["nu"][2, 7, 0] == 0 and host["S"][3, 4, 0] == 0 and host["S"][2, 9, 1] < 0
    for k, i in ((2, 2), (3, 2), (4, 3)):
        assert np.array_equal(host["X32"][k][:, i], I.c32(Xb[k + 1])[:, i], equal_nan=True)
        assert (host["nu"][k][:, i] == 0).all() and host["nis"][k, i] == 0
    # P after the restart: P- where all of it is finite, else P0
    assert np.array_equal(host["P32"][2][:, :, 2], host["Ppred32"][2][:, :, 2]) and np.isfinite(host["Ppred32"][2][:, :, 2]).all()
    assert not np.isfinite(host["Ppred32"][3][:, :, 2]).all() and np.array_equal(host["P32"][3][:, :, 2], I.c32(d["P"])[:, :, 2])
    assert not np.isfinite(host["Ppred32"][4][:, :, 3]).all() and np.array_equal(host["P32"][4][:, :, 3], I.c32(d["P"])[:, :, 3])
    # the recursion goes on: the steps after are finite and agree with the restatement
    assert np.isfinite(host["X"][4:, :, 2]).all() and np.isfinite(host["X"][5:, :, 3]).all()
    cols = np.array([0] + list(range(4, m)))
    sub = lambda r: {k: v[..., cols] for k, v in r.items() if k in ref}  # noqa: E731
    e = I.pass_errors(sub(host), sub(ref))
    for k, v in e.items():
        assert float(v.max()) <= 2 * I.E32_WORST[k], (k, v)
    for i in (2, 3):
        assert float(E.err_state(host["X"][5][:, i:i + 1], ref["X"][5][:, i:i + 1]).max()) <= 2 * I.E32_WORST["x"]
        assert float(E.err_P(host["P"][5][:, :, i:i + 1], ref["P"][5][:, :, i:i + 1]).max()) <= 2 * I.E32_WORST["P"]


def test_cost_status_host():
    """P0 that is not PD, a trajectory node that is not finite, Qd_j = 0 with and without a defect in that row"""
    d = I.inputs("poly")
    m = d["X0"].shape[1]
    Xt, P0, Qd = d["Xekf"].copy(), d["P"].copy(), d["Qd"].copy()
    P0[:, :, 0] *= -1.0
    Xt[2, 4, 1] = np.nan
    Qd[1, 2] = 0.0                           # a defect in that row: the nominal is no rollout
    Qd[1, 3] = 0.0
    for k in range(d["U"].shape[0]):         # no defect in row 1 (an additive coordinate: the difference is exactly 0)
        Xt[k + 1, 1, 3] = I.f32x(d["orc"].state_update(Xt[k][:, 3:4], d["U"][k][:, 3:4], E.DT))[1, 0]
    a = (d["X0"], P0, Xt, I.f32x(I.images(d["orc"], Xt, d["U"])), d["Z"], d["masks"], Qd, d["Rd"], E.MAG, d["eps"])
    ref, host = I.cost(*a), I.host_cost(*a)
    want = np.zeros(m, np.int64)
    want[0], want[1], want[2] = I.P0_NOT_PD, I.NONFINITE, I.QZERO_DEFECT
    assert np.array_equal(ref["status"], want) and np.array_equal(host["status"], want)
    keep = np.arange(m) >= 2
    e = I.cost_errors({k: host[k][keep] for k in I.COST_KEYS}, {k: ref[k][keep] for k in I.COST_KEYS})
    for k, v in e.items():
        assert float(v.max()) <= 2 * I.E32_WORST[k], (k, v)


# ---- candidates and accept -------------------------------------------------------------------------------------------------------------
def test_candidates_and_accept_host():
    d = I.inputs("poly")
    m, T_ = d["X0"].shape[1], d["U"].shape[0]
    F, A = I.linearise(d["orc"], d["Xekf"], d["U"])
    Xs = I.f32x(I.nodes(I.smooth(I.pass_(d["X0"], d["P"], d["Xekf"], F, A, d["Z"], d["masks"], d["Qd"], d["Rd"], E.MAG, d["eps"]))))
    ref, refU = I.candidates(d["Xekf"], Xs, d["U"])
    Xc, Uc = I.host_candidates(d["Xekf"], Xs, d["U"])
    assert np.array_equal(Uc, I.c32(refU))
    for k in range(T_ + 1):
        assert float(E.err_state(Xc[k].astype(np.float64), ref[k]).max()) <= I.E32_WORST["x"]
    # crafted costs: instance 0 takes the first candidate, 1 the third, 2 none, 3 would take the first but its trajectory is not finite
    Jcur = np.full(m, 10.0)
    Jc = np.full((4, m), 11.0)
    Jc[0, 0], Jc[2, 1], Jc[3, 1], Jc[0, 3], Jc[1, 3] = 9.0, 8.0, 7.0, 5.0, 9.5
    stc = np.zeros((4, m), np.int32)
    stc[0, 3], stc[1, 3] = I.NONFINITE, I.QZERO_DEFECT
    st0 = np.zeros(m, np.int32)
    st0[2] = I.P0_NOT_PD
    rX, ra, rJ, rs, _ = I.accept(Jcur, Jc.reshape(-1), stc.reshape(-1), Xc.astype(np.float64), d["Xekf"], st0)
    hX, ha, hJ, hs = I.host_accept(Jcur, Jc.reshape(-1), stc.reshape(-1), Xc, d["Xekf"], st0)
    assert np.array_equal(ha[:4], [1.0, 0.25, 0.0, 0.5]) and np.array_equal(hJ[:4], [9.0, 8.0, 10.0, 9.5])
    assert np.array_equal(hs[:4], [0, 0, I.P0_NOT_PD | I.NO_DECREASE, I.QZERO_DEFECT])
    assert np.array_equal(ha, ra) and np.array_equal(hJ, rJ) and np.array_equal(hs, rs) and np.array_equal(hX, I.c32(rX))
    assert np.array_equal(hX[:, :, 2], I.c32(d["Xekf"])[:, :, 2]) and np.array_equal(hX[:, :, 0], Xc[:, :, 0])


# ---- mutated headers must fail (item 6) --------------------------------------------------------------------------------------------
MUTATIONS = {
    "c_dropped": ("s.dm[r] = cr + acc;", "s.dm[r] = acc;"),
    "measured_at_the_prediction": ("ekf_measure<true>(eps, o.mag_ned, L.e.xm, m);", "ekf_measure<true>(eps, o.mag_ned, xp, m);"),
    "Qd_omitted": ("if (j == r) v += L.q;", ""),
    "d_starts_at_zero": ("rts_minus(x0, L.e.xm, L.e.d);", "for (int j = 0; j < 12; ++j) L.e.d[j] = 0.f;"),
}
GN_SCALES = (0.5, 0.25)


def gauss_newton_check(pass_fn, name="poly"):
    """item 1 of tests/test_ieks_ref.py on `pass_fn`: the relative mismatch against the dense problem halves with the scale"""
    big, small = (I.gn_mismatch(pass_fn, I.gn_case(name, s)) for s in GN_SCALES)
    print(f"[ieks gn] {name}: {big} -> {small}")
    assert (small < big).all(), (big, small)
    assert ((big / small >= 1.5) & (big / small <= 2.5)).all(), big / small


def test_host_build_has_the_gauss_newton_property():
    gauss_newton_check(I.host_pass)


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_ieks_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_rts.hpp"', f'#include "{CSRC}/ac_rts.hpp"'))
    with pytest.raises(AssertionError):
        gauss_newton_check(lambda *a: I.host_pass(*a, header=path))


# ---- Python argument checks (before any device call; item 7) -----------------------------------------------------------------------------
def _bank(n=4):
    import torch

    from aircraft_amd import EKF

    ac = make_aircraft("poly")
    z = lambda *s: torch.zeros(s)  # noqa: E731
    return ac, EKF(ac, z(13, n), z(12, 12, n), z(12, n), z(15, n), E.MAG, z(8), True, False)


@pytest.mark.parametrize("kw", [
    dict(iters=-1), dict(iters=2.5), dict(iters=True), dict(ladder=()), dict(ladder=(1, 1)), dict(ladder=(0.5, 1.0)), dict(ladder=(1.5,)),
    dict(ladder=(1, 0)), dict(ladder=tuple([1.0 / (k + 1) for k in range(9)])), dict(ladder="x"), dict(init="filter"),
    dict(init=np.zeros((3, 13, 4))), dict(init=np.zeros((4, 12, 4))), dict(init=np.zeros((4, 13, 5))), dict(Z=np.zeros((3, 14, 4))),
    dict(Z=np.zeros((0, 15, 4))), dict(U=np.zeros((2, 7, 4))), dict(mask=np.zeros((3, 5), np.int32)), dict(dt=0.0), dict(dt=np.nan),
])
def test_map_smooth_argument_checks(kw):
    ac, bank = _bank()
    a = dict(U=np.zeros((3, 7, 4)), dt=0.01, Z=np.zeros((3, 15, 4)))
    a.update(kw)
    with pytest.raises(ValueError):
        bank.map_smooth(a.pop("U"), a.pop("dt"), a.pop("Z"), **a)
    assert not ac._handle  # nothing reached the library


def test_map_smooth_rejects_a_smooth_without_initial_node():
    from aircraft_amd import EkfMapSmooth, EkfSmooth

    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.map_smooth(np.zeros((3, 7, 4)), 0.01, np.zeros((3, 15, 4)), init=EkfSmooth(np.zeros((3, 13, 4)), None, None, None, None, None))
    assert not ac._handle
    assert [f for f in EkfMapSmooth.__dataclass_fields__][:8] == ["X", "P", "X0", "P0", "cost", "alpha", "status", "trace"]


# ---- resources ---------------------------------------------------------------------------------------------------------------------------
def test_kernel_resources(tmp_path):
    """the forward kernel keeps its lane state in registers (0 B scratch) within the register file of one wave per SIMD and its
    mirrors within 48 KiB + the bank pad; the other kernels use no scratch either"""
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "ieks_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("ieks_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "ieks.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("k_ieks_filter", "k_ieks_candidates", "k_ieks_cost_nodes", "k_ieks_cost_reduce", "k_ieks_accept"):
        assert scratch_bytes(r.stderr, k) == 0, k
    b = [b for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:] if "k_ieks_filter" in b.split("\n")[0]]
    assert len(b) == 1
    vgpr, agpr = int(re.search(r" VGPRs: (\d+)", b[0]).group(1)), int(re.search(r" AGPRs: (\d+)", b[0]).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b[0]).group(1))
    print(f"[ieks resources] k_ieks_filter: {vgpr} VGPRs, {agpr} AGPRs, {lds} B LDS")
    assert vgpr + agpr <= 512 and lds == 16 * 784 * 4 and lds <= 64 * 1024
