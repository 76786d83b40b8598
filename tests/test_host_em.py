"""The per-lane code of the EM statistics for the EKF's noise variances (aircraft_amd/csrc/ac_em.hpp) compiled for the host with
g++ (tests/host_em/em_host.cpp, -DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/em_ref.py) on
identical float32-rounded records and smoothed traces, per instance and per measure, over the filter chains of every model;
counts, status and the new variances; the planted failure paths; mutated copies of the header that these checks must catch;
the argument checks of EKF.set_noise / noise_stats / fit_noise that run before any device is touched; the scratch and LDS
budget of the kernel from the compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import ekf_ref as E
from tests import em_ref as M
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_em")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_em.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_em.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "em_host.cpp")
    so = os.path.join(HERE, "libem_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp", "ac_dynamics.hpp", "ac_ekf.hpp", "ac_rts.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_EM_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_em_stats.argtypes = [FP, C.c_float, C.c_float] + [FP] * 5 + [IP, FP, FP, C.c_long, C.c_long, FP, FP, IP, IP, IP, FP, FP]
    lib.host_em_stats.restype = C.c_int
    lib.host_em_chunk.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
LENGTHS = (None, 1, 2, 3)  # the whole chain and its first nodes


def measure(name, header=None, lengths=LENGTHS):
    """e32 of every measure on the chain of `name`, worst over the trace lengths: {measure: (m,)}; counts, status and new variances
    are checked on the way"""
    c = M.chain_case(name)
    worst = None
    for T_ in lengths:
        args = [c[k][:T_] if k not in ("Qd", "Rd") else c[k] for k in M.ARGS]
        ref, host = M.noise_stats(*args, eps=c["eps"]), M.host_noise_stats(*args, eps=c["eps"], header=header)
        assert (ref["status"] == 0).all() and np.array_equal(host["status"], ref["status"])
        assert np.array_equal(host["nq"], ref["nq"]) and np.array_equal(host["nr"], ref["nr"]), "counts"
        if T_ is None:
            assert (ref["nq"] == c["Xpred"].shape[0]).all() and (ref["nr"][6:] == c["Xpred"].shape[0]).all() and (ref["nr"][:6] == 4).all()
            if header is None:  # the new variances are the means (no floor is active on these chains)
                assert np.abs(host["Qn"] / ref["Qn"] - 1).max() <= 1e-3 and np.abs(host["Rn"] / ref["Rn"] - 1).max() <= 1e-3
        e = M.errors(host, ref)
        worst = e if worst is None else {k: np.maximum(worst[k], e[k]) for k in e}
    return worst


_MEASURED = {}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = measure(name)
    return _MEASURED[name]


def check(m):
    """the assertions a measurement has to meet (the mutated headers must fail at least one)"""
    for key, bar in M.E32_WORST.items():
        assert float(m[key].max()) <= bar, (key, float(m[key].max()), bar)


@pytest.mark.parametrize("name", E.MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (em_ref.E32_WORST) hold on every model's chain, and every instance is inside
    2 x them: the reference itself does not need the GPU tests' 5 % allowance."""
    m = measured(name)
    print(f"[em e32] {name}: " + ", ".join(f"{k} {float(m[k].max()):.2e}" for k in M.E32_WORST))
    check(m)
    assert M.checked(m).all()


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst over the models, not a loose bound: each entry is within 3 x of what is measured."""
    for key, bar in M.E32_WORST.items():
        w = max(float(measured(n)[key].max()) for n in E.MODELS)
        assert bar <= 3 * w, (key, w, bar)


def test_chunk_length_is_the_contract():
    from aircraft_amd import _lib

    assert lib_host().host_em_chunk() == _lib.EM_CHUNK == 32


def test_new_variances_are_optional_and_floored_host():
    c = M.chain_case("poly")
    args = [c[k] for k in M.ARGS]
    a, b = M.host_noise_stats(*args, eps=c["eps"]), M.host_noise_stats(*args, eps=c["eps"], new=False)
    assert b["Qn"] is None and b["Rn"] is None
    for k in ("Q32", "R32", "nq", "nr", "status"):
        assert np.array_equal(a[k], b[k]), k
    # floor_rel 0 means 1e-4; a floor above every mean gives floor x input
    d = M.host_noise_stats(*args, eps=c["eps"], floor=1e-4)
    assert np.array_equal(a["Qn32"], d["Qn32"]) and np.array_equal(a["Rn32"], d["Rn32"])
    big = M.host_noise_stats(*args, eps=c["eps"], floor=1e6)
    assert np.array_equal(big["Qn32"], np.float32(1e6) * E.c32(c["Qd"])) and np.array_equal(big["Rn32"], np.float32(1e6) * E.c32(c["Rd"]))


def test_short_and_chunked_traces_host():
    """T = 0 (zero sums and counts, Qn, Rn the inputs bit for bit), T = 1, and traces across the chunk boundary: the chain tiled
    in time to 2 kEmChunk + 5 nodes against float64 (the nodes are independent, so any order of records is a valid input)"""
    c = M.chain_case("poly")
    for T_ in (0, 1, 2):
        args = [c[k][:T_] if k not in ("Qd", "Rd") else c[k] for k in M.ARGS]
        ref, host = M.noise_stats(*args, eps=c["eps"]), M.host_noise_stats(*args, eps=c["eps"])
        assert np.array_equal(host["nq"], ref["nq"]) and np.array_equal(host["nr"], ref["nr"]) and (host["nq"] == T_).all()
        if T_ == 0:
            assert (host["Q32"] == 0).all() and (host["R32"] == 0).all() and (host["nr"] == 0).all()
            assert np.array_equal(host["Qn32"], E.c32(c["Qd"])) and np.array_equal(host["Rn32"], E.c32(c["Rd"]))
        else:
            assert M.checked(M.errors(host, ref)).all(), T_
    reps = (2 * 32 + 5 + 19) // 20
    args = [np.concatenate([c[k]] * reps)[:2 * 32 + 5] if k not in ("Qd", "Rd") else c[k] for k in M.ARGS]
    ref, host = M.noise_stats(*args, eps=c["eps"]), M.host_noise_stats(*args, eps=c["eps"])
    assert (host["nq"] == 69).all() and np.array_equal(host["nr"], ref["nr"])
    assert M.checked(M.errors(host, ref)).all()


def planted(c, n=4):
    """the failure paths on the first n instances of a chain case: instance 1 a non-PD P- at node 12 (out of Q, its R terms stay)
    and a zero pivot at node 5, instance 2 a NaN record at node 7, instance 3 a GPS row never used and an infinite x^s at node
    15 -> (args, want status)"""
    a = {k: c[k][..., :n].copy() for k in M.ARGS}
    a["Ppred"][12][:, :, 1] *= -1.0
    a["Ppred"][5][2, 2, 1] = 0.0
    a["Ps"][7][3, 4, 2] = np.nan
    a["Xs"][15][8, 3] = np.inf
    a["used"][:, 3] &= ~1
    want = np.zeros((c["Xpred"].shape[0], n), np.int32)
    want[12, 1], want[5, 1], want[7, 2], want[15, 3] = M.NOT_PD, M.NOT_PD, M.NONFINITE, M.NONFINITE
    return a, want


def test_status_paths_host():
    c = M.chain_case("poly")
    T_ = c["Xpred"].shape[0]
    a, want = planted(c)
    args = [a[k] for k in M.ARGS]
    ref, host = M.noise_stats(*args, eps=c["eps"]), M.host_noise_stats(*args, eps=c["eps"])
    assert np.array_equal(ref["status"], want) and np.array_equal(host["status"], want)
    assert np.array_equal(host["nq"], ref["nq"]) and np.array_equal(host["nr"], ref["nr"])
    assert list(host["nq"]) == [T_, T_ - 2, T_ - 1, T_ - 1]
    assert (host["nr"][6:, 1] == T_).all() and (host["nr"][6:, 2] == T_ - 1).all()       # non-PD: the R terms stay; NaN: they go
    assert host["nr"][0, 3] == 0 and host["R32"][0, 3] == 0 and host["Rn32"][0, 3] == np.float32(c["Rd"][0, 3])  # a row never used
    assert np.isfinite(host["Q32"]).all() and np.isfinite(host["R32"]).all()
    clean = M.host_noise_stats(*[c[k][..., :4] for k in M.ARGS], eps=c["eps"])
    for k in ("Q32", "R32", "Qn32", "Rn32", "nq", "nr", "status"):
        assert np.array_equal(host[k][..., 0], clean[k][..., 0]), k  # the untouched instance
    assert M.checked(M.errors(host, ref)).all()


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "difference_term_dropped": ("fmaf(yj, yj, -wjj)", "(yj * yj)"),
    "Ps_factored_for_Ppred": ("const float ch = L.cur.pm[j];", "const float ch = L.cur.ps[j];"),
    "Q_for_Q_squared": ("const float q2 = L.q * L.q;", "const float q2 = L.q;"),
    "H_at_the_prediction": ("ekf_measure<true>(io.eps, io.mag, xs, m);",
                            "ekf_measure<true>(io.eps, io.mag, xm, m); { EkfMeas m2; ekf_measure<false>(io.eps, io.mag, xs, m2); "
                            "for (int q = 0; q < kEkfZ; ++q) m.h[q] = m2.h[q]; }"),
    "unused_rows_counted": ("r < kEkfZ && ((L.cur.used >> r) & 1) &&", "r < kEkfZ &&"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_em_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_rts.hpp"', f'#include "{CSRC}/ac_rts.hpp"'))
    with pytest.raises(AssertionError):
        check(measure("poly", path, lengths=(None,)))


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
def _bank(n=4):
    import torch

    from aircraft_amd import EKF

    ac = make_aircraft("poly")
    z = lambda *s: torch.zeros(s)  # noqa: E731
    return ac, EKF(ac, z(13, n), z(12, 12, n), torch.ones(12, n), torch.ones(15, n), E.MAG, z(8), True, False)


def _trace(n=4, T_=3, **kw):
    from aircraft_amd import EkfTrace

    z = lambda *s: np.zeros(s)  # noqa: E731
    f = dict(X=z(T_, 13, n), P=z(T_, 12, 12, n), nu=z(T_, 15, n), S=z(T_, 15, n), nis=z(T_, n), ll=z(n), used=z(T_, n), status=z(T_, n),
             Xpred=z(T_, 13, n), Ppred=z(T_, 12, 12, n), Abar=z(T_, 12, 12, n), X0=z(13, n), P0=z(12, 12, n))
    f.update(kw)
    return EkfTrace(**f)


def _smooth(n=4, T_=3, **kw):
    from aircraft_amd import EkfSmooth

    f = dict(X=np.zeros((T_, 13, n)), P=np.zeros((T_, 12, 12, n)), X0=None, P0=None, C=None, status=np.zeros((T_, n)))
    f.update(kw)
    return EkfSmooth(**f)


@pytest.mark.parametrize("tkw,skw,Z", [
    (dict(Xpred=None), {}, np.zeros((3, 15, 4))), (dict(Ppred=None), {}, np.zeros((3, 15, 4))), (dict(used=None), {}, np.zeros((3, 15, 4))),
    ({}, dict(X=None), np.zeros((3, 15, 4))), ({}, dict(P=None), np.zeros((3, 15, 4))), ({}, {}, np.zeros((2, 15, 4))),
    ({}, {}, np.zeros((3, 14, 4))), (dict(Ppred=np.zeros((3, 12, 4))), {}, np.zeros((3, 15, 4))),
    ({}, dict(X=np.zeros((2, 13, 4))), np.zeros((3, 15, 4))), ({}, dict(P=np.zeros((3, 12, 12, 5))), np.zeros((3, 15, 4))),
    (dict(used=np.zeros((3, 5))), {}, np.zeros((3, 15, 4))), (dict(Xpred=np.zeros((13, 4))), {}, np.zeros((3, 15, 4))),
])
def test_noise_stats_argument_checks(tkw, skw, Z):
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.noise_stats(_trace(**tkw), _smooth(**skw), Z)
    assert not ac._handle  # nothing reached the library


def test_noise_stats_wants_the_trace_and_the_smoothed_run():
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.noise_stats(_smooth(), _smooth(), np.zeros((3, 15, 4)))
    with pytest.raises(ValueError):
        bank.noise_stats(_trace(), _trace(), np.zeros((3, 15, 4)))
    assert not ac._handle


@pytest.mark.parametrize("kw", [dict(q=-np.ones(12)), dict(r=np.zeros(15)), dict(r=-np.ones((15, 4))), dict(q=np.ones(11)), dict(r=np.ones((15, 3))),
                                dict(q=np.full(12, np.nan)), dict(r=np.full(15, np.inf))])
def test_set_noise_argument_checks(kw):
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.set_noise(**kw)
    assert not ac._handle


@pytest.mark.parametrize("kw", [dict(iters=0), dict(iters=1.5), dict(iters=True), dict(update=("q", "x")), dict(update="qr"), dict(floor=-1.0),
                                dict(floor=float("nan")), dict(floor=float("inf"))])
def test_fit_noise_argument_checks(kw):
    ac, bank = _bank()
    with pytest.raises(ValueError):
        bank.fit_noise(np.zeros((3, 7, 4)), 0.01, np.zeros((3, 15, 4)), **kw)
    assert not ac._handle


def test_result_fields():
    from aircraft_amd import EkfNoiseFit, EkfNoiseStats

    assert [f for f in EkfNoiseStats.__dataclass_fields__] == ["Qsum", "Rsum", "nq", "nr", "q", "r", "status"]
    assert [f for f in EkfNoiseFit.__dataclass_fields__] == ["q", "r", "ll", "nq", "nr", "status"]


# ---- resources -------------------------------------------------------------------------------------------------------------------------
def test_em_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "em_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("em_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "em.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert scratch_bytes(r.stderr, "k_ekf_em_nodes") == 0 and scratch_bytes(r.stderr, "k_ekf_em_reduce") == 0
    b = [b for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:] if "k_ekf_em_nodes" in b.split("\n")[0]]
    assert len(b) == 1
    # 48 KiB of LDS and 256 registers: two workgroups per CU, two waves per SIMD
    assert int(re.search(r" VGPRs: (\d+)", b[0]).group(1)) <= 256 and int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b[0]).group(1)) <= 48 * 1024
    assert int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b[0]).group(1)) >= 2
