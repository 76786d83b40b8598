"""The eigenvalue chain and the flight-mode unit (aircraft_amd/csrc/ac_eig.hpp) compiled for the host with g++
(tests/host_modes/modes_host.cpp, -DAC_HOST_CHECK -ffp-contract=off): e32, the build's float32 outputs against float64 eigvals of the
same float32 matrix as a matching distance (tests/modes_ref.py), per case set; the canonical order and the conjugate pairs,
bitwise; the textbook cases; mutated copies of the header that these checks must catch; the argument checks of
Aircraft.modes / Aircraft.eig that run before any device is touched; scratch and LDS of the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import lqr_ref as L
from tests import modes_ref as M
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_modes")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_eig.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_eig.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "modes_host.cpp")
    so = os.path.join(HERE, "libmodes_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, "ac_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_EIG_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_eig.argtypes = [FP, C.c_int, C.c_int, C.c_long, FP, FP, IP, IP]
    lib.host_modes_eig.argtypes = [FP, FP, FP, C.c_uint, C.c_int, C.c_int, C.c_float, C.c_long, FP, FP, FP, FP, IP, IP]
    lib.host_eig_lds_bytes.argtypes = [C.c_int]
    for f in (lib.host_eig, lib.host_modes_eig, lib.host_eig_lds_bytes):
        f.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
SETS = {"C1": M.c1, "C2": M.c2, "C3": M.c3}


def numpy_f32_err(Mx, ref):
    """numpy eigvals on the float32 array against the float64 eigenvalues, as err_eig"""
    a32 = np.asarray(Mx, dtype=np.float32)
    got = np.stack([np.linalg.eigvals(a32[:, :, i]).astype(np.complex128) for i in range(a32.shape[2])], axis=-1)
    return M.err_eig(got, ref)


def sgeev_err(Mx, ref):
    """LAPACK's float32 driver (scipy.linalg.eigvals keeps float32: sgeev) against the float64 eigenvalues, as err_eig"""
    import scipy.linalg

    a32 = np.asarray(Mx, dtype=np.float32)
    got = np.stack([scipy.linalg.eigvals(a32[:, :, i]).astype(np.complex128) for i in range(a32.shape[2])], axis=-1)
    return M.err_eig(got, ref)


def measure(which, header=None, yardsticks=True):
    """e32 per label of a case set: {label: dict(e, status, iters, wr, wi, numpy, sgeev[, s])}"""
    out = {}
    for label, (Mx, dt) in SETS[which]().items():
        ref = M.eigvals(Mx)
        lam, st, it, (wr, wi) = M.host_eig(Mx, header=header)
        d = dict(e=M.err_eig(lam, ref), status=st, iters=it, wr=wr, wi=wi)
        if yardsticks:
            d["numpy"], d["sgeev"] = numpy_f32_err(Mx, ref), sgeev_err(Mx, ref)
        if which == "C1":
            _, s32, st2, _, raw = M.host_modes(M.embed_flight(Mx), dt=dt, header=header)
            d["s"] = M.err_s(s32, M.s_of(ref, dt), dt)
            d["modes_status"], d["raw"] = st2, raw
        out[label] = d
    return out


_MEASURED = {}


def measured(which):
    if which not in _MEASURED:
        _MEASURED[which] = measure(which)
    return _MEASURED[which]


def worst(m, key="e"):
    return max(float(d[key].max()) for d in m.values())


def check(which, m):
    """the assertions a measurement has to meet (the mutated headers must fail at least one)"""
    for label, d in m.items():
        assert (d["status"] == 0).all(), (label, d["status"])
        assert (d["e"] <= 2 * M.E32_WORST[which]).all(), (which, label, float(d["e"].max()), M.E32_WORST[which])
        M.check_order(d["wr"], d["wi"])
        if "s" in d:
            assert (d["modes_status"] == 0).all()
            assert (d["s"] <= 2 * M.E32_WORST["s"]).all(), ("s", label, float(d["s"].max()), M.E32_WORST["s"])
            es, eo = M.sigma_form_err(d["raw"], 8, float(label.split("@")[1]))
            assert (es <= 1).all() and (eo <= 1).all(), ("sigma, omega against the routine's own eigenvalues", label, es.max(), eo.max())


@pytest.mark.parametrize("which", sorted(SETS))
def test_e32_within_recorded_worst(which):
    """Every instance of the case set is inside 2 x the recorded worst (modes_ref.E32_WORST), every instance
    converges, and the outputs stand in the canonical order with bitwise conjugate pairs."""
    m = measured(which)
    for label, d in m.items():
        print(f"[modes e32] {which} {label}: host {d['e'].max():.2e} (median {np.median(d['e']):.2e}), numpy {d['numpy'].max():.2e}, "
              f"sgeev {d['sgeev'].max():.2e}, QR iterations per eigenvalue mean {d['iters'].mean() / d['wr'].shape[0]:.2f} "
              f"max per instance {d['iters'].max()}" + (f", s {d['s'].max():.2e}" if "s" in d else ""))
    check(which, m)
    assert M.E32_WORST[which] <= 3 * worst(m), ("the recorded worst is slack", which, worst(m))


@pytest.mark.parametrize("which", sorted(SETS))
def test_recorded_worst_against_numpy_float32(which):
    """The recorded worst of the case set may not exceed 4 x the error of numpy eigvals on the float32 array, measured here on
    the same case set, with a floor of 2e-7.  numpy.linalg.eigvals promotes a float32 array to float64, runs dgeev and rounds
    the result, so this yardstick is the rounding of a float64 answer (3.0e-8 .. 5.9e-8): it is what made the routine's
    arithmetic float64 (a float32 chain, LAPACK's sgeev included, lands at 1e-6 .. 8e-5 on these sets)."""
    m = measured(which)
    bar = max(4 * worst(m, "numpy"), 2e-7)
    print(f"[modes e32] {which}: recorded worst {M.E32_WORST[which]:.2e}, numpy on the float32 array {worst(m, 'numpy'):.2e}, bar {bar:.2e}")
    assert M.E32_WORST[which] <= bar, (which, M.E32_WORST[which], bar)


@pytest.mark.parametrize("which", sorted(SETS))
def test_recorded_worst_against_lapack_float32(which):
    """The same bar against LAPACK's float32 driver sgeev (scipy.linalg.eigvals keeps the dtype): what a float32 chain
    reaches on these sets, for the record in DESIGN.md §4.16."""
    m = measured(which)
    bar = max(4 * worst(m, "sgeev"), 2e-7)
    print(f"[modes e32] {which}: recorded worst {M.E32_WORST[which]:.2e}, sgeev {worst(m, 'sgeev'):.2e}, bar {bar:.2e}")
    assert M.E32_WORST[which] <= bar, (which, M.E32_WORST[which], bar)


@pytest.mark.parametrize("m", range(1, 14))
def test_shapes_host(m):
    """C5: seeded Gaussian matrices of every order, every batch size of lqr_ref.SIZES"""
    for n in L.SIZES:
        Mx = M.c5(m, n)
        lam, st, it, (wr, wi) = M.host_eig(Mx)
        e = M.err_eig(lam, M.eigvals(Mx))
        assert (st == 0).all() and (e <= 2 * M.E32_WORST["C5"]).all(), (m, n, st, e.max())
        M.check_order(wr, wi)
        if n == 257:
            print(f"[modes e32] C5 m={m}: {e.max():.2e}, QR iterations per eigenvalue {it.mean() / m:.2f}")


# ---- C4: textbook cases ----------------------------------------------------------------------------------------------------------
def host_solver(header=None):
    return lambda Mx, max_iters: M.host_eig(Mx, max_iters, header)


def check_textbook(header=None):
    M.check_textbook(host_solver(header))


def check_balancing(header=None):
    M.check_balancing(host_solver(header))


def test_textbook_cases():
    check_textbook()


def test_balancing_undoes_a_bad_scaling():
    check_balancing()


def test_status_codes_host():
    S = M.c1()["poly@0.01"][0][:, :, :4].copy()
    clean = M.host_eig(S)
    bad = S.copy()
    bad[2, 5, 1] = np.nan
    bad[7, 0, 3] = np.inf
    lam, st, it, _ = M.host_eig(bad)
    assert list(st) == [0, 3, 0, 3] and list(it[[1, 3]]) == [0, 0]
    assert np.isnan(lam[:, [1, 3]]).all() and np.array_equal(lam[:, [0, 2]], clean[0][:, [0, 2]])
    lam, st, it, _ = M.host_eig(S, max_iters=1)
    assert (st == 1).all() and np.isnan(lam).all()
    # the modes unit: NaN instances give NaN in the m rows, rows >= m stay 0
    lam, s, st, it, raw = M.host_modes(M.embed_flight(bad))
    assert list(st) == [0, 3, 0, 3] and np.isnan(raw[:, :8, 1]).all() and (raw[:, 8:] == 0).all()


def test_modes_unit_matches_reference():
    """k_modes_eig's unit in closed loop and with every coordinate selection: the structural zeros, A - B K and the selection
    agree with the float64 reference on the float32-rounded operands"""
    A, B = (M.f32x(a) for a in M.projection("poly"))
    noisy = A.copy()
    noisy[np.ix_(M.FLIGHT, L.IGNORABLE)] += 1e-6  # what the float32 projection leaves there
    for sel in ("8", "11", "12"):
        K, ok = M.closed_gains("poly", sel)
        K = M.f32x(K[..., ok])
        lam64, s64 = M.reference(A[..., ok], B[..., ok], K, M.COORDS[sel])
        lam, s, st, it, raw = M.host_modes(noisy[..., ok], B[..., ok], K, M.COORDS[sel])
        e, es = M.err_eig(lam, lam64), M.err_s(s, s64, M.DT)
        print(f"[modes e32] unit, closed loop {sel}: eig {e.max():.2e}, s dt {es.max():.2e}, rho {np.abs(lam).max():.6f}")
        assert (st == 0).all() and (e <= 2 * M.E32_WORST["C2"]).all()
        # s dt = log(lambda): the eigenvalue's error over |lambda|, plus what the float32 sigma and omega formulas lose on the
        # rounded eigenvalue (modes_ref.sigma_form_err: t <= 1 inside the unit circle, |omega dt| <= pi)
        lmin = np.abs(lam64).min()
        assert (es <= 2 * M.E32_WORST["C2"] / lmin + M.U32 * (1.5 / lmin ** 2 + 5 * abs(np.log(lmin)) + 5 * np.pi)).all()
        assert (np.abs(lam) < 1).all() and (raw[:, len(M.COORDS[sel]):] == 0).all()
        M.check_order(raw[0, :len(M.COORDS[sel])], raw[1, :len(M.COORDS[sel])])
        assert np.array_equal(np.abs(lam).max(axis=0) < 1, L.rho(A[..., ok], B[..., ok], K, L.SELECTIONS[sel]) < 1)


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "no_exceptional_shifts": [("if (its == 10 || its == 20) {", "if (false) {")],
    "no_permutation": [("again && l > 0;", "false;"), ("again && k < l;", "false;")],
    "no_scaling": [("bool noconv = true;", "bool noconv = false;")],
    "loose_deflation": [("constexpr double kEigEps = 2.220446049250313e-16;", "constexpr double kEigEps = 1e-3;")],
    "sigma_from_log_hypot": [("sigma = 0.5f * log1pf(d) / dt;", "sigma = logf(hypotf(wr, wi)) / dt;")],
}


def mutated(which, tmp_path):
    text = open(HEADER).read()
    for old, new in MUTATIONS[which]:
        assert text.count(old) == 1, (which, old)
        text = text.replace(old, new)
    text = text.replace('#include "ac_math.hpp"', f'#include "{os.path.join(CSRC, "ac_math.hpp")}"')
    text = text.replace('#include "../../include/aircraft_hip.h"',
                        f'#include "{os.path.abspath(os.path.join(CSRC, "..", "..", "include", "aircraft_hip.h"))}"')
    path = str(tmp_path / f"ac_eig_{which}.hpp")
    with open(path, "w") as f:
        f.write(text)
    return path


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    path = mutated(which, tmp_path)
    with pytest.raises(AssertionError):
        if which == "no_exceptional_shifts":
            check_textbook(path)
        elif which == "no_permutation":
            # (the shuffled triangular matrix then needs QR iterations: iters is no longer 0)
            check_textbook(path)
        elif which == "no_scaling":
            check_balancing(path)
        else:
            check("C1", measure("C1", path, yardsticks=False))


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
def _xu(n=4):
    x = np.zeros((13, n))
    x[3], x[9] = 30.0, 1.0
    return x, np.zeros((7, n))


@pytest.mark.parametrize("kw", [
    dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")), dict(dt=float("inf")), dict(max_iters=0), dict(max_iters=2.5),
    dict(coords="body"), dict(coords=(3, 4, 5)), dict(coords=tuple(range(3, 13))), dict(coords=(3, 3, 4, 5, 6, 7, 9, 10, 11)),
    dict(coords=(3, 4, 5, 6, 7, 9, 10, 11.5)), dict(gains=np.zeros((7, 12, 3))), dict(gains=np.zeros((12, 7, 4))),
    dict(ws=np.zeros(10, np.float32)),
])
def test_modes_argument_checks(kw):
    ac = make_aircraft("poly")
    args = dict(dt=0.01)
    args.update(kw)
    with pytest.raises(ValueError):
        ac.modes(_xu(), **args)
    assert not ac._handle  # nothing reached the library


@pytest.mark.parametrize("xu", [(np.zeros((13, 4)), np.zeros((7, 3))), (np.zeros((12, 4)), np.zeros((7, 4))), np.zeros((13, 4)), None])
def test_modes_nominal_checks(xu):
    ac = make_aircraft("poly")
    with pytest.raises(ValueError):
        ac.modes(xu, 0.01)
    assert not ac._handle


def test_modes_refuses_gains_of_another_dt():
    from aircraft_amd import LqrResult

    ac = make_aircraft("poly")
    res = LqrResult(np.zeros((7, 12, 4)), None, None, None, None, None, None, None, None, None, 0.02, None, None, ac)
    with pytest.raises(ValueError):
        ac.modes(_xu(), 0.01, gains=res)
    assert not ac._handle


@pytest.mark.parametrize("shape", [(14, 14, 2), (3, 4, 2), (0, 0, 2), (5,), (2, 2, 2, 2)])
def test_eig_argument_checks(shape):
    ac = make_aircraft("poly")
    with pytest.raises(ValueError):
        ac.eig(np.zeros(shape))
    assert not ac._handle


# ---- resources -------------------------------------------------------------------------------------------------------------------------
def test_modes_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "modes_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("modes_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "modes.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("k_modes_eig", "k_eig"):
        assert scratch_bytes(r.stderr, k) == 0, k
    # the matrix lives in dynamically sized LDS: (m^2 + 2 m) float64 words per instance; a full wave of instances per
    # workgroup while that fits 64 KiB (m <= 10), half a wave beyond
    lds = lib_host().host_eig_lds_bytes
    assert lds(8) == 80 * 64 * 8 and lds(10) == 120 * 64 * 8 and lds(11) == 143 * 32 * 8 and lds(13) == 195 * 32 * 8
    assert all(lds(m) <= 64 * 1024 for m in range(1, 14))
