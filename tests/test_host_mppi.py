"""The MPPI per-unit code (aircraft_amd/csrc/ac_mppi.hpp) compiled for the host with g++ (tests/host_mppi/mppi_host.cpp,
-DAC_HOST_CHECK) against the NumPy restatement (tests/mppi_ref.py): Philox words, normals, the sampler, the weights.  Also the
statistics and the shard invariance of the noise definition itself, the argument checks of `MPPI` that run before any device is
touched, and the scratch use of the three new kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import mppi_ref as R
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_mppi")
SO = os.path.join(HERE, "libmppi_host.so")
CSRC = os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc")
FP, UP, IP = C.POINTER(C.c_float), C.POINTER(C.c_uint), C.POINTER(C.c_int)
NORMAL_UNIT = 2.0 ** -24  # the normals' bound is 32 of these times max(1, r)


def _lib_host():
    src = os.path.join(HERE, "mppi_host.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_mppi.hpp")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", SO, src],
                       check=True)
    L = C.CDLL(SO)
    L.host_philox.argtypes = [C.c_long, UP, UP, UP]
    L.host_box_muller.argtypes = [C.c_long, UP, UP, FP, FP]
    L.host_mppi_sample.argtypes = [C.POINTER(_lib.MppiOpts), C.c_uint, FP, C.c_int, C.c_long, C.c_long, FP]
    L.host_mppi_weight.argtypes = [C.c_long, FP, C.c_float, C.c_float, FP, IP]
    L.host_mppi_better.argtypes = [C.c_float, C.c_int, C.c_float, C.c_int]
    return L


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def make_opts(sigma, u_min, u_max, lam=1.0, seed=0, instance_offset=0, keep_nominal=True):
    o = _lib.MppiOpts()
    o.sigma[:], o.u_min[:], o.u_max[:] = [float(v) for v in sigma], [float(v) for v in u_min], [float(v) for v in u_max]
    o.lambda_, o.seed, o.instance_offset, o.keep_nominal = float(lam), int(seed), int(instance_offset), int(keep_nominal)
    return o


def sample_tolerance(ref, rad, sigma):
    """|Uc - ref| allowed: the normals' bound times sigma[r], plus one fp32 ulp of the result."""
    sg = np.asarray(sigma, dtype=np.float64)[None, :, None]
    return 32 * NORMAL_UNIT * np.maximum(1.0, rad) * sg + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


# ---- 1. the reference itself ------------------------------------------------------------------------------------------------------
def test_reference_known_answers():
    for ctr, key, out in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(*ctr, *key)
        assert tuple(int(g) for g in got) == out


# ---- 2. the per-unit code -----------------------------------------------------------------------------------------------------------
def test_host_philox_bit_equal():
    L = _lib_host()
    rng = np.random.default_rng(11)
    edge = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    n = 4096
    c = rng.integers(0, 2 ** 32, size=(4, n), dtype=np.uint64).astype(np.uint32)
    k = rng.integers(0, 2 ** 32, size=(2, n), dtype=np.uint64).astype(np.uint32)
    # a grid of small counters (the ones the sampler forms) and the edge words
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(3), np.arange(6), indexing="ij")).reshape(4, -1).astype(np.uint32)
    c = np.concatenate([c, g, np.tile(edge, (4, 1)), np.stack([np.roll(edge, i) for i in range(4)])], axis=1)
    k = np.concatenate([k, np.tile(np.array([[7], [256]], dtype=np.uint32), (1, g.shape[1])), np.tile(edge, (2, 1)),
                        np.stack([np.roll(edge, 2), np.roll(edge, 5)])], axis=1)
    for ctr, key, _ in R.KNOWN_ANSWERS:
        c = np.concatenate([c, np.array(ctr, dtype=np.uint32)[:, None]], axis=1)
        k = np.concatenate([k, np.array(key, dtype=np.uint32)[:, None]], axis=1)
    c, k = u32(c), u32(k)
    n = c.shape[1]
    out = np.zeros((4, n), np.uint32)
    assert L.host_philox(n, c.ctypes.data_as(UP), k.ctypes.data_as(UP), out.ctypes.data_as(UP)) == 0
    ref = np.stack(R.philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]))
    assert np.array_equal(out, ref)
    assert tuple(int(v) for v in out[:, -1]) == R.KNOWN_ANSWERS[-1][2]


def test_host_normals_within_bound():
    L = _lib_host()
    rng = np.random.default_rng(12)
    n = 1 << 20
    xa = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    xb = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0, 255, 256, 0xFFFFFF00, 0xFFFFFFFF, 0x80000000, 0x40000000, 0xC0000000, 0x3FFFFF00, 0x7FFFFF00], dtype=np.uint32)
    ea, eb = np.meshgrid(edge, edge, indexing="ij")
    xa, xb = u32(np.concatenate([xa, ea.ravel()])), u32(np.concatenate([xb, eb.ravel()]))
    n = xa.size
    na, nb = np.zeros(n, np.float32), np.zeros(n, np.float32)
    assert L.host_box_muller(n, xa.ctypes.data_as(UP), xb.ctypes.data_as(UP), na.ctypes.data_as(FP), nb.ctypes.data_as(FP)) == 0
    ra, rb, r = R.box_muller(xa, xb)
    units = np.maximum(np.abs(na - ra), np.abs(nb - rb)) / (NORMAL_UNIT * np.maximum(1.0, r))
    print(f"host normals: worst {units.max():.2f} units of 2^-24 max(1, r) over {n} pairs (bound 32)")
    assert units.max() <= 32.0
    assert np.abs(na).max() <= R.N_MAX * (1 + 1e-6) and np.abs(nb).max() <= R.N_MAX * (1 + 1e-6)


@pytest.mark.parametrize("case", ["all_rows", "rows_0_2", "no_keep", "offset"])
def test_host_sample_matches_reference(case):
    L = _lib_host()
    B, K, H = 5, 9, 4
    rng = np.random.default_rng(13)
    sigma = [0.7, 1.3, 0.4, 0.2, 0.05, 0.3, 0.1] if case != "rows_0_2" else [1.0, 0.5, 2.0, 0, 0, 0, 0]
    u_min, u_max = [-5, -5, -5, 0, -1, -1, 0], [5, 5, 5, 1, 1, 1, 1]
    Unom = f32(rng.uniform(-6, 6, (H, 7, B)))  # some nominals outside the box
    seed, it = (1 << 40) + 7, 3
    off = 1000 if case == "offset" else 0
    keep = case != "no_keep"
    o = make_opts(sigma, u_min, u_max, seed=seed, instance_offset=off, keep_nominal=keep)
    Uc = np.zeros((H, 7, K * B), np.float32)
    assert L.host_mppi_sample(C.byref(o), it, Unom.ctypes.data_as(FP), K, B, H, Uc.ctypes.data_as(FP)) == 0
    ref, rad = R.sample(Unom, sigma, u_min, u_max, seed, it, K, instance_offset=off, keep_nominal=keep, want_radius=True)
    assert (np.abs(Uc - ref) <= sample_tolerance(ref, rad, sigma)).all()
    lo, hi = f32(u_min)[None, :, None], f32(u_max)[None, :, None]
    assert (Uc >= lo).all() and (Uc <= hi).all()
    clipped = np.minimum(np.maximum(Unom, lo), hi)
    dead = [r for r in range(7) if sigma[r] == 0]
    assert np.array_equal(Uc.reshape(H, 7, K, B)[:, dead], np.repeat(clipped[:, dead, None, :], K, axis=2))
    if keep:
        assert np.array_equal(Uc[:, :, :B], clipped)
    else:
        assert not np.array_equal(Uc[:, :3, :B], clipped[:, :3])


def test_host_weight_matches_reference():
    L = _lib_host()
    rng = np.random.default_rng(14)
    for lam in (0.1, 1.0, 100.0, 1e-4):
        J = f32(10.0 ** rng.uniform(-1, 3, 500))
        J[::17] = np.nan
        J[5::23] = np.inf
        J[7::29] = -np.inf
        jmin = float(J[np.isfinite(J)].min())
        w, fin = np.zeros(J.size, np.float32), np.zeros(J.size, np.int32)
        assert L.host_mppi_weight(J.size, J.ctypes.data_as(FP), jmin, lam, w.ctypes.data_as(FP), fin.ctypes.data_as(IP)) == 0
        assert np.array_equal(fin.astype(bool), np.isfinite(J))
        lam32 = float(np.float32(lam))
        x = np.where(np.isfinite(J), (J.astype(np.float64) - jmin) / lam32, np.inf)
        ref = np.where(np.isfinite(J), np.exp(-x), 0.0)
        # fp32: the argument carries (|x| + 1) 2^-23 of rounding (subtraction, division), expf one more ulp; 2^-149 for the subnormals
        tol = (2 * np.where(np.isfinite(x), x, 0.0) + 2) * 2.0 ** -23 * ref + 2.0 ** -149
        assert (np.abs(w - ref) <= tol).all()
        assert w[np.argmin(np.where(np.isfinite(J), J, np.inf))] == 1.0
    assert L.host_mppi_better(1.0, 5, 2.0, 1) == 1 and L.host_mppi_better(1.0, 5, 1.0, 1) == 0
    assert L.host_mppi_better(1.0, 1, 1.0, 5) == 1 and L.host_mppi_better(np.nan, 0, 1.0, 1) == 0


# ---- 3. statistics of the definition -----------------------------------------------------------------------------------------------
def test_noise_statistics():
    seed, it, B, K, H = (1 << 40) + 7, 3, 64, 128, 19
    n = R.normals(seed, it, K, B, H)  # [H][7][K][B]
    N = n.size
    assert N == 1089536
    se = 1 / np.sqrt(N)
    figures = dict(mean=n.mean() / se, var=(n.var() - 1) / np.sqrt(2.0 / N), m4=((n ** 4).mean() - 3) / np.sqrt(96.0 / N))
    corr = lambda a, b: (a * b).mean() / (1 / np.sqrt(a.size))  # noqa: E731
    figures.update(lag_node=corr(n[1:], n[:-1]), lag_row=corr(n[:, 1:], n[:, :-1]), lag_sample=corr(n[:, :, 1:], n[:, :, :-1]),
                   lag_instance=corr(n[..., 1:], n[..., :-1]), lag_it=corr(n, R.normals(seed, it + 1, K, B, H)))
    print("noise statistics in standard errors:", {k: round(float(v), 2) for k, v in figures.items()})
    for k, v in figures.items():
        assert abs(v) <= 5.0, (k, v)
    assert np.abs(n).max() <= R.N_MAX


# ---- 4. shard invariance -------------------------------------------------------------------------------------------------------------
def test_reference_shard_invariance():
    rng = np.random.default_rng(15)
    H, K = 6, 11
    Unom = rng.uniform(-4, 4, (H, 7, 7))
    sigma, lo, hi = [1, 1, 1, 0.1, 0.1, 0.1, 0.2], [-5] * 7, [5] * 7
    whole = R.sample(Unom, sigma, lo, hi, 99, 2, K).reshape(H, 7, K, 7)
    part = R.sample(Unom[:, :, 2:5], sigma, lo, hi, 99, 2, K, instance_offset=2).reshape(H, 7, K, 3)
    assert np.array_equal(whole[..., 2:5], part)
    assert not np.array_equal(whole[..., 0:3], part)


# ---- 5. argument checks (before any device call) ---------------------------------------------------------------------------------------
def _problem(time="fixed"):
    from aircraft_amd.control import ILQR, QuadraticCost

    ac = make_aircraft("poly")
    return ac, ILQR(system=ac, dt=0.01, num_nodes=10, cost=QuadraticCost.goal((30.0, 2.0)), time=time)


@pytest.mark.parametrize("kw", [
    dict(samples=0), dict(samples=2.5), dict(samples=True), dict(temperature=0.0), dict(temperature=-1.0),
    dict(temperature=float("nan")), dict(temperature=float("inf")), dict(sigma=(1, 1, 1)), dict(sigma=(1, 1, 1, 0, 0, 0, -0.1)),
    dict(sigma=(1, 1, 1, 0, 0, 0, float("nan"))), dict(sigma=1.0), dict(seed=-1), dict(seed=2 ** 64), dict(instance_offset=-1),
    dict(instance_offset=2 ** 32),
])
def test_mppi_argument_checks(kw):
    from aircraft_amd.control import MPPI

    ac, prob = _problem()
    with pytest.raises(ValueError):
        MPPI(prob, **kw)
    assert not ac._handle  # nothing reached the library


def test_mppi_refuses_variable_time_and_bad_shapes():
    import torch

    from aircraft_amd.control import MPPI

    ac, prob = _problem(time="variable")
    with pytest.raises(ValueError):
        MPPI(prob)
    with pytest.raises(ValueError):
        MPPI(object())
    ac, prob = _problem()
    m = MPPI(prob, samples=8)
    assert m.num_nodes == 10 and m.dt == 0.01 and m.problem is prob  # delegation
    for U in (torch.zeros(9, 7, 2), torch.zeros(10, 6, 2), torch.zeros(10, 7), torch.zeros(10, 7, 2, dtype=torch.float64)):
        with pytest.raises(ValueError):
            m.sample(U)
        with pytest.raises(ValueError):
            m.update(torch.zeros(16), torch.zeros(10, 7, 16), U)
    with pytest.raises(ValueError):
        m.sample(torch.zeros(10, 7, 2), x0=torch.zeros(13, 3))
    assert not ac._handle


def test_mppi_opts_layout():
    """ac_mppi_opts as the C compiler lays it out: 22 floats, the 8-byte seed on an 8-byte boundary, two 4-byte words."""
    assert C.sizeof(_lib.MppiOpts) == 104 and _lib.MppiOpts.seed.offset == 88 and _lib.MppiOpts.keep_nominal.offset == 100
    assert set(("ac_mppi_workspace_floats", "ac_mppi_sample_f32", "ac_mppi_update_f32")) <= set(_lib.PROTOTYPES)


# ---- 6. resources ------------------------------------------------------------------------------------------------------------------------
def test_mppi_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "mppi_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("mppi_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "mppi.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("k_mppi_sample", "k_mppi_weights", "k_mppi_blend"):
        assert scratch_bytes(r.stderr, k) == 0, k
    # every instantiation, not only the first one of each template
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    mine = [b for b in blocks if re.match(r"_ZN2ac\d+k_mppi_", b)]
    assert len(mine) == 2 + 5 + 10
    for b in mine:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split("\n")[0]
