"""The LQR's per-lane code (aircraft_amd/csrc/ac_lqr.hpp) compiled for the host with g++ (tests/host_lqr/lqr_host.cpp,
-DAC_HOST_CHECK -ffp-contract=off): e32, the float32 build against float64 (tests/lqr_ref.py) on identical float32-rounded
inputs, per instance, for the projection, P, K and the expanded gains; mutated copies of the header that these checks must
catch; the argument checks of Aircraft.lqr that run before any device is touched; the register and scratch budget of the
four kernels from the compiled code object."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import lqr_ref as L
from tests.helpers import make_aircraft
from tests.test_headline_resources import scratch_bytes

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_lqr")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_lqr.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_lqr.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "lqr_host.cpp")
    so = os.path.join(HERE, "liblqr_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key] + [os.path.join(CSRC, f) for f in ("ac_math.hpp", "ac_group.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_LQR_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_lqr_project.argtypes = [FP, FP, FP, FP, C.c_long, FP, FP]
    lib.host_lqr_dare.argtypes = [C.c_void_p, FP, FP, C.c_int, C.c_long, FP, FP, FP, IP, IP]
    lib.host_lqr_gains.argtypes = [FP, FP, C.c_long, C.c_long, FP]
    lib.host_steady_error.argtypes = [FP, FP, C.c_long, FP]
    lib.host_lqr_gj.argtypes = [FP, FP, FP, IP]
    for f in (lib.host_lqr_project, lib.host_lqr_dare, lib.host_lqr_gains, lib.host_steady_error, lib.host_lqr_gj):
        f.restype = C.c_int
    _LIBS[key] = lib
    return lib


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
H_GAINS = 8
MODELS = ("poly", "default")


def measure(name, header=None):
    """e32 of every quantity on the grid of `name`: dict of (n,) arrays keyed proj, P:<sel>, K:<sel>, res:<sel>, gains, xi"""
    ac, orc, x, u = L.grid(name)
    xp, A, B, _ = (L.f32x(a) for a in orc.step_sens(x, u, L.DT))
    A64, B64 = L.project(x, xp, A, B)
    A32, B32 = L.host_project(x, xp, A, B, header)
    out = {"proj": np.maximum(L.unit_max_abs(A32, A64), L.unit_max_abs(B32, B64))}
    Ax, Bx = L.f32x(A64), L.f32x(B64)
    K8 = None
    for sel, q in L.SELECTIONS.items():
        P64, K64, res64, st64, _ = L.solve(Ax, Bx, q)
        P32, K32, res32, st32, it32 = L.host_dare(Ax, Bx, q, header=header)
        assert (st64 == 0).all()
        out["status:" + sel] = st32
        out["iters:" + sel] = it32
        out["P:" + sel] = L.unit_max_rel(P32, P64)
        out["K:" + sel] = L.unit_max_abs(K32, K64) / np.abs(K64).reshape(-1, K64.shape[-1]).max(axis=0)
        out["res:" + sel] = res32
        np32 = [L.sda32(Ax[:, :, i], Bx[:, :, i], q, L.R1)[1] for i in range(Ax.shape[2])]
        out["Knp:" + sel] = L.unit_max_abs(np.stack(np32, axis=-1), K64) / np.abs(K64).reshape(-1, K64.shape[-1]).max(axis=0)
        out["cost:" + sel] = L.excess_cost(Ax, Bx, K32, P64, q, L.R1)
        if sel == "11":
            K8 = L.f32x(K64)
    Xnom = L.f32x(orc.rollout(x, np.repeat(u[None], H_GAINS, axis=0), L.DT))
    g64 = L.expand(Xnom, K8)
    g32 = L.host_gains(Xnom, K8, header)
    out["gains"] = np.max([L.unit_max_rel(g32[k], g64[k]) for k in range(H_GAINS)], axis=0)
    rng = np.random.default_rng(7)
    xi0 = rng.uniform(-1, 1, (12, x.shape[1])) * np.array([5, 5, 5, 1, 1, 1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])[:, None]
    xs = L.f32x(L.unchart(xi0, x))
    xi64 = L.chart(xs, x)
    out["xi"] = L.unit_max_abs(L.host_error(xs, x, header), xi64) / np.maximum(np.abs(xi64).max(axis=0), 1.0)
    out["xi0"] = np.abs(L.host_error(x, x, header)).max(axis=0)
    return out


_MEASURED = {}


def measured(name):
    if name not in _MEASURED:
        _MEASURED[name] = measure(name)
    return _MEASURED[name]


def worst(m, key):
    return max(float(v.max()) for k, v in m.items() if k == key or k.startswith(key + ":"))


def check(m):
    """the assertions a measurement has to meet (the mutated headers must fail at least one)"""
    for sel in L.SELECTIONS:
        assert (m["status:" + sel] == 0).all(), (sel, m["status:" + sel])
        assert m["iters:" + sel].max() <= 16, (sel, m["iters:" + sel].max())
    for key in ("proj", "P", "K", "gains", "xi"):
        assert worst(m, key) <= L.E32_WORST[key], (key, worst(m, key), L.E32_WORST[key])
    assert worst(m, "xi0") == 0.0


@pytest.mark.parametrize("name", MODELS)
def test_e32_within_recorded_worst(name):
    """The recorded worst values (lqr_ref.E32_WORST) hold, every instance converges within 16 doubling
    steps, and the closed-loop cost of the float32 gain is within 1e-6 of the optimum."""
    m = measured(name)
    print(f"[lqr e32] {name}: " + ", ".join(f"{k} {worst(m, k):.2e}" for k in ("proj", "P", "K", "Knp", "res", "cost", "gains", "xi")),
          {sel: (int(m['iters:' + sel].min()), int(m['iters:' + sel].max())) for sel in L.SELECTIONS})
    check(m)
    assert worst(m, "res") <= 1e-4 and worst(m, "cost") <= 1e-6


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst (over both models), not a loose bound: each entry is within 3 x of what is measured."""
    for key in ("proj", "P", "K", "gains"):
        w = max(worst(measured(n), key) for n in MODELS)
        assert L.E32_WORST[key] <= 3 * w, (key, w, L.E32_WORST[key])


def test_K_e32_lands_where_numpy_float32_does():
    """The same iteration in NumPy/LAPACK float32 (lqr_ref.sda32) on identical inputs is the yardstick for the elimination
    and the symmetrisation: per model and selection the header's worst max|dK| / max|K| stays within 2 x NumPy's worst."""
    for name in MODELS:
        m = measured(name)
        for sel in L.SELECTIONS:
            mine, theirs = float(m["K:" + sel].max()), float(m["Knp:" + sel].max())
            print(f"[lqr e32] {name} selection {sel}: K header {mine:.2e}, NumPy float32 {theirs:.2e}")
            assert mine <= 2 * theirs, (name, sel, mine, theirs)


# ---- the group elimination on a system that needs pivoting ------------------------------------------------------------------------
def pivot_case():
    rng = np.random.default_rng(3)
    W = np.eye(12) + 0.3 * rng.standard_normal((12, 12))
    W[0, 0] = 0.0          # no elimination without a row exchange
    W[5, 5] = 1e-7         # and a tiny diagonal entry further down
    return L.f32x(W), L.f32x(rng.standard_normal((12, 24)))


def check_pivot(header=None):
    W, rhs = pivot_case()
    X, bad = L.host_gj(W, rhs, header)
    want = np.linalg.solve(W, rhs)
    assert not bad
    assert np.abs(X - want).max() <= 1e-4 * np.abs(want).max(), np.abs(X - want).max() / np.abs(want).max()


def test_elimination_pivots():
    check_pivot()


def test_elimination_reports_singular():
    W, rhs = pivot_case()
    W[:, 3] = 0.0
    _, bad = L.host_gj(W, rhs)
    assert bad


def test_status_codes_host():
    ac, orc, x, u = L.grid("poly")
    A, B = (L.f32x(a) for a in L.oracle_projection(orc, x[:, :4], u[:, :4]))
    A[3, 4, 1] = np.nan
    P, K, res, st, it = L.host_dare(A, B, L.Q8, iters=3)
    assert list(st) == [1, 3, 1, 1] and np.isnan(P[:, :, 1]).all() and np.isnan(K[:, :, 1]).all() and np.isnan(res[1])
    assert np.isfinite(P[:, :, [0, 2, 3]]).all() and list(it) == [3, 0, 3, 3]
    # frozen instances: bit-identical between iters and iters + 4; dropped coordinates and thrust rows exactly 0
    a = L.host_dare(A, B, L.Q8, iters=20)
    b = L.host_dare(A, B, L.Q8, iters=24)
    ok = a[3] == 0
    assert ok[[0, 2, 3]].all()
    for p, q in zip(a, b):
        assert np.array_equal(p[..., ok], q[..., ok])
    d = L.dropped(L.Q8)
    assert (a[0][d][..., ok] == 0).all() and (a[0][:, d][..., ok] == 0).all() and (a[1][:, d][..., ok] == 0).all()
    assert (a[1][3:6][..., ok] == 0).all()


# ---- mutated headers must fail ------------------------------------------------------------------------------------------------------
MUTATIONS = {
    "no_pivoting": ("const int p = lqr_pivot_lane(s.c, best);", "int p = lqr_pivot_lane(s.c, best); p = k;"),
    "transposed_A_in_H_update": ("const double akr = s.m[3][k][rc];  // A_k[k][r]", "const double akr = s.m[3][rc][k];  // A_k[r][k]"),
    "missing_Zt_in_attitude_rows": ("E[6 + i][6 + j] = fmaf(f.Z[0][i], N2[0][j], fmaf(f.Z[1][i], N2[1][j], f.Z[2][i] * N2[2][j]));",
                                    "E[6 + i][6 + j] = N2[i][j];"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_lqr_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    with pytest.raises(AssertionError):
        if which == "no_pivoting":
            check_pivot(path)
        else:
            check(measure("poly", path))


# ---- Python argument checks (before any device call) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(dt=0.0), dict(dt=-0.01), dict(dt=float("nan")), dict(iters=0), dict(iters=2.5), dict(tol=-1.0), dict(tol=float("nan")),
    dict(q=np.ones(11)), dict(q=-np.ones(12)), dict(q=np.full(12, np.nan)), dict(r=np.zeros(7)), dict(r=np.ones(6)),
    dict(ws=np.zeros(10, np.float32)),
])
def test_lqr_argument_checks(kw):
    ac = make_aircraft("poly")
    x = np.zeros((13, 4))
    x[3], x[9] = 30.0, 1.0
    args = dict(dt=0.01)
    args.update(kw)
    with pytest.raises(ValueError):
        ac.lqr((x, np.zeros((7, 4))), **args)
    assert not ac._handle  # nothing reached the library


@pytest.mark.parametrize("xu", [(np.zeros((13, 4)), np.zeros((7, 3))), (np.zeros((12, 4)), np.zeros((7, 4))), np.zeros((13, 4)), None])
def test_lqr_nominal_checks(xu):
    ac = make_aircraft("poly")
    with pytest.raises(ValueError):
        ac.lqr(xu, 0.01)
    assert not ac._handle


# ---- resources -------------------------------------------------------------------------------------------------------------------------
def test_lqr_kernels_use_no_scratch(tmp_path):
    from aircraft_amd import build as B

    src = os.path.join(B.CSRC, "lqr_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("lqr_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "lqr.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for k in ("k_lqr_project", "k_lqr_dare", "k_lqr_gains", "k_steady_error"):
        assert scratch_bytes(r.stderr, k) == 0, k
    # the Riccati kernel: the documented budget
    blk = r.stderr[r.stderr.index("k_lqr_dare"):]
    vgprs = int(re.search(r" VGPRs: (\d+)", blk).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", blk).group(1))
    assert vgprs <= 256 and lds <= 16 * 1024, (vgprs, lds)
