"""GPU tests of the LQR about steady-flight trims (ac_lqr_f32, ac_lqr_gains_f32, ac_steady_error_f32, Aircraft.lqr /
rollout_lqr / steady_error) against the float64 restatement tests/lqr_ref.py.

Instances: the points of trim_ref.grid() that trim in float64 (lqr_ref.grid), cycled to the batch sizes SIZES, which straddle
the 16-lane group (4 instances per wave), the wave and the workgroup.  Every output and the workspace sit between guard words.

The bars.  e32 is the host build of the same header (g++, float32) against float64 ON THE DEVICE'S OWN INPUTS, per instance.
An instance is checked when its e32 is within 2 x the recorded worst (lqr_ref.E32_WORST; the factor 2 is room for a different
summation order); at most 5 % of a batch's distinct instances may miss that (two trims of the shipped net are close to
uncontrollable in the path coordinates: float32 and NumPy alike lose three digits there).  The device is then held to
8 x the worst e32 of the checked instances of its batch: a single instance's e32 is one draw of a rounding error and can be
arbitrarily small, the batch's worst is its scale."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import lqr_ref as L
from tests.helpers import check_against_conditioning, instance_err

pytestmark = pytest.mark.gpu

GUARD = 64
F_SENTINEL, I_SENTINEL = 12345.0, 0x5A5A5A5A
STATE_TOL = 1e-5
MODELS = ("poly", "default", "linear", "real_net")
SELECTION_OF = {1: "8", 3: "8", 4: "8", 5: "8", 63: "11", 64: "8", 65: "11", 257: "12"}
CASES = [(m, n) for m in MODELS for n in L.SIZES] + [("net_4x128", 65)]


class Guarded:
    """a device array between two runs of GUARD sentinel words"""

    def __init__(self, shape, gpu, dtype=None):
        import torch

        self.dtype = dtype or torch.float32
        self.sentinel = F_SENTINEL if self.dtype == torch.float32 else I_SENTINEL
        self.n = int(np.prod(shape))
        self.full = torch.full((self.n + 2 * GUARD,), self.sentinel, device=gpu, dtype=self.dtype)
        self.t = self.full[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def check(self):
        assert bool((self.full[:GUARD] == self.sentinel).all()) and bool((self.full[GUARD + self.n:] == self.sentinel).all()), \
            "a guard word was overwritten"

    def np(self):
        a = self.t.cpu().numpy()
        return a.astype(np.float64) if a.dtype == np.float32 else a


def ws_layout(addr, n):
    """float offsets of x+ [13][n], A [13][13][n], B [13][7][n] in the workspace: each on the next 256-byte boundary"""
    off, p = [], int(addr)
    for rows in (13, 169, 91):
        p = (p + 255) & ~255
        off.append((p - addr) // 4)
        p += 4 * rows * n
    return off, (p - addr) // 4


def run(ac, gpu, x, u, q, iters=L.ITERS, tol=L.TOL, dt=L.DT):
    """one ac_lqr_f32 call in guarded buffers -> dict of float64 / int arrays, and the device tensors of the workspace parts"""
    import torch

    lib = ac._sync()
    n = x.shape[1]
    X, U = (torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=gpu) for a in (x, u))
    need = C.c_size_t()
    assert lib.ac_lqr_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(A=Guarded((12, 12, n), gpu), B=Guarded((12, 7, n), gpu), P=Guarded((12, 12, n), gpu), K=Guarded((7, 12, n), gpu),
             res=Guarded((n,), gpu), st=Guarded((n,), gpu, torch.int32), it=Guarded((n,), gpu, torch.int32),
             ws=Guarded((need.value,), gpu))
    o = L.lqr_opts(q, L.R1, tol)
    rc = lib.ac_lqr_f32(ac._handle, C.byref(o), X.data_ptr(), U.data_ptr(), C.c_float(dt), int(iters), n, g["A"].ptr(), g["B"].ptr(),
                        g["P"].ptr(), g["K"].ptr(), g["res"].ptr(), g["st"].ptr(), g["it"].ptr(), g["ws"].ptr(), need.value,
                        ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    off, end = ws_layout(g["ws"].ptr(), n)
    assert end <= need.value
    w = g["ws"].t
    parts = (w[off[0]:off[0] + 13 * n].view(13, n), w[off[1]:off[1] + 169 * n].view(13, 13, n), w[off[2]:off[2] + 91 * n].view(13, 7, n))
    out = {k: v.np() for k, v in g.items() if k != "ws"}
    out["X"], out["U"], out["ws"] = X, U, parts
    return out


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def k_rel(K, K64):
    return L.unit_max_abs(K, K64) / np.abs(K64).reshape(-1, K64.shape[-1]).max(axis=0)


# ---- 1. projection and Riccati solve --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=[f"{m}-{n}" for m, n in CASES])
def test_lqr_against_float64(gpu, name, n):
    import torch

    ac, orc, xg, ug = L.grid(name)
    m = min(n, xg.shape[1])  # distinct instances in the batch (the first m of the grid)
    # (the grid is chosen on the float64 / host pair alone: the synthetic net about trims that are not its own keeps every
    # instance with the 8 coordinates only, the shipped net leaves out 2 of 42 with 11 and 3 with all 12)
    sel = "8" if name == "net_4x128" else "11" if (name, n) == ("real_net", 257) else SELECTION_OF[n]
    q = L.SELECTIONS[sel]
    x, u = L.cycle(xg, n), L.cycle(ug, n)
    d = run(ac, gpu, x, u, q)
    # -- the workspace holds the handle's own step sensitivities, bit for bit
    Xn, A, Bm, _ = ac.step_sens(d["X"], d["U"], L.DT, want_c=False)
    for got, want in zip(d["ws"], (Xn, A, Bm)):
        assert torch.equal(got, want)
    # -- a repeated instance gives the same bits wherever it sits in the batch
    first = np.arange(n) % m
    for k in ("A", "B", "P", "K", "res"):
        assert bits_equal(d[k], d[k][..., first]), k
    assert np.array_equal(d["st"], d["st"][first]) and np.array_equal(d["it"], d["it"][first])
    u_ = slice(0, m)
    xp, A64in, B64in = (t.cpu().numpy().astype(np.float64)[..., u_] for t in d["ws"])
    # -- projection
    A64, B64 = L.project(x[:, u_], xp, A64in, B64in)
    A32, B32 = L.host_project(x[:, u_], xp, A64in, B64in)
    e32 = np.maximum(L.unit_max_abs(A32, A64), L.unit_max_abs(B32, B64))
    assert (e32 <= 2 * L.E32_WORST["proj"]).all(), ("e32 condition, projection", e32.max())
    err = np.maximum(L.unit_max_abs(d["A"][..., u_], A64), L.unit_max_abs(d["B"][..., u_], B64))
    print(f"[lqr] {name} n={n}: projection e32 {e32.max():.2e}, device {err.max():.2e}")
    assert (err <= 8 * e32.max()).all(), ("projection", err.max(), e32.max())
    assert (d["B"][:, 3:6] == 0).all(), "the thrust columns of B_xi are exactly zero"
    # -- Riccati: float64 and the host build on the device's A_xi, B_xi
    Ad, Bd = d["A"][..., u_], d["B"][..., u_]
    P64, K64, res64, st64, it64 = L.solve(Ad, Bd, q)
    P32, K32, res32, st32, it32 = L.host_dare(Ad, Bd, q)
    eP, eK = L.unit_max_rel(P32, P64), k_rel(K32, K64)
    keep = (eP <= 2 * L.E32_WORST["P"]) & (eK <= 2 * L.E32_WORST["K"]) & (st64 == 0)
    assert (~keep).sum() <= 0.05 * m, ("e32 condition: left out", int((~keep).sum()), "of", m, eP.max(), eK.max())
    Pd, Kd = d["P"][..., u_], d["K"][..., u_]
    assert (d["st"][u_][st64 == 0] == 0).all(), ("status", d["st"][u_], it64)
    assert np.isfinite(Pd).all() and np.isfinite(Kd).all()
    dP, dK = L.unit_max_rel(Pd, P64), k_rel(Kd, K64)
    print(f"[lqr] {name} n={n} selection {sel}: kept {keep.sum()}/{m}; P e32 {eP[keep].max():.2e} device {dP[keep].max():.2e}; "
          f"K e32 {eK[keep].max():.2e} device {dK[keep].max():.2e}; steps {d['it'].min()}..{d['it'].max()}")
    assert (dP[keep] <= 8 * eP[keep].max()).all(), ("P", dP[keep].max(), eP[keep].max())
    assert (dK[keep] <= 8 * eK[keep].max()).all(), ("K", dK[keep].max(), eK[keep].max())
    assert (d["res"][u_][keep] <= 8 * res32[keep].max()).all(), ("residual", d["res"][u_][keep].max(), res32[keep].max())
    # -- structure: dropped coordinates and thrust rows exactly 0
    dr = L.dropped(q)
    assert (d["P"][dr] == 0).all() and (d["P"][:, dr] == 0).all() and (d["K"][:, dr] == 0).all()
    assert (d["K"][3:6] == 0).all()
    # -- the device's gain in float64: stable, and as cheap to fly as the host build's
    rho = L.rho(Ad, Bd, Kd, q)
    assert (rho[keep] < 1).all(), rho.max()
    cd, ch = (L.excess_cost(Ad[..., keep], Bd[..., keep], K[..., keep], P64[..., keep], q, L.R1) for K in (Kd, K32))
    print(f"[lqr] {name} n={n}: rho {rho[keep].max():.4f}; excess cost device {cd.max():.2e} host {ch.max():.2e}")
    assert (cd <= 8 * ch.max()).all(), ("closed-loop cost", cd.max(), ch.max())


def test_frozen_instances_are_bit_identical(gpu):
    ac, orc, xg, ug = L.grid("poly")
    x, u = L.cycle(xg, 65), L.cycle(ug, 65)
    a = run(ac, gpu, x, u, L.Q11, iters=16)
    b = run(ac, gpu, x, u, L.Q11, iters=20)
    done = a["st"] == 0
    assert done.sum() >= 60 and (a["it"][done] <= 16).all(), (done.sum(), a["it"])
    for k in ("P", "K", "res"):
        assert bits_equal(a[k][..., done], b[k][..., done]), k
    assert np.array_equal(a["it"][done], b["it"][done]) and (b["st"][done] == 0).all()
    short = run(ac, gpu, x, u, L.Q11, iters=3)
    assert (short["st"] == 1).all() and (short["it"] == 3).all() and np.isfinite(short["P"]).all()


# ---- 2. planted bad columns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poly", "real_net"])
def test_planted_nan_columns(gpu, name):
    ac, orc, xg, ug = L.grid(name)
    x, u = L.cycle(xg, 65), L.cycle(ug, 65)
    clean = run(ac, gpu, x, u, L.Q8)
    xb, ub = x.copy(), u.copy()
    xb[4, 7] = np.nan       # a velocity
    ub[1, 20] = np.nan      # the elevator
    ub[4, 33] = np.nan      # a thrust row (the force model ignores it; the design still refuses it)
    xb[8, 64] = np.inf      # the last instance of the batch
    bad = np.zeros(65, bool)
    bad[[7, 20, 33, 64]] = True
    d = run(ac, gpu, xb, ub, L.Q8)
    assert (d["st"][bad] == 3).all() and (d["it"][bad] == 0).all()
    for k in ("P", "K", "res"):
        assert np.isnan(d[k][..., bad]).all(), k
        assert bits_equal(d[k][..., ~bad], clean[k][..., ~bad]), k
    for k in ("A", "B"):
        assert bits_equal(d[k][..., ~bad], clean[k][..., ~bad]), k
    assert np.array_equal(d["st"][~bad], clean["st"][~bad]) and np.array_equal(d["it"][~bad], clean["it"][~bad])


# ---- 3. gains and error ---------------------------------------------------------------------------------------------------------
def test_gains_and_error(gpu):
    import torch

    ac, orc, xg, ug = L.grid("poly")
    turning = np.abs(xg[12]) > 0.01
    x, u = L.cycle(xg[:, turning], 65), L.cycle(ug[:, turning], 65)
    m = int(turning.sum())
    Hn = 8
    A, B = L.oracle_projection(orc, x, u)
    K = L.f32x(L.solve(A, B, L.Q11)[1])
    Xnom_d = ac.rollout(torch.tensor(x, dtype=torch.float32, device=gpu),
                        torch.tensor(np.repeat(u[None], Hn, axis=0), dtype=torch.float32, device=gpu), L.DT)
    Xnom = Xnom_d.cpu().numpy().astype(np.float64)
    assert np.abs(Xnom[-1, 6:10] - Xnom[0, 6:10]).max() > 1e-3  # the attitude turns: E changes from node to node
    Kd = torch.tensor(K, dtype=torch.float32, device=gpu)
    g = Guarded((Hn, 7, 13, 65), gpu)
    lib = ac._sync()
    assert lib.ac_lqr_gains_f32(ac._handle, Xnom_d.data_ptr(), Kd.data_ptr(), 65, Hn, g.ptr(), ac._stream()) == 0
    torch.cuda.synchronize()
    g.check()
    want, host = L.expand(Xnom, K), L.host_gains(Xnom, K)
    e32 = np.max([L.unit_max_rel(host[k], want[k]) for k in range(Hn)])
    err = np.max([L.unit_max_rel(g.np()[k], want[k]) for k in range(Hn)])
    print(f"[lqr] gains: e32 {e32:.2e}, device {err:.2e}")
    assert e32 <= 2 * L.E32_WORST["gains"] and err <= 8 * e32
    assert (g.np()[:, 3:6] == 0).all()
    # the Python surface returns the same bits
    from aircraft_amd import LqrResult

    res = LqrResult(Kd, None, None, None, None, None, None, None, None, None, L.DT, None, None, ac)
    assert torch.equal(res.gains(Xnom_d), g.t)
    # -- the chart
    rng = np.random.default_rng(5)
    xi0 = rng.uniform(-1, 1, (12, 65)) * np.array([5, 5, 5, 1, 1, 1, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])[:, None]
    xs = L.f32x(L.unchart(xi0, x))
    want = L.chart(xs, x)
    den = np.maximum(np.abs(want).max(axis=0), 1.0)
    e32 = (L.unit_max_abs(L.host_error(xs, x), want) / den).max()
    got = ac.steady_error(xs, x)
    err = (L.unit_max_abs(got, want) / den).max()
    print(f"[lqr] steady_error: e32 {e32:.2e}, device {err:.2e}")
    assert e32 <= 2 * L.E32_WORST["xi"] and err <= 8 * e32
    for n in L.SIZES:
        xn = L.cycle(xg, n)
        assert (ac.steady_error(xn, xn) == 0).all()
    # opposite quaternion signs are the same attitude
    xneg = xs.copy()
    xneg[6:10] *= -1
    assert np.array_equal(ac.steady_error(xneg, x), got)


# ---- 4. closed loop ---------------------------------------------------------------------------------------------------------------
def test_closed_loop_against_oracle(gpu):
    """H = 200 steps of 0.01 s from |xi_0| = lqr_ref.XI0_SIZE (0.5 m, 0.5 m/s, 0.02 rad, 0.02 rad/s per coordinate, random
    signs), path hold (selection 11).  tests/test_lqr_ref.py shows on the CPU that the float64 loop alone lets xi' P xi fall
    from the first node to the last from this start.  The device's loop against the oracle's loop with the device's gains
    and nominal under check_against_conditioning; the device's final cost-to-go falls as the oracle's does (5 %: states
    within 1e-5 block-relative are within 2 mm and 0.7 mm/s, against errors of 0.1 .. 0.5 still left at the last node)."""
    ac, orc, x, u = L.grid("poly")
    n, H = x.shape[1], L.H_LOOP
    res = ac.lqr((x, u), L.DT, q=L.Q11)
    assert res.converged.all() and res.K.shape == (7, 12, n) and res.P.shape == (12, 12, n)
    x0 = L.f32x(L.unchart(L.closed_loop_start(n), x))
    X, U, Xnom = ac.rollout_lqr(res, x0, H)
    assert X.shape == (H + 1, 13, n) and U.shape == (H, 7, n) and Xnom.shape == (H + 1, 13, n)
    Kx = res.gains(Xnom)
    assert Kx.shape == (H, 7, 13, n)

    def loop(x_start):
        return L.closed_loop(orc, x_start, x, u, Kx, Xnom=Xnom)[0]

    Xr = loop(x0)
    rng = np.random.default_rng(0)
    cond = np.zeros(n)
    for _ in range(2):
        Xp = loop(x0 * (1.0 + 1e-7 * rng.choice([-1.0, 1.0], x0.shape)))
        cond = np.maximum(cond, np.nan_to_num(instance_err(Xp, Xr), nan=np.inf))
    check_against_conditioning("lqr_closed_loop[poly]", X, Xr, cond, STATE_TOL)
    A, B = L.oracle_projection(orc, x, u)
    P = L.solve(A, B, L.Q11)[0]
    v0, vH, vHr = L.cost_to_go(X[0], Xnom[0], P), L.cost_to_go(X[-1], Xnom[-1], P), L.cost_to_go(Xr[-1], Xnom[-1], P)
    print(f"[lqr] closed loop: xi'P xi falls by {np.min(v0 / vH):.2f} .. {np.max(v0 / vH):.1f} x; device / oracle - 1: "
          f"{np.abs(vH / vHr - 1).max():.1e}")
    assert (vHr < v0).all() and (vH < v0).all()
    assert (np.abs(vH / vHr - 1) <= 0.05).all()
    # the chart on the device sees the same decay
    xiH = ac.steady_error(X[-1], Xnom[-1])
    assert (np.einsum("in,ijn,jn->n", xiH, P, xiH) < v0).all()
    # control limits: the loop clips
    lim = (np.full(7, -0.05), np.full(7, 0.05))
    Xc, Uc, _ = ac.rollout_lqr(res, x0, 20, limits=(u.min(axis=1) + lim[0], u.max(axis=1) + lim[1]))
    assert (Uc <= (u.max(axis=1) + lim[1])[None, :, None] + 1e-6).all() and (Uc >= (u.min(axis=1) + lim[0])[None, :, None] - 1e-6).all()


# ---- 5. the ABI -------------------------------------------------------------------------------------------------------------------
def test_lqr_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    ac, orc, xg, ug = L.grid("poly")
    ac._sync()
    n = 8
    X = torch.tensor(L.cycle(xg, n), dtype=torch.float32, device=gpu)
    U = torch.tensor(L.cycle(ug, n), dtype=torch.float32, device=gpu)
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    A, B, P, K, res = z(12, 12, n), z(12, 7, n), z(12, 12, n), z(7, 12, n), z(n)
    S, it = torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu)
    need = C.c_size_t()
    assert lib.ac_lqr_workspace_floats(ac._handle, n, C.byref(need)) == 0 and need.value >= n * 273
    ws = z(need.value)
    o = L.lqr_opts()

    def call(h, opts, iters=24, wsn=need.value, dt=L.DT, n_=n, x_ptr=X.data_ptr()):
        return lib.ac_lqr_f32(h, C.byref(opts), x_ptr, U.data_ptr(), C.c_float(dt), iters, n_, A.data_ptr(), B.data_ptr(), P.data_ptr(),
                              K.data_ptr(), res.data_ptr(), S.data_ptr(), it.data_ptr(), ws.data_ptr(), wsn, None)

    assert call(ac._handle, o) == 0
    torch.cuda.synchronize()
    assert (S == 0).all()
    assert call(ac._handle, o, wsn=need.value - 1) == -6  # AC_ERR_WORKSPACE
    assert call(ac._handle, o, iters=0) == -1  # AC_ERR_BAD_ARG
    assert call(ac._handle, o, dt=0.0) == -1 and call(ac._handle, o, n_=-1) == -1 and call(ac._handle, o, x_ptr=None) == -1
    assert call(ac._handle, o, n_=0) == 0
    for field, i, v in (("q", 4, -1.0), ("q", 0, float("nan")), ("r", 2, 0.0), ("r", 6, -1.0), ("tol", None, -1.0)):
        bad = _lib.LqrOpts.from_buffer_copy(o)
        if i is None:
            setattr(bad, field, v)
        else:
            getattr(bad, field)[i] = v
        assert call(ac._handle, bad) == -1, (field, i, v)
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle, o) == -3  # AC_ERR_UNSUPPORTED
    assert lib.ac_lqr_workspace_floats(qd._handle, n, C.byref(need)) == -3
    Kx, xi = z(4, 7, 13, n), z(12, n)
    Xnom = z(5, 13, n)
    assert lib.ac_lqr_gains_f32(qd._handle, Xnom.data_ptr(), K.data_ptr(), n, 4, Kx.data_ptr(), None) == -3
    assert lib.ac_steady_error_f32(qd._handle, X.data_ptr(), X.data_ptr(), n, xi.data_ptr(), None) == -3
    assert lib.ac_lqr_gains_f32(ac._handle, None, K.data_ptr(), n, 4, Kx.data_ptr(), None) == -1
    assert lib.ac_lqr_gains_f32(ac._handle, Xnom.data_ptr(), K.data_ptr(), n, -1, Kx.data_ptr(), None) == -1
    assert lib.ac_steady_error_f32(ac._handle, X.data_ptr(), None, n, xi.data_ptr(), None) == -1
    torch.cuda.synchronize()


def test_lqr_from_a_trim_result(gpu):
    """Aircraft.lqr takes the TrimResult itself; numpy in, numpy out; one instance as vectors"""
    ac, orc, xg, ug = L.grid("poly")
    trim = ac.trim(np.linspace(30.0, 50.0, 5), turn_rate=0.1)
    assert trim.converged.all()
    a = ac.lqr(trim, L.DT)
    b = ac.lqr((trim.x, trim.u), L.DT, q=L.Q8, r=L.R1)
    assert a.converged.all() and a.K.shape == (7, 12, 5) and a.K.dtype == np.float64 and a.dt == L.DT
    for k in ("K", "P", "A", "B", "residual", "status", "iterations"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    one = ac.lqr((trim.x[:, 2], trim.u[:, 2]), L.DT)
    assert one.K.shape == (7, 12) and np.array_equal(one.K, a.K[:, :, 2]) and int(one.status) == 0
    d = L.dropped(L.Q8)
    assert (a.P[d] == 0).all() and (a.K[:, d] == 0).all() and (a.K[3:6] == 0).all()
    assert (L.rho(a.A, a.B, a.K, L.Q8) < 1).all()


def test_lqr_graph_replay(gpu):
    import torch

    ac, orc, xg, ug = L.grid("poly")
    n = 65
    X = torch.tensor(L.cycle(xg, n), dtype=torch.float32, device=gpu)
    U = torch.tensor(L.cycle(ug, n), dtype=torch.float32, device=gpu)
    ref = ac.lqr((X, U), L.DT, q=L.Q11)
    ws = ac.lqr_workspace(n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.lqr((X, U), L.DT, q=L.Q11, ws=ws)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = ac.lqr((X, U), L.DT, q=L.Q11, ws=ws)
    g.replay()
    torch.cuda.synchronize()
    for k in ("K", "P", "A", "B", "residual", "status", "iterations"):
        assert torch.equal(getattr(ref, k), getattr(out, k)), k
    assert bool(out.converged.all())
