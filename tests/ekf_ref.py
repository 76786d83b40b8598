"""Float64 restatement of the extended Kalman filter over the step sensitivities (aircraft_amd/csrc/ac_ekf.hpp;
include/aircraft_hip.h, ac_ekf_step_f32) for the tests: the multiplicative error chart and its tangents G and
E, the measurement function and its analytic Jacobian, the time update, the fifteen sequential scalar updates and the batch
Joseph update they must agree with, the error measures, the inputs of the parity tests, the host build's entry points and
the recorded worst float32 errors E32_WORST.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import ctypes as C

import numpy as np

from tests import lqr_ref as L
from tests import trim_ref as T

ROWS = 15
ALL = 0x7FFF
GPS = 0x3F
DT = 0.01
MAG = np.array([0.45, 0.03, 0.89])
# the issue's noise levels: sigma of the initial error, of the process noise per step and of the 15 measurement rows
SIG_P0 = np.array([2, 2, 2, 0.5, 0.5, 0.5, 0.03, 0.03, 0.05, 0.05, 0.05, 0.05])
SIG_Q = np.array([0.01] * 3 + [0.05] * 3 + [0.002] * 3 + [0.02] * 3)
SIG_R = np.array([1.5, 1.5, 3, 0.2, 0.2, 0.3, 0.01, 0.01, 0.01, 0.5, 0.01, 0.01, 0.02, 0.02, 0.02])
MODELS = ("poly", "default", "linear", "real_net", "net_4x128")
SIZES = L.SIZES

# e32: the host build (g++, -ffp-contract=off) against this restatement on identical float32-rounded inputs (x, P, x-, A, z,
# Qd, Rd), worst instance over the grids of MODELS, the mask cases (mask_cases) and the 20-step chain (chain_inputs; per step,
# both chains on their own estimates).  tests/test_host_ekf.py measures them and fails if they are exceeded; DESIGN.md §4.14
# quotes them.  The GPU tests check an instance when its e32 is within 2 x these and hold the device to 8 x the worst e32 of
# the checked instances of its batch.  Measures: see the functions below.
E32_WORST = {"x": 8.0e-6, "P": 3.5e-4, "S": 4.4e-6, "nu": 4.6e-5, "nis": 2.4e-5, "ll": 9.0e-6, "Ppred": 6.5e-7, "Abar": 2.6e-7,
             "mag": 1.9e-7}

f32x, c32, cycle, mm, mv, mtv, tr, skew = L.f32x, L.c32, L.cycle, L.mm, L.mv, L.mtv, L.tr, L.skew
I3 = np.eye(3)[:, :, None]


def epsilon(ac):
    return float(ac._param_struct().epsilon)


# ---- the chart ---------------------------------------------------------------------------------------------------------------
def boxplus(x, d):
    """x [+] d: x (13, n), d (12, n)"""
    e = np.concatenate([0.5 * d[6:9], np.ones((1, d.shape[1]))])
    q = T.qmul(x[6:10], e)
    return np.concatenate([x[0:3] + d[0:3], x[3:6] + d[3:6], q / np.sqrt((q * q).sum(0)), x[10:13] + d[9:12]])


def boxminus(x, xb):
    """the d with xb [+] d = x (x of unit attitude; rotations of less than pi)"""
    e = T.qmul(T.qconj(xb[6:10]), x[6:10])  # (the norm of xb's attitude cancels in the ratio)
    return np.concatenate([x[0:3] - xb[0:3], x[3:6] - xb[3:6], 2 * e[:3] / e[3], x[10:13] - xb[10:13]])


def G_of(x):
    """d(x [+] d)/dd at 0 (13, 12, n)"""
    n = x.shape[1]
    a, w = x[6:9], x[9]
    G = np.zeros((13, 12, n))
    G[0:3, 0:3] = G[3:6, 3:6] = G[10:13, 9:12] = I3
    G[6:9, 6:9] = 0.5 * (w * I3 + skew(a))
    G[9, 6:9] = -0.5 * a
    return G


def E_of(x):
    """dd/dx (12, 13, n)"""
    n = x.shape[1]
    a, w = x[6:9], x[9]
    n2 = (x[6:10] ** 2).sum(0)
    E = np.zeros((12, 13, n))
    E[0:3, 0:3] = E[3:6, 3:6] = E[9:12, 10:13] = I3
    E[6:9, 6:9] = 2 * (w * I3 - skew(a)) / n2
    E[6:9, 9] = -2 * a / n2
    return E


# ---- measurements ------------------------------------------------------------------------------------------------------------
def _air(x, eps):
    R = L.rotmat(L.unit(x[6:10]))
    vb = mtv(R, x[3:6])
    vr = vb + eps
    V = np.sqrt((vr * vr).sum(0) + eps)
    return R, vb, vr, V


def h(x, mag=MAG, eps=0.0):
    """h(x) (15, n)"""
    R, vb, vr, V = _air(x, eps)
    n = x.shape[1]
    return np.concatenate([x[0:3], x[3:6], x[10:13], V[None], np.arctan2(vr[2], vr[0] + eps)[None], np.arcsin(vr[1] / V)[None],
                           mtv(R, np.repeat(np.asarray(mag, dtype=np.float64)[:, None], n, axis=1))])


def H_of(x, mag=MAG, eps=0.0):
    """dh(x [+] d)/dd at 0 (15, 12, n), analytic"""
    n = x.shape[1]
    R, vb, vr, V = _air(x, eps)
    cx, cy, cz = vr[0] + eps, vr[1], vr[2]
    J = np.zeros((3, 3, n))
    J[0] = vr / V
    J[1, 0], J[1, 2] = -cz / (cx * cx + cz * cz), cx / (cx * cx + cz * cz)
    J[2] = -cy * vr / (V * V * np.sqrt(V * V - cy * cy))
    J[2, 1] += 1.0 / np.sqrt(V * V - cy * cy)
    H = np.zeros((ROWS, 12, n))
    H[0:3, 0:3] = H[3:6, 3:6] = H[6:9, 9:12] = I3
    H[9:12, 3:6] = mm(J, tr(R))
    H[9:12, 6:9] = mm(J, skew(vb))
    H[12:15, 6:9] = skew(mtv(R, np.repeat(np.asarray(mag, dtype=np.float64)[:, None], n, axis=1)))
    return H


# ---- the filter --------------------------------------------------------------------------------------------------------------
def abar(x, xp, A):
    """Abar = E(x-) A G(x) (12, 12, n)"""
    return mm(mm(E_of(xp), A), G_of(x))


def sym(P):
    return 0.5 * (P + tr(P))


def predict(x, P, xp, A, Qd):
    """-> Abar, P- = Abar P Abar' + diag(Qd)"""
    Ab = abar(x, xp, A)
    Pm = sym(mm(mm(Ab, P), tr(Ab)))
    Pm[np.arange(12), np.arange(12)] += Qd
    return Ab, Pm


def update(xm, Pm, z, mask, Rd, mag=MAG, eps=0.0):
    """The fifteen scalar updates in row order at the prediction (xm, Pm) -> dict of X, P, nu, S, nis, ll, used, status, d.
    mask: None or (n,) integers."""
    n = xm.shape[1]
    mask = np.full(n, ALL) if mask is None else np.asarray(mask).astype(np.int64)
    with np.errstate(all="ignore"):
        predok = np.isfinite(xm).all(axis=0) & np.isfinite(Pm).reshape(-1, n).all(axis=0)
        xs = np.where(predok, xm, 0.0)
        xs[9] = np.where(predok, xm[9], 1.0)
        xs[3] = np.where(predok, xm[3], 30.0)
        H = H_of(xs, mag, eps)
        nu0 = z - h(xs, mag, eps)
        P, d = np.where(predok, Pm, 0.0), np.zeros((12, n))
        nu, S = np.zeros((ROWS, n)), np.zeros((ROWS, n))
        nis, ll = np.zeros(n), np.zeros(n)
        usedbits, rejected, applied = np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, int)
        for i in range(ROWS):
            hi = H[i]
            ph = np.einsum("rjn,jn->rn", P, hi)
            s = (hi * ph).sum(0) + Rd[i]
            rho = nu0[i] - (hi * d).sum(0)
            used = predok & (((mask >> i) & 1) == 1) & np.isfinite(z[i])
            ok = used & (s > 0) & np.isfinite(s)
            rejected |= used & ~ok
            w = np.where(ok, 1.0 / np.where(ok, s, 1.0), 0.0)
            r_ok, ph_ok = np.where(ok, rho, 0.0), np.where(ok, ph, 0.0)
            d = d + ph_ok * (r_ok * w)
            P = P - ph_ok[:, None] * ph_ok[None, :] * w
            nu[i], S[i] = np.where(used, rho, 0.0), np.where(used, s, 0.0)
            nis += r_ok * r_ok * w
            ll += np.where(ok, -0.5 * (np.log(2 * np.pi * np.where(ok, s, 1.0)) + r_ok * r_ok * w), 0.0)
            usedbits |= np.where(used, 1 << i, 0)
            applied += ok
        X = np.where(applied > 0, boxplus(xs, d), xm)
        P = np.where(predok, P, Pm)
    return dict(X=X, P=P, nu=nu, S=S, nis=nis, ll=ll, used=usedbits, status=rejected * 1 + (~predok) * 2, d=d)


def step(x, P, xp, A, z, mask, Qd, Rd, mag=MAG, eps=0.0, predict_=True):
    """one filter step from the estimate (x, P) with the step xp = F(x, u, dt) and its Jacobian A -> update()'s dict plus
    Xpred, Ppred, Abar"""
    n = x.shape[1]
    if predict_:
        Ab, Pm = predict(x, P, xp, A, Qd)
        xm = xp
    else:
        Ab, Pm, xm = np.repeat(np.eye(12)[:, :, None], n, axis=2), sym(P), x
    out = update(xm, Pm, z, mask, Rd, mag, eps)
    out.update(Xpred=xm, Ppred=Pm, Abar=Ab)
    return out


def simulate(orc, x0, u, T, Qd, Rd, rng, mag=MAG, eps=0.0, dt=DT):
    """Truth driven by process noise through [+] under constant controls, and its noisy measurements:
    x_{t+1} = F(x_t, u) [+] N(0, Qd), z_{t+1} = h(x_{t+1}) + N(0, Rd) -> truth (T+1, 13, n), Z (T, 15, n) float32-exact"""
    X, Z = [np.array(x0, dtype=np.float64)], []
    n = x0.shape[1]
    for _ in range(T):
        X.append(boxplus(orc.state_update(X[-1], u, dt), np.sqrt(Qd) * rng.standard_normal((12, n))))
        Z.append(f32x(h(X[-1], mag, eps) + np.sqrt(Rd) * rng.standard_normal((ROWS, n))))
    return np.stack(X), np.stack(Z)


def chain(step_fn, sens_fn, x, P, u, Z, masks, Qd, Rd, mag=MAG, eps=0.0, dt=DT, host=False):
    """T filter steps with step_fn (step or host_step) from (x, P), the step and its Jacobian at each estimate from
    sens_fn(x, u, dt) -> (x-, A, ..): -> dict of the per-step outputs stacked on a leading axis, ll summed in step order
    (host: step_fn is host_step; the sum is then float32, as ac_ekf_filter_f32 forms it)"""
    outs, ll = [], None
    for t in range(Z.shape[0]):
        xp, A = sens_fn(x, u, dt)[:2]
        kw = dict(ll_in=ll) if host and ll is not None else {}
        o = step_fn(x, P, xp, A, Z[t], None if masks is None else masks[t], Qd, Rd, mag, eps, **kw)
        ll = o["ll32"] if host else (o["ll"] if ll is None else ll + o["ll"])
        x, P = o["X"], o["P"]
        outs.append(o)
    res = {k: np.stack([o[k] for o in outs]) for k in ("X", "P", "nu", "S", "nis", "used", "status")}
    res["ll"] = np.asarray(ll, dtype=np.float64)
    return res


def chain_errors(got, ref):
    """the step measures, worst over the steps of a chain (ll: of the sum) -> dict of (n,)"""
    T_ = ref["X"].shape[0]
    e = {"x": np.max([err_state(got["X"][t], ref["X"][t]) for t in range(T_)], axis=0),
         "P": np.max([err_P(got["P"][t], ref["P"][t]) for t in range(T_)], axis=0),
         "S": np.max([err_S(got["S"][t], ref["S"][t]) for t in range(T_)], axis=0),
         "nu": np.max([err_nu(got["nu"][t], ref["nu"][t], ref["S"][t]) for t in range(T_)], axis=0),
         "nis": np.max([err_scalar(got["nis"][t], ref["nis"][t]) for t in range(T_)], axis=0),
         "ll": err_scalar(got["ll"], ref["ll"])}
    return e


CHAIN_T = 20


def chain_inputs(name, n=None, T_=CHAIN_T, seed=0):
    """inputs(name) (cycled to n) with T_ steps of simulated measurements from its truth and masks with the GPS rows every
    5th step -> the dict of inputs plus Z (T, 15, n), masks (T, n)"""
    d = dict(inputs(name, seed))
    m = d["x"].shape[1]
    rng = np.random.default_rng(200 + seed)
    with np.errstate(all="ignore"):
        Xt, Z = simulate(d["orc"], d["truth"], d["u"], T_, d["Qd"], d["Rd"], rng, MAG, d["eps"])
        # the flights that stay flights: at 70 m/s the default model's pitch mode is outside RK4's stability region at this dt
        # and the TRUTH reaches 1e8 rad/s within six steps (helpers.well_conditioned draws the same line)
        keep = np.isfinite(Xt).all(axis=(0, 1)) & (np.abs(Xt[:, 10:13]).max(axis=(0, 1)) < 5.0)
    masks = np.full((T_, m), ALL & ~GPS, np.int32)
    masks[4::5] = ALL
    d.update(Z=Z, masks=masks)
    for k in ("x", "u", "P", "z", "Qd", "Rd", "truth", "Z", "masks"):
        d[k] = d[k][..., keep]
    if n is not None:
        for k in ("x", "u", "P", "z", "Qd", "Rd", "truth", "Z", "masks"):
            d[k] = cycle(d[k], n)
    return d


def joseph(xm, Pm, z, rows, Rd, mag=MAG, eps=0.0):
    """The batch Kalman update over `rows` (the same for every instance) in Joseph form -> P, d, nis, ll"""
    n = xm.shape[1]
    H, nu0 = H_of(xm, mag, eps), z - h(xm, mag, eps)
    P, d, nis, ll = np.zeros((12, 12, n)), np.zeros((12, n)), np.zeros(n), np.zeros(n)
    for k in range(n):
        Hk, Pk, R = H[rows, :, k], Pm[:, :, k], np.diag(Rd[rows, k])
        Sk = Hk @ Pk @ Hk.T + R
        K = np.linalg.solve(Sk, Hk @ Pk).T
        IKH = np.eye(12) - K @ Hk
        P[:, :, k] = IKH @ Pk @ IKH.T + K @ R @ K.T
        d[:, k] = K @ nu0[rows, k]
        nis[k] = nu0[rows, k] @ np.linalg.solve(Sk, nu0[rows, k])
        ll[k] = -0.5 * (np.linalg.slogdet(2 * np.pi * Sk)[1] + nis[k])
    return P, d, nis, ll


# ---- measures (per instance, (n,)) -------------------------------------------------------------------------------------------
def err_state(a, ref):
    from tests.helpers import instance_err

    return instance_err(a, ref)


def err_P(a, ref):
    """max |dP_ij| / sqrt(P64_ii P64_jj)"""
    dg = np.sqrt(ref[np.arange(12), np.arange(12)])
    return (np.abs(a - ref) / (dg[:, None] * dg[None, :])).reshape(144, -1).max(axis=0)


def err_S(a, ref):
    with np.errstate(all="ignore"):
        return np.where(ref > 0, np.abs(a - ref) / ref, (a != ref) * 1.0).max(axis=0)


def err_nu(a, ref, S):
    with np.errstate(all="ignore"):
        return np.where(S > 0, np.abs(a - ref) / np.sqrt(S), (a != ref) * 1.0).max(axis=0)


def err_scalar(a, ref):
    return np.abs(a - ref) / (1 + np.abs(ref))


def errors(got, ref):
    """every measure of a step's outputs (dicts with X, P, nu, S, nis, ll and optionally Ppred, Abar) -> dict of (n,)"""
    e = {"x": err_state(got["X"], ref["X"]), "P": err_P(got["P"], ref["P"]), "S": err_S(got["S"], ref["S"]),
         "nu": err_nu(got["nu"], ref["nu"], ref["S"]), "nis": err_scalar(got["nis"], ref["nis"]), "ll": err_scalar(got["ll"], ref["ll"])}
    if got.get("Ppred") is not None:
        e["Ppred"] = err_P(got["Ppred"], ref["Ppred"])
    if got.get("Abar") is not None:
        e["Abar"] = L.unit_max_rel(got["Abar"], ref["Abar"])
    return e


KEYS = ("x", "P", "S", "nu", "nis", "ll", "Ppred", "Abar")


def checked(e32):
    """instances whose host/float64 pair is within 2 x the recorded worst in every measure"""
    keep = np.ones(len(e32["x"]), bool)
    for k, v in e32.items():
        keep &= v <= 2 * E32_WORST[k]
    return keep


def hold(name, dev, e32, distinct):
    """The bars: at most 5 % of the batch's distinct instances left out; the device within 8 x the worst e32 of the checked
    instances, measure by measure.  Prints each figure before it asserts."""
    keep = checked(e32)
    left = int((~keep[:distinct]).sum())
    worst = {k: (float(dev[k][keep].max()), float(e32[k][keep].max())) for k in e32} if keep.any() else {}
    print(f"[ekf] {name}: left out {left}/{distinct}; " + ", ".join(f"{k} dev {d:.2e} e32 {e:.2e}" for k, (d, e) in worst.items()))
    assert left <= 0.05 * distinct, (name, "e32 condition: left out", left, "of", distinct, {k: float(v.max()) for k, v in e32.items()})
    for k, (d, e) in worst.items():
        assert d <= 8 * e, (name, k, d, e)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def correlation(rng):
    M = rng.standard_normal((12, 24))
    Cm = M @ M.T
    s = np.sqrt(np.diag(Cm))
    return Cm / s[:, None] / s[None, :]


_INPUTS = {}


def inputs(name, seed=0, scale=1.0):
    """The distinct instances of the parity tests for the model `name` (cycle() them to a batch size): the trims of
    lqr_ref.grid(name) as estimates, P0 = D^1/2 C D^1/2 with a seeded random correlation C, truth = x [+] d with d ~ N(0, P0),
    z = h(F(truth)) + N(0, Rd).  Everything float32-exact.  -> dict(ac, orc, eps, x, u, P, z, Qd, Rd)"""
    key = (name, seed, scale)
    if key in _INPUTS:
        return _INPUTS[key]
    ac, orc, x, u = L.grid(name)
    m = x.shape[1]
    rng = np.random.default_rng(100 + seed)
    eps = epsilon(ac)
    sp = SIG_P0 * scale
    P, d = np.zeros((12, 12, m)), np.zeros((12, m))
    for k in range(m):
        P[:, :, k] = f32x(sp[:, None] * correlation(rng) * sp[None, :])
        d[:, k] = np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12)
    truth = boxplus(x, d)
    Rd = f32x(np.repeat((SIG_R ** 2)[:, None], m, axis=1))
    Qd = f32x(np.repeat((SIG_Q ** 2)[:, None], m, axis=1))
    z = f32x(h(orc.state_update(truth, u, DT), MAG, eps) + np.sqrt(Rd) * rng.standard_normal((ROWS, m)))
    out = dict(ac=ac, orc=orc, eps=eps, x=x, u=u, P=P, z=z, Qd=Qd, Rd=Rd, truth=truth)
    _INPUTS[key] = out
    return out


def measure_states(name, seed=3):
    """the states the measurement function is checked at: the estimates of inputs(name) displaced by N(0, SIG_P0) through [+],
    attitudes of any norm (0.8 .. 1.2), float32-exact (13, m)"""
    d = inputs(name)
    m = d["x"].shape[1]
    rng = np.random.default_rng(seed)
    x = boxplus(d["x"], SIG_P0[:, None] * rng.standard_normal((12, m)))
    x[6:10] *= 1.0 + 0.2 * rng.uniform(-1, 1, m)
    return f32x(x)


def mask_cases(n):
    """name -> mask (n,) (None: all rows): every single row, no row, GPS only, everything but GPS"""
    out = {"all": None, "none": np.zeros(n, np.int32), "gps": np.full(n, GPS, np.int32), "no_gps": np.full(n, ALL & ~GPS, np.int32)}
    for i in range(ROWS):
        out[f"row{i}"] = np.full(n, 1 << i, np.int32)
    return out


# ---- the host build's entry points (tests/host_ekf/ekf_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) ---------------------
def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def ekf_opts(mag=MAG, predict_=True):
    from aircraft_amd import _lib

    o = _lib.EkfOpts()
    o.mag_ned[:] = [float(v) for v in mag]
    o.predict = int(predict_)
    return o


def host_step(x, P, xp, A, z, mask, Qd, Rd, mag=MAG, eps=0.0, predict_=True, ll_in=None, header=None):
    """the float32 host build on float32-rounded inputs -> the dict of step() (float64 / int arrays)"""
    from tests.test_host_ekf import lib_host

    n = x.shape[1]
    a = [c32(x), c32(np.reshape(P, (144, n))), c32(xp if predict_ else x), c32(np.reshape(A, (169, n))) if predict_ else None, c32(z)]
    mk = None if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
    q, r = c32(Qd), c32(Rd)
    lin = None if ll_in is None else c32(ll_in)
    f = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    Xo, Po, nu, S, nis, ll = f(13, n), f(144, n), f(ROWS, n), f(ROWS, n), f(n), f(n)
    used, st = np.zeros(n, np.int32), np.zeros(n, np.int32)
    Xpred, Ppred, Ab = f(13, n), f(144, n), f(144, n)
    o = ekf_opts(mag, predict_)
    assert lib_host(header).host_ekf_step(C.byref(o), C.c_float(eps), *[_fp(v) for v in a], _ip(mk), _fp(q), _fp(r), _fp(lin), n, _fp(Xo),
                                          _fp(Po), _fp(nu), _fp(S), _fp(nis), _fp(ll), _ip(used), _ip(st), _fp(Xpred), _fp(Ppred),
                                          _fp(Ab)) == 0
    d64 = lambda v: v.astype(np.float64)  # noqa: E731
    return dict(X=d64(Xo), P=d64(Po).reshape(12, 12, n), nu=d64(nu), S=d64(S), nis=d64(nis), ll=d64(ll), used=used, status=st,
                Xpred=d64(Xpred), Ppred=d64(Ppred).reshape(12, 12, n), Abar=d64(Ab).reshape(12, 12, n), P32=Po.reshape(12, 12, n),
                X32=Xo, ll32=ll)


def host_measure(x, mag=MAG, eps=0.0, header=None):
    from tests.test_host_ekf import lib_host

    n = x.shape[1]
    xs, Z = c32(x), np.zeros((ROWS, n), np.float32)
    o = ekf_opts(mag)
    assert lib_host(header).host_ekf_measure(C.byref(o), C.c_float(eps), _fp(xs), n, _fp(Z)) == 0
    return Z.astype(np.float64)
