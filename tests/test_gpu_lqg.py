"""GPU tests of the loop closed through the estimator (ac_sense_f32, ac_disturb_f32, ac_policy_f32, ac_estimate_score_f32,
ac_lqg_rollout_f32, Aircraft.sense / rollout_lqg).

Batches n in SIZES cross the 256-lane workgroup with ragged tails; T = 12 steps, GPS every 5th step from step 2, the air data
dropped 3 times in 10; the cubic-fit and the shipped-net models.  Mask, schedule and control law: the device equals the host
build (tests/host_lqg) bit for bit.  Noisy values: within test_host_lqg's tolerances of float64 (sincosf and logf differ from
the host's).  Score: within 8 x lqg_ref.E32_WORST of float64, every instance.  The rollout: every output equals, bit for bit, a
Python loop over the device's own single-step ABI calls; T-step trajectories are NOT compared with float64 (the closed loop
amplifies rounding).  Every output and the workspace sit between guard words."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import ekf_ref as E
from tests import lqg_ref as R
from tests import lqr_ref as L
from tests.test_gpu_ekf import batch, dev
from tests.test_gpu_lqr import Guarded
from tests.test_host_lqg import disturb_ratios, disturb_tolerance, sense_tolerance

pytestmark = pytest.mark.gpu

MODELS = ("poly", "real_net")
SIZES = (1, 5, 17, 257)
T = 12
CASES = [(m, n) for m in MODELS for n in SIZES]
IDS = [f"{m}-{n}" for m, n in CASES]
SENS = R.Sensors(seed=0xC0FFEE123456789, instance_offset=3, period=(5, 5, 1, 1, 1), phase=(2, 2, 0, 0, 0), dropout=(0.0, 0.0, 0.0, 0.3, 0.0))
LO, HI = np.array([-20.0, -20, -20, -np.inf, -np.inf, -np.inf, 0]), np.array([20.0, 20, 20, np.inf, np.inf, np.inf, 1])
_LOOP = {}
AC_ERR_BAD_ARG, AC_ERR_UNSUPPORTED, AC_ERR_WORKSPACE = -1, -3, -6  # include/aircraft_hip.h


def ibits(t):
    import torch

    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(ibits(a), ibits(b))


def limits(lo=LO, hi=HI):
    lim = _lib.IlqrCost()
    lim.u_min[:] = [float(v) for v in lo]
    lim.u_max[:] = [float(v) for v in hi]
    return lim


def loop_case(name, n):
    """batch(name, n) plus the truth, the float64 LQR gains about every trim and the nominal (cycled like the rest)"""
    if name not in _LOOP:
        d = E.inputs(name)
        A, B = L.oracle_projection(d["orc"], d["x"], d["u"])
        K = L.solve(A, B)[1]
        Unom = np.repeat(d["u"][None], T, axis=0)
        Xnom = E.f32x(d["orc"].rollout(d["x"], Unom, E.DT))
        _LOOP[name] = dict(Xnom=Xnom, Unom=Unom, Kx=E.f32x(L.expand(Xnom, K)), truth=E.f32x(d["truth"]))
    d, m = batch(name, n)
    d.update({k: E.cycle(v, n) for k, v in _LOOP[name].items()})
    return d, m


# ---- the single calls ------------------------------------------------------------------------------------------------------------------
def d_sense(ac, s, step, X, sig, step_dev=None):
    import torch

    n = X.shape[1]
    Z, M = Guarded((15, n), X.device), Guarded((n,), X.device, torch.int32)
    o = R.sense_opts(s)
    rc = ac._sync().ac_sense_f32(ac._handle, C.byref(o), step, None if step_dev is None else step_dev.data_ptr(), X.data_ptr(), sig.data_ptr(),
                                 n, Z.ptr(), M.ptr(), ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    return Z, M


def d_disturb(ac, s, step, X, sig, out=None):
    n = X.shape[1]
    Xo = Guarded((13, n), X.device) if out is None else out
    o = R.sense_opts(s)
    rc = ac._sync().ac_disturb_f32(ac._handle, C.byref(o), step, None, X.data_ptr(), sig.data_ptr(), n, Xo.ptr() if out is None else out.data_ptr(),
                                   ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    return Xo


def d_policy(ac, Fb, Xnom, Unom, Kx, lim=None):
    n = Fb.shape[1]
    U = Guarded((7, n), Fb.device)
    lim = lim or limits()
    rc = ac._sync().ac_policy_f32(ac._handle, C.byref(lim), Fb.data_ptr(), Xnom.data_ptr(), Unom.data_ptr(), Kx.data_ptr(), n, U.ptr(), ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    return U


def d_score(ac, X, Xh, P):
    import torch

    n = X.shape[1]
    e, nees, st = Guarded((12, n), X.device), Guarded((n,), X.device), Guarded((n,), X.device, torch.int32)
    rc = ac._sync().ac_estimate_score_f32(ac._handle, X.data_ptr(), Xh.data_ptr(), P.data_ptr(), n, e.ptr(), nees.ptr(), st.ptr(), ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    return e, nees, st


def checked(*gs):
    import torch

    torch.cuda.synchronize()
    for g in gs:
        g.check()
    return gs


def sig_dev(sig, n, gpu):
    return dev(np.repeat(np.asarray(sig, dtype=np.float64)[:, None], n, axis=1), gpu)


# ---- 1. sense, disturb, policy against the host build and float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_sense_disturb_policy(gpu, name, n):
    d, m = loop_case(name, n)
    ac, eps = d["ac"], d["eps"]
    x = d["truth"]
    X = dev(x, gpu)
    for step in (7, 9):  # 7: the GPS reports (phase 2, period 5); 9: it does not
        Z, M = checked(*d_sense(ac, SENS, step, X, sig_dev(E.SIG_R, n, gpu)))
        Zh, mh = R.host_sense(x, E.SIG_R, SENS, step, eps)
        Z64, mask, hx, rad = R.sense(x, E.SIG_R, SENS, step, eps)
        assert np.array_equal(M.np(), mh) and np.array_equal(mh, mask) and np.array_equal(np.isnan(Z.np()), np.isnan(Zh))
        rep = ~np.isnan(Z64)
        assert rep[0:6].all() == (step == 7) and rep[0:6].any() == (step == 7) and rep[6:9].all()
        tol, err = sense_tolerance(Z64, rad, hx), np.abs(Z.np() - Z64)
        print(f"[lqg] {name}-{n} sense step {step}: worst |dZ| / tol {np.nanmax(err / tol):.3f}; bit-identical to the host build: "
              f"{np.array_equal(Z.np()[rep], Zh.astype(np.float64)[rep])}")
        assert (err[rep] <= tol[rep]).all()
    (Xo,) = checked(d_disturb(ac, SENS, 4, X, sig_dev(E.SIG_Q, n, gpu)))
    Xr, _, rad = R.disturb(x, E.SIG_Q, SENS, 4)
    tol, err = disturb_tolerance(Xr, rad), np.abs(Xo.np() - Xr)
    print(f"[lqg] {name}-{n} disturb: worst |dX| / tol " + disturb_ratios(err, tol))
    assert (err <= tol).all()
    # in place: the same bits
    Xc = X.clone()
    d_disturb(ac, SENS, 4, Xc, sig_dev(E.SIG_Q, n, gpu), out=Xc)
    assert same(Xc, Xo.t)
    # the control law, on the estimate's side of the batch: the host build's bits
    fb = E.f32x(E.boxplus(d["x"], 3 * E.SIG_P0[:, None] * np.random.default_rng(n).standard_normal((12, n))))
    Kx = 3 * d["Kx"][0]  # (scaled so that some rows reach their limits)
    (U,) = checked(d_policy(ac, dev(fb, gpu), dev(d["Xnom"][0], gpu), dev(d["Unom"][0], gpu), dev(Kx, gpu)))
    Uh = R.host_policy(fb, d["Xnom"][0], d["Unom"][0], Kx, LO, HI)
    assert np.array_equal(U.t.cpu().numpy().view(np.int32), Uh.view(np.int32))
    assert np.array_equal(Uh, R.policy32(fb, d["Xnom"][0], d["Unom"][0], Kx, LO, HI))


# ---- 2. an instance's bits depend neither on n nor on its place ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_batch_independence(gpu, name):
    n = 257
    d, m = loop_case(name, n)
    ac = d["ac"]
    X, Xh, P = dev(d["truth"], gpu), dev(d["x"], gpu), dev(d["P"], gpu)
    sr, sq = sig_dev(E.SIG_R, n, gpu), sig_dev(E.SIG_Q, n, gpu)
    Xn, Un, Kx = dev(d["Xnom"][0], gpu), dev(d["Unom"][0], gpu), dev(d["Kx"][0], gpu)
    Z, M = d_sense(ac, SENS, 7, X, sr)
    Xo = d_disturb(ac, SENS, 7, X, sq)
    U = d_policy(ac, Xh, Xn, Un, Kx)
    e, nees, st = d_score(ac, X, Xh, P)
    for i in (0, 16, 255, 256):
        c = slice(i, i + 1)
        si = R.Sensors(seed=SENS.seed, instance_offset=SENS.instance_offset + i, period=SENS.period, phase=SENS.phase, dropout=SENS.dropout)
        Zi, Mi = d_sense(ac, si, 7, X[:, c].contiguous(), sr[:, c].contiguous())
        assert same(Zi.t, Z.t[:, c]) and same(Mi.t, M.t[c])
        assert same(d_disturb(ac, si, 7, X[:, c].contiguous(), sq[:, c].contiguous()).t, Xo.t[:, c])
        assert same(d_policy(ac, Xh[:, c].contiguous(), Xn[:, c].contiguous(), Un[:, c].contiguous(), Kx[:, :, c].contiguous()).t, U.t[:, c])
        ei, ni, sti = d_score(ac, X[:, c].contiguous(), Xh[:, c].contiguous(), P[:, :, c].contiguous())
        assert same(ei.t, e.t[:, c]) and same(ni.t, nees.t[c]) and same(sti.t, st.t[c])
    # a repeated instance gives the same bits wherever it sits (the score and the law draw nothing)
    first = np.arange(n) % m
    assert same(e.t, e.t[:, first]) and same(nees.t, nees.t[first]) and same(U.t, U.t[:, first])


# ---- 3. the score against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_score_against_float64(gpu, name, n):
    d, m = loop_case(name, n)
    e, nees, st = checked(*d_score(d["ac"], dev(d["truth"], gpu), dev(d["x"], gpu), dev(d["P"], gpu)))
    er, nr, sr = R.score(d["truth"], d["x"], d["P"])
    got = {"e": R.err_e(e.np(), er, d["P"]), "nees": E.err_scalar(nees.np(), nr)}
    print(f"[lqg] {name}-{n} score: " + ", ".join(f"{k} dev {v.max():.2e} (8 x worst e32 {8 * R.E32_WORST[k]:.2e})" for k, v in got.items()))
    assert not st.np().any() and not sr.any()
    for k, v in got.items():
        assert (v <= 8 * R.E32_WORST[k]).all(), (k, float(v.max()))


def test_score_status(gpu):
    d, m = loop_case("poly", 5)
    P = d["P"].copy()
    P[3, 3, 1] = -1.0
    P[:, :, 2] = np.nan
    e, nees, st = checked(*d_score(d["ac"], dev(d["truth"], gpu), dev(d["x"], gpu), dev(P, gpu)))
    assert list(st.np()) == [0, 1, 1, 0, 0] and np.isnan(nees.np()[[1, 2]]).all() and np.isfinite(nees.np()[[0, 3, 4]]).all()
    assert np.isfinite(e.np()).all()


# ---- 4. the rollout is its single calls, bit for bit ---------------------------------------------------------------------------------------
OUT_F = dict(Xo=(13,), Po=(12, 12), Xtrue=(T + 1, 13), Xhat=(T + 1, 13), U=(T, 7), Ps=(T, 12, 12), Z=(T, 15), nis=(T,), nees=(T,), err=(T, 12))
OUT_I = ("mask", "used", "est_status", "score_status")
ORDER = ("Xo", "Po", "Xtrue", "Xhat", "U", "Ps", "Z", "mask", "nis", "nees", "used", "est_status", "score_status", "err")


def est_ws_floats(ac, est, n):
    need = C.c_size_t()
    fn = ac._sync().ac_ukf_workspace_floats if est == "ukf" else ac._sync().ac_ekf_workspace_floats
    assert fn(ac._handle, n, C.byref(need)) == 0
    return need.value


def lqg_ws_floats(ac, est, n):
    need = C.c_size_t()
    assert ac._sync().ac_lqg_workspace_floats(ac._handle, _lib.LQG_ESTIMATORS[est], n, C.byref(need)) == 0
    return need.value


def d_rollout(ac, gpu, t, est, feedback, sq, s=SENS, kappa=1.0, step0=4, short=0, steps=T, lim=None, dt=E.DT, handle=None):
    """ac_lqg_rollout_f32 on the device tensors t in guarded buffers -> (rc, dict of Guarded)"""
    import torch

    n = t["X0"].shape[1]
    g = {k: Guarded(shp + (n,), gpu) for k, shp in OUT_F.items()}
    g.update({k: Guarded((T, n), gpu, torch.int32) for k in OUT_I})
    need = lqg_ws_floats(ac, est, n)
    g["ws"] = Guarded((need,), gpu)
    o = _lib.LqgOpts()
    o.estimator, o.feedback, o.kappa, o.step0 = _lib.LQG_ESTIMATORS[est], _lib.LQG_FEEDBACK[feedback], kappa, step0
    so, lim = R.sense_opts(s), lim or limits()
    rc = ac._sync().ac_lqg_rollout_f32(handle or ac._handle, C.byref(o), C.byref(so), C.byref(lim), t["X0"].data_ptr(), t["Xh0"].data_ptr(),
                                       t["P0"].data_ptr(), t["Xnom"].data_ptr(), t["Unom"].data_ptr(), t["Kx"].data_ptr(), t["Qd"].data_ptr(),
                                       t["Rd"].data_ptr(), None if sq is None else sq.data_ptr(), t["sr"].data_ptr(), C.c_float(dt), n, steps,
                                       *[g[k].ptr() for k in ORDER], g["ws"].ptr(), need - short, ac._stream())
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    return rc, g


def tensors(d, gpu, n):
    t = dict(X0=dev(d["truth"], gpu), Xh0=dev(d["x"], gpu), P0=dev(d["P"], gpu), Xnom=dev(d["Xnom"], gpu), Unom=dev(d["Unom"], gpu),
             Kx=dev(d["Kx"], gpu), Qd=dev(d["Qd"], gpu), Rd=dev(d["Rd"], gpu), sr=sig_dev(E.SIG_R, n, gpu), sq=sig_dev(E.SIG_Q, n, gpu))
    return t


def composed(ac, gpu, t, est, feedback, sq, s=SENS, kappa=1.0, step0=4):
    """the same loop as single ABI calls -> dict of tensors"""
    import torch

    lib = ac._sync()
    n = t["X0"].shape[1]
    f32, i32 = dict(device=gpu, dtype=torch.float32), dict(device=gpu, dtype=torch.int32)
    x, xh, P = t["X0"], t["Xh0"], t["P0"]
    out = {k: [] for k in ORDER[2:]}
    out["Xtrue"].append(x)
    out["Xhat"].append(xh)
    need = est_ws_floats(ac, est, n)
    ws = torch.empty(need, **f32)
    eo = E.ekf_opts(E.MAG, True)
    if est == "ukf":
        eo = _lib.UkfOpts()
        eo.mag_ned[:], eo.predict, eo.kappa = [float(v) for v in E.MAG], 1, kappa
    step_fn = lib.ac_ukf_step_f32 if est == "ukf" else lib.ac_ekf_step_f32
    for k in range(T):
        u = d_policy(ac, xh if feedback == "estimate" else x, t["Xnom"][k], t["Unom"][k], t["Kx"][k]).t
        xn = torch.empty((13, n), **f32)
        assert lib.ac_step_f32(ac._handle, x.data_ptr(), u.data_ptr(), C.c_float(E.DT), None, n, xn.data_ptr(), ac._stream()) == 0
        if sq is not None:
            xn = d_disturb(ac, s, step0 + k, xn, sq).t
        Z, M = d_sense(ac, s, step0 + k + 1, xn, t["sr"])
        Xo, Po, nu, S = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32), torch.empty((15, n), **f32), torch.empty((15, n), **f32)
        nis, ll, used, st = torch.empty(n, **f32), torch.empty(n, **f32), torch.empty(n, **i32), torch.empty(n, **i32)
        rc = step_fn(ac._handle, C.byref(eo), xh.data_ptr(), P.data_ptr(), u.data_ptr(), C.c_float(E.DT), Z.ptr(), M.ptr(), t["Qd"].data_ptr(),
                     t["Rd"].data_ptr(), n, Xo.data_ptr(), Po.data_ptr(), nu.data_ptr(), S.data_ptr(), nis.data_ptr(), ll.data_ptr(),
                     used.data_ptr(), st.data_ptr(), None, None, None, ws.data_ptr(), need, ac._stream())
        assert rc == 0, _lib.load().ac_last_error()
        e, nees, sst = d_score(ac, xn, Xo, Po)
        for key, v in (("Xtrue", xn), ("Xhat", Xo), ("U", u), ("Ps", Po), ("Z", Z.t), ("mask", M.t), ("nis", nis), ("nees", nees.t),
                       ("used", used), ("est_status", st), ("score_status", sst.t), ("err", e.t)):
            out[key].append(v)
        x, xh, P = xn, Xo, Po
    torch.cuda.synchronize()
    res = {k: torch.stack(v) for k, v in out.items()}
    res["Xo"], res["Po"] = xh, P
    return res


@pytest.mark.parametrize("est", ("ekf", "ukf"))
@pytest.mark.parametrize("name,n", CASES, ids=IDS)
def test_rollout_is_its_single_calls(gpu, name, n, est):
    d, m = loop_case(name, n)
    ac = d["ac"]
    t = tensors(d, gpu, n)
    for feedback in ("estimate", "truth"):
        for sq in (None, t["sq"]):
            rc, g = d_rollout(ac, gpu, t, est, feedback, sq)
            assert rc == 0, _lib.load().ac_last_error()
            assert ac.last_launch()[0] == "k_lqg_score"  # (every launch of the loop is noted, the last one last)
            ref = composed(ac, gpu, t, est, feedback, sq)
            for k in ORDER:
                assert same(g[k].t, ref[k]), (feedback, sq is not None, k)
            Z, used = g["Z"].np(), g["used"].np()
            # the schedule shows in what the estimator used: GPS at the steps with (step0 + k + 1 - 2) % 5 == 0 only
            gps = np.array([(4 + k + 1 - 2) % 5 == 0 for k in range(T)])
            assert (((used & E.GPS) != 0).any(axis=1) == gps).all() and np.array_equal(np.isnan(Z[:, 0:6]).all(axis=(1, 2)), ~gps)
            assert not g["est_status"].np().any() and not g["score_status"].np().any() and np.isfinite(g["Xtrue"].np()).all()
    # the estimate sees the truth: at the last node the error is inside a generous multiple of what P says
    assert np.nanmax(g["nees"].np()[-1]) < 12 * 25


# ---- 5. no noise: Z is the measurement of the truth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_zero_noise_measures_the_truth(gpu, name):
    import torch

    n = 17
    d, m = loop_case(name, n)
    ac = d["ac"]
    t = tensors(d, gpu, n)
    t["sr"] = torch.zeros_like(t["sr"])
    rc, g = d_rollout(ac, gpu, t, "ekf", "estimate", torch.zeros_like(t["sq"]), s=R.Sensors(seed=1))
    assert rc == 0, _lib.load().ac_last_error()
    lib = ac._sync()
    o = E.ekf_opts(E.MAG)
    for k in range(T):
        Zk = torch.empty((15, n), device=gpu, dtype=torch.float32)
        assert lib.ac_ekf_measure_f32(ac._handle, C.byref(o), g["Xtrue"].t[k + 1].data_ptr(), n, Zk.data_ptr(), ac._stream()) == 0
        assert same(Zk, g["Z"].t[k]), k
    assert (g["mask"].t == E.ALL).all() and (g["used"].t == E.ALL).all()


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_captured_rollout_lqg_and_sense(gpu):
    import torch

    from aircraft_amd import SensorModel

    n = 17
    d, m = loop_case("poly", n)
    ac = d["ac"]
    x, u = dev(d["x"], gpu), dev(d["u"], gpu)
    res = ac.lqr((x, u), E.DT)
    sens = SensorModel(sigma=sig_dev(E.SIG_R, n, gpu), period=SENS.period, phase=SENS.phase, dropout=SENS.dropout, seed=SENS.seed)
    kw = dict(q=dev(d["Qd"], gpu), r=dev(d["Rd"], gpu), mag_ned=E.MAG)
    x0, P0, sq = dev(d["truth"], gpu), dev(d["P"], gpu), sig_dev(E.SIG_Q, n, gpu)

    def fly(bank):
        return ac.rollout_lqg(res, bank, x0, T, sens, process_sigma=sq, record=("P",), ws=ws)

    ws = ac.lqg_workspace("ekf", n)
    eager = fly(ac.ekf(x, P0, **kw))
    bank = ac.ekf(x, P0, **kw)
    xs, Ps = bank._X, bank._P
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fly(bank)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    bank._X, bank._P = xs, Ps
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = fly(bank)
    g.replay()
    torch.cuda.synchronize()
    for k in ("X", "Xhat", "U", "Z", "mask", "nis", "nees", "err", "used", "status", "Xnom", "P"):
        assert same(getattr(eager, k), getattr(out, k)), k
    assert same(bank.x, out.Xhat[-1]) and same(bank.P, out.P[-1]) and tuple(out.X.shape) == (T + 1, 13, n)
    # a captured sense whose step lives on the device: every replay draws the noise of its own step
    step = torch.zeros(1, device=gpu, dtype=torch.int32)
    with torch.cuda.stream(s):
        ac.sense(x0, sens, 3, step_dev=step)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        Z, M = ac.sense(x0, sens, 3, step_dev=step)
    for k in range(4):
        step.fill_(k)
        g2.replay()
        torch.cuda.synchronize()
        Zk, Mk = ac.sense(x0, sens, 3 + k)
        assert same(Z, Zk) and same(M, Mk), k
    assert not same(ac.sense(x0, sens, 3)[0], ac.sense(x0, sens, 4)[0])


# ---- 7. the workspace and the argument checks: nothing is launched -------------------------------------------------------------------------------
def test_short_workspace_and_bad_arguments_launch_nothing(gpu):
    from tests.test_gpu_lqr import F_SENTINEL

    n = 5
    d, m = loop_case("poly", n)
    ac = d["ac"]
    t = tensors(d, gpu, n)
    for est in ("ekf", "ukf"):
        assert lqg_ws_floats(ac, est, n) > est_ws_floats(ac, est, n) + 363 * n
        rc, g = d_rollout(ac, gpu, t, est, "estimate", None, short=1)
        assert rc == AC_ERR_WORKSPACE and b"ac_lqg_workspace_floats" in _lib.load().ac_last_error()
        assert all(bool((g[k].t == F_SENTINEL).all()) for k in OUT_F) and bool((g["ws"].t == F_SENTINEL).all())
    bad = [dict(s=R.Sensors(period=(0, 1, 1, 1, 1))), dict(s=R.Sensors(dropout=(0, 0, 1.0, 0, 0))), dict(s=R.Sensors(dropout=(0, -0.5, 0, 0, 0))),
           dict(dt=0.0), dict(dt=float("inf")), dict(kappa=-1.0), dict(lim=limits(HI, LO)), dict(steps=-1), dict(step0=2 ** 31 - T)]
    for kw in bad:
        rc, g = d_rollout(ac, gpu, t, "ukf", "estimate", None, **kw)
        assert rc == AC_ERR_BAD_ARG, kw
        assert all(bool((g[k].t == F_SENTINEL).all()) for k in OUT_F)
    missing = dict(t)
    missing["Kx"] = type("Null", (), {"data_ptr": staticmethod(lambda: None), "shape": t["Kx"].shape})()
    rc, g = d_rollout(ac, gpu, missing, "ekf", "estimate", None)
    assert rc == AC_ERR_BAD_ARG and all(bool((g[k].t == F_SENTINEL).all()) for k in OUT_F)
    rc, g = d_rollout(ac, gpu, t, "ekf", "estimate", None, steps=0)
    assert rc == 0 and all(bool((g[k].t == F_SENTINEL).all()) for k in OUT_F)
    # the single calls
    lib = ac._sync()
    o = R.sense_opts(R.Sensors(period=(1, 1, 1, 1, 0)))
    assert lib.ac_sense_f32(ac._handle, C.byref(o), 0, None, t["X0"].data_ptr(), t["sr"].data_ptr(), n, None, None, ac._stream()) == AC_ERR_BAD_ARG
    o = R.sense_opts(R.Sensors())
    assert lib.ac_sense_f32(ac._handle, C.byref(o), 0, None, t["X0"].data_ptr(), t["sr"].data_ptr(), n, None, None, ac._stream()) == AC_ERR_BAD_ARG
    assert lib.ac_sense_f32(ac._handle, C.byref(o), 0, None, None, None, 0, None, None, ac._stream()) == 0
    assert lib.ac_estimate_score_f32(ac._handle, None, None, None, -1, None, None, None, ac._stream()) == AC_ERR_BAD_ARG


def test_the_quadrotor_is_refused(gpu):
    from aircraft_amd import Quadrotor
    from tests.test_gpu_lqr import F_SENTINEL

    n = 5
    d, m = loop_case("poly", n)
    ac = d["ac"]
    t = tensors(d, gpu, n)
    qd = Quadrotor()
    lib = qd._sync()
    need = C.c_size_t()
    assert lib.ac_lqg_workspace_floats(qd._handle, 0, n, C.byref(need)) == AC_ERR_UNSUPPORTED
    for est in ("ekf", "ukf"):
        rc, g = d_rollout(ac, gpu, t, est, "estimate", None, handle=qd._handle)
        assert rc == AC_ERR_UNSUPPORTED and all(bool((g[k].t == F_SENTINEL).all()) for k in OUT_F)
    o, lim, st = R.sense_opts(SENS), limits(), qd._stream()
    Z, M, U, e = Guarded((15, n), gpu), Guarded((n,), gpu), Guarded((13, n), gpu), Guarded((12, n), gpu)
    x, sr, sq = t["X0"].data_ptr(), t["sr"].data_ptr(), t["sq"].data_ptr()
    assert lib.ac_sense_f32(qd._handle, C.byref(o), 0, None, x, sr, n, Z.ptr(), M.ptr(), st) == AC_ERR_UNSUPPORTED
    assert lib.ac_disturb_f32(qd._handle, C.byref(o), 0, None, x, sq, n, U.ptr(), st) == AC_ERR_UNSUPPORTED
    assert lib.ac_policy_f32(qd._handle, C.byref(lim), x, x, t["Unom"].data_ptr(), t["Kx"].data_ptr(), n, U.ptr(), st) == AC_ERR_UNSUPPORTED
    assert lib.ac_estimate_score_f32(qd._handle, x, x, t["P0"].data_ptr(), n, e.ptr(), Z.ptr(), M.ptr(), st) == AC_ERR_UNSUPPORTED
    for g in checked(Z, M, U, e):
        assert bool((g.t == F_SENTINEL).all())
