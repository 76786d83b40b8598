"""GPU tests of the extended Kalman filter over the step sensitivities (ac_ekf_step_f32, ac_ekf_filter_f32, ac_ekf_measure_f32,
Aircraft.ekf / measure) against the float64 restatement tests/ekf_ref.py.

Instances: the trims of lqr_ref.grid as estimates with seeded covariances, truths and noisy measurements (ekf_ref.inputs),
cycled to the batch sizes SIZES, which straddle the 16-lane group (4 instances per wave), the wave and the workgroup.  Every
output and the workspace sit between guard words.

The bars (the protocol of tests/test_gpu_lqr.py).  e32 is the host build of the same header (g++, float32) against float64,
both from THE DEVICE'S OWN workspace x-, A, per instance and per output.  An instance is checked when its e32 is within 2 x
the recorded worst (ekf_ref.E32_WORST); at most 5 % of a batch's distinct instances may miss that.  The device is then held
to 8 x the worst e32 of the checked instances of its batch, measure by measure (ekf_ref.hold prints each figure first)."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import ekf_ref as E
from tests.test_gpu_lqr import Guarded, bits_equal, ws_layout

pytestmark = pytest.mark.gpu

CASES = [(m, n) for m in E.MODELS[:4] for n in E.SIZES] + [("net_4x128", 65)]
OUT_F = ("X", "P", "nu", "S", "nis", "ll")
OUT_I = ("used", "status")


def batch(name, n):
    """inputs(name) cycled to n columns, and the number of distinct instances"""
    d = dict(E.inputs(name))
    m = min(n, d["x"].shape[1])
    for k in ("x", "u", "P", "z", "Qd", "Rd"):
        d[k] = E.cycle(d[k], n)
    return d, m


def dev(a, gpu, dtype=None):
    import torch

    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32 if dtype == "i" else np.float32), device=gpu)


def run(ac, gpu, x, P, u, z, mask, Qd, Rd, predict=True, optional=True, dt=E.DT):
    """one ac_ekf_step_f32 call in guarded buffers -> dict of float64 / int arrays (and the float32 originals under *32), and
    the device tensors of the workspace parts"""
    import torch

    lib = ac._sync()
    n = x.shape[1]
    X, Pd, U, Z, Q, R = (dev(a, gpu) for a in (x, P, u, z, Qd, Rd))
    M = None if mask is None else dev(mask, gpu, "i")
    need = C.c_size_t()
    assert lib.ac_ekf_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(X=Guarded((13, n), gpu), P=Guarded((12, 12, n), gpu), nu=Guarded((15, n), gpu), S=Guarded((15, n), gpu),
             nis=Guarded((n,), gpu), ll=Guarded((n,), gpu), used=Guarded((n,), gpu, torch.int32), status=Guarded((n,), gpu, torch.int32),
             ws=Guarded((need.value,), gpu))
    if optional:
        g.update(Xpred=Guarded((13, n), gpu), Ppred=Guarded((12, 12, n), gpu), Abar=Guarded((12, 12, n), gpu))
    o = E.ekf_opts(E.MAG, predict)
    opt = [g[k].ptr() if optional else None for k in ("Xpred", "Ppred", "Abar")]
    rc = lib.ac_ekf_step_f32(ac._handle, C.byref(o), X.data_ptr(), Pd.data_ptr(), U.data_ptr(), C.c_float(dt), Z.data_ptr(),
                             None if M is None else M.data_ptr(), Q.data_ptr(), R.data_ptr(), n, g["X"].ptr(), g["P"].ptr(),
                             g["nu"].ptr(), g["S"].ptr(), g["nis"].ptr(), g["ll"].ptr(), g["used"].ptr(), g["status"].ptr(), *opt,
                             g["ws"].ptr(), need.value, ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    off, end = ws_layout(g["ws"].ptr(), n)
    assert end <= need.value
    w = g["ws"].t
    out = {k: v.np() for k, v in g.items() if k != "ws"}
    out["raw"] = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
    out["ws"] = (w[off[0]:off[0] + 13 * n].view(13, n), w[off[1]:off[1] + 169 * n].view(13, 13, n), w[off[2]:off[2] + 91 * n].view(13, 7, n))
    out["Xd"], out["Ud"] = X, U
    return out


def same_bits(a, b, keys=OUT_F + OUT_I, cols=slice(None)):
    for k in keys:
        assert np.array_equal(a["raw"][k][..., cols].view(np.int32), b["raw"][k][..., cols].view(np.int32)), k


def structure(out, n):
    """what holds for every call: P symmetric bit for bit"""
    P = out["raw"]["P"]
    assert np.array_equal(P.view(np.int32), P.transpose(1, 0, 2).view(np.int32)), "P is not bitwise symmetric"


def against_float64(name, d, m, out, mask, predict=True):
    """the bars of one step on the batch's distinct instances, from the device's own workspace"""
    u_ = slice(0, m)
    if predict:
        xp, A = (t.cpu().numpy().astype(np.float64)[..., u_] for t in out["ws"][:2])
    else:
        xp = A = None
    mk = None if mask is None else mask[u_]
    args = (d["x"][:, u_], d["P"][..., u_], xp, A, d["z"][:, u_], mk, d["Qd"][:, u_], d["Rd"][:, u_], E.MAG, d["eps"])
    ref, host = E.step(*args, predict_=predict), E.host_step(*args, predict_=predict)
    got = {k: out[k][..., u_] for k in OUT_F + ("Ppred", "Abar") if k in out}
    E.hold(name, E.errors(got, ref), E.errors(host, ref), m)
    assert np.array_equal(out["used"][u_], ref["used"]) and np.array_equal(out["status"][u_], ref["status"])
    return ref


# ---- 1. one step against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES, ids=[f"{m}-{n}" for m, n in CASES])
def test_step_against_float64(gpu, name, n):
    import torch

    d, m = batch(name, n)
    ac = d["ac"]
    args = (d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    out = run(ac, gpu, *args)
    structure(out, n)
    # -- the workspace holds the handle's own step sensitivities, bit for bit; Xpred is that x-
    Xn, A, Bm, _ = ac.step_sens(out["Xd"], out["Ud"], E.DT, want_c=False)
    for got, want in zip(out["ws"], (Xn, A, Bm)):
        assert torch.equal(got, want)
    assert bits_equal(out["raw"]["Xpred"], Xn.cpu().numpy())
    # -- without the optional outputs: the same bits elsewhere
    same_bits(out, run(ac, gpu, *args, optional=False))
    # -- a repeated instance gives the same bits wherever it sits in the batch
    first = np.arange(n) % m
    for k in OUT_F + OUT_I + ("Ppred", "Abar"):
        assert np.array_equal(out["raw"][k].view(np.int32), out["raw"][k][..., first].view(np.int32)), k
    ref = against_float64(f"{name} n={n}", d, m, out, None)
    assert (out["used"] == E.ALL).all() and (out["status"] == 0).all() and ref["S"].min() > 0


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(E.mask_cases(1)))
def test_rows(gpu, case):
    d, m = batch("poly", 65)
    mask = E.mask_cases(65)[case]
    out = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], mask, d["Qd"], d["Rd"])
    structure(out, 65)
    against_float64(f"rows {case}", d, m, out, mask)
    want = E.ALL if mask is None else mask
    assert (out["used"] == want).all() and (out["status"] == 0).all()
    unused = [i for i in range(15) if not (int(np.atleast_1d(want)[0]) >> i) & 1]
    assert (out["raw"]["nu"][unused] == 0).all() and (out["raw"]["S"][unused] == 0).all()
    if case == "none":  # pure prediction
        assert bits_equal(out["raw"]["X"], out["ws"][0].cpu().numpy()) and bits_equal(out["raw"]["P"], out["raw"]["Ppred"])
        assert (out["raw"]["nis"] == 0).all() and (out["raw"]["ll"] == 0).all()


def test_nan_row_is_a_cleared_mask_bit(gpu):
    d, m = batch("poly", 65)
    z = d["z"].copy()
    some = np.arange(65) % 3 == 1
    z[4, some] = np.nan
    z[13, some] = np.inf
    mask = np.full(65, E.ALL, np.int32)
    mask[some] &= ~((1 << 4) | (1 << 13))
    a = run(d["ac"], gpu, d["x"], d["P"], d["u"], z, None, d["Qd"], d["Rd"])
    b = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], mask, d["Qd"], d["Rd"])
    same_bits(a, b)
    assert np.array_equal(a["used"], mask) and (a["status"] == 0).all()
    assert np.isfinite(a["X"]).all() and np.isfinite(a["P"]).all() and np.isfinite(a["nu"]).all()


# ---- 3. the measurement function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.MODELS)
def test_measure(gpu, name):
    import torch

    d, m = batch(name, 65)
    ac = d["ac"]
    lib = ac._sync()
    x = E.cycle(E.measure_states(name), 65)
    X = dev(x, gpu)
    g = Guarded((15, 65), gpu)
    o = E.ekf_opts()
    assert lib.ac_ekf_measure_f32(ac._handle, C.byref(o), X.data_ptr(), 65, g.ptr(), ac._stream()) == 0
    torch.cuda.synchronize()
    g.check()
    Z = g.t.cpu().numpy()
    aero = torch.empty((22, 65), device=gpu)
    U = dev(d["u"], gpu)
    assert lib.ac_aero_f32(ac._handle, X.data_ptr(), U.data_ptr(), 65, aero.data_ptr(), ac._stream()) == 0
    assert bits_equal(Z[9:12], aero[3:6].cpu().numpy()), "air rows are ac_aero_f32's airspeed, alpha, beta bit for bit"
    assert bits_equal(Z[0:6], x[0:6]) and bits_equal(Z[6:9], x[10:13])
    want = E.h(x, E.MAG, d["eps"])
    e32 = E.L.unit_max_rel(E.host_measure(x, E.MAG, d["eps"])[12:15], want[12:15])
    err = E.L.unit_max_rel(Z[12:15].astype(np.float64), want[12:15])
    print(f"[ekf] measure {name}: magnetometer e32 {e32.max():.2e}, device {err.max():.2e}")
    assert (e32 <= 2 * E.E32_WORST["mag"]).all() and (err <= 8 * e32.max()).all()
    assert bits_equal(ac.measure(X, E.MAG).cpu().numpy(), Z)


# ---- 4. the measurement update alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_update_only(gpu, name):
    d, m = batch(name, 65)
    out = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"], predict=False)
    structure(out, 65)
    against_float64(f"update only {name}", d, m, out, None, predict=False)
    assert bits_equal(out["raw"]["Xpred"], d["x"]) and bits_equal(out["raw"]["Ppred"], d["P"])
    assert bits_equal(out["raw"]["Abar"], np.repeat(np.eye(12)[:, :, None], 65, axis=2))
    assert (out["ws"][0] == 12345.0).all(), "no sensitivity launch"


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(gpu):
    d, m = batch("poly", 257)
    big = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    for k in (0, 5, 41):
        c = slice(k, k + 1)
        one = run(d["ac"], gpu, d["x"][:, c], d["P"][..., c], d["u"][:, c], d["z"][:, c], None, d["Qd"][:, c], d["Rd"][:, c])
        for pos in (k, k + m, k + 5 * m):  # in a first group, mid-wave, in the last workgroups
            for key in OUT_F + OUT_I + ("Ppred", "Abar"):
                assert np.array_equal(one["raw"][key][..., 0].view(np.int32), big["raw"][key][..., pos].view(np.int32)), (key, k, pos)


# ---- 6. the filter ----------------------------------------------------------------------------------------------------------------------
def filter_call(ac, gpu, d, T, per_step=True):
    import torch

    lib = ac._sync()
    n = d["x"].shape[1]
    X, Pd, U, Z, Q, R = (dev(a, gpu) for a in (d["x"], d["P"], np.repeat(d["u"][None], T, axis=0), d["Z"], d["Qd"], d["Rd"]))
    M = dev(d["masks"], gpu, "i")
    need = C.c_size_t()
    assert lib.ac_ekf_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(Xo=Guarded((13, n), gpu), Po=Guarded((12, 12, n), gpu), ll=Guarded((n,), gpu), ws=Guarded((need.value,), gpu))
    if per_step:
        g.update(X=Guarded((T, 13, n), gpu), P=Guarded((T, 12, 12, n), gpu), nu=Guarded((T, 15, n), gpu), S=Guarded((T, 15, n), gpu),
                 nis=Guarded((T, n), gpu), used=Guarded((T, n), gpu, torch.int32), status=Guarded((T, n), gpu, torch.int32))
    o = E.ekf_opts()
    ps = [g[k].ptr() if per_step else None for k in ("X", "P", "nu", "S", "nis", "used", "status")]
    rc = lib.ac_ekf_filter_f32(ac._handle, C.byref(o), X.data_ptr(), Pd.data_ptr(), U.data_ptr(), C.c_float(E.DT), Z.data_ptr(),
                               M.data_ptr(), Q.data_ptr(), R.data_ptr(), n, T, g["Xo"].ptr(), g["Po"].ptr(), g["ll"].ptr(), *ps,
                               g["ws"].ptr(), need.value, ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    return {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}


def test_filter(gpu):
    T, n = E.CHAIN_T, 65
    d = E.chain_inputs("poly", n)
    m = min(n, E.chain_inputs("poly")["x"].shape[1])
    ac = d["ac"]
    f = filter_call(ac, gpu, d, T)
    # -- bit-equal to T calls of the step, ll summed in float32 in step order
    x, P, ll = d["x"], d["P"], None
    for t in range(T):
        o = run(ac, gpu, x, P, d["u"], d["Z"][t], d["masks"][t], d["Qd"], d["Rd"], optional=False)
        for k in ("X", "P", "nu", "S", "nis", "used", "status"):
            assert np.array_equal(o["raw"][k].view(np.int32), f[k][t].view(np.int32)), (k, t)
        ll = o["raw"]["ll"] if ll is None else (ll + o["raw"]["ll"]).astype(np.float32)
        x, P = o["raw"]["X"], o["raw"]["P"]
    assert bits_equal(ll, f["ll"]) and bits_equal(f["Xo"], f["X"][-1]) and bits_equal(f["Po"], f["P"][-1])
    assert np.array_equal(f["used"], d["masks"]) and (f["status"] == 0).all()
    # -- without the per-step outputs: the same final estimate
    g = filter_call(ac, gpu, d, T, per_step=False)
    for k in ("Xo", "Po", "ll"):
        assert bits_equal(f[k], g[k]), k
    # -- against the float64 chain; e32 over the host build's own chain (its steps and Jacobians from this handle)
    u_ = slice(0, m)
    args = (d["x"][:, u_], d["P"][..., u_], d["u"][:, u_], d["Z"][..., u_], d["masks"][:, u_], d["Qd"][:, u_], d["Rd"][:, u_], E.MAG, d["eps"])
    ref = E.chain(E.step, d["orc"].step_sens, *args)
    host = E.chain(E.host_step, lambda *a: ac.step_sens(*a), *args, host=True)
    got = {k: f[k][..., u_].astype(np.float64) for k in ("X", "P", "nu", "S", "nis", "ll")}
    E.hold("filter", E.chain_errors(got, ref), E.chain_errors(host, ref), m)


def test_step_graph_replay(gpu):
    import torch

    d, m = batch("poly", 65)
    ac = d["ac"]
    X, P, U, Z = (dev(d[k], gpu) for k in ("x", "P", "u", "z"))
    kw = dict(q=dev(d["Qd"], gpu), r=dev(d["Rd"], gpu), mag_ned=E.MAG)
    ref = ac.ekf(X, P, **kw).step(U, E.DT, Z)
    filt = ac.ekf(X, P, ws=ac.ekf_workspace(65), **kw)
    x0, P0 = filt._X, filt._P
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        filt.step(U, E.DT, Z)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    filt._X, filt._P = x0, P0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = filt.step(U, E.DT, Z)
    g.replay()
    torch.cuda.synchronize()
    for k in ("X", "P", "nu", "S", "nis", "ll", "used", "status"):
        assert torch.equal(getattr(ref, k), getattr(out, k)), k
    assert torch.equal(filt.x, out.X)


# ---- 7. status paths (finite inputs or planted NaNs: value paths, nothing here faults) -----------------------------------------------------
def test_status_paths(gpu):
    d, m = batch("poly", 65)
    clean = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"], predict=False)
    # an Rd row of 0 with a singular P row / column: s = 0 exactly, the row is rejected, the others are applied
    P, Rd = d["P"].copy(), d["Rd"].copy()
    rej = np.zeros(65, bool)
    rej[[2, 17, 64]] = True
    P[0][:, rej] = 0.0
    P[:, 0][:, rej] = 0.0
    Rd[0, rej] = 0.0
    out = run(d["ac"], gpu, d["x"], P, d["u"], d["z"], None, d["Qd"], Rd, predict=False)
    structure(out, 65)
    assert (out["status"][rej] == 1).all() and (out["status"][~rej] == 0).all() and (out["used"] == E.ALL).all()
    assert (out["S"][0, rej] == 0).all() and np.isfinite(out["X"]).all() and np.isfinite(out["P"]).all()
    same_bits(out, clean, cols=~rej)
    ref = E.step(d["x"], P, None, None, d["z"], None, d["Qd"], Rd, E.MAG, d["eps"], predict_=False)
    assert np.array_equal(ref["status"], out["status"])
    # a NaN state in some instances: bit 2, the prediction comes back, the others' bits are unchanged
    full = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    x = d["x"].copy()
    bad = np.zeros(65, bool)
    bad[[7, 20, 64]] = True
    x[4, 7], x[8, 20], x[11, 64] = np.nan, np.nan, np.inf
    out = run(d["ac"], gpu, x, d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    assert (out["status"][bad] == 2).all() and (out["status"][~bad] == 0).all() and (out["used"][bad] == 0).all()
    for k in ("nu", "S", "nis", "ll"):
        assert (out["raw"][k][..., bad] == 0).all(), k
    assert bits_equal(out["raw"]["X"][:, bad], out["ws"][0].cpu().numpy()[:, bad]) and not np.isfinite(out["X"][:, bad]).all(axis=0).any()
    same_bits(out, full, cols=~bad)


# ---- 8. the ABI and the Python surface -----------------------------------------------------------------------------------------------------
def test_ekf_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    d, m = batch("poly", 8)
    ac = d["ac"]
    ac._sync()
    n = 8
    X, P, U, Z, Q, R = (dev(d[k], gpu) for k in ("x", "P", "u", "z", "Qd", "Rd"))
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    zi = lambda *s: torch.zeros(s, device=gpu, dtype=torch.int32)  # noqa: E731
    Xo, Po, nu, S, nis, ll, used, st = z(13, n), z(12, 12, n), z(15, n), z(15, n), z(n), z(n), zi(n), zi(n)
    need = C.c_size_t()
    assert lib.ac_ekf_workspace_floats(ac._handle, n, C.byref(need)) == 0 and need.value >= n * 273
    ws = z(need.value)

    def call(h, predict=1, wsn=need.value, dt=E.DT, n_=n, x_ptr=X.data_ptr(), u_ptr=U.data_ptr(), st_ptr=st.data_ptr()):
        o = E.ekf_opts(E.MAG, predict)
        return lib.ac_ekf_step_f32(h, C.byref(o), x_ptr, P.data_ptr(), u_ptr, C.c_float(dt), Z.data_ptr(), None, Q.data_ptr(),
                                   R.data_ptr(), n_, Xo.data_ptr(), Po.data_ptr(), nu.data_ptr(), S.data_ptr(), nis.data_ptr(),
                                   ll.data_ptr(), used.data_ptr(), st_ptr, None, None, None, ws.data_ptr(), wsn, None)

    def filt(h, T, dt=E.DT, wsn=need.value, xo_ptr=Xo.data_ptr()):
        o = E.ekf_opts()
        Ut, Zt = U.unsqueeze(0).contiguous(), Z.unsqueeze(0).contiguous()
        return lib.ac_ekf_filter_f32(h, C.byref(o), X.data_ptr(), P.data_ptr(), Ut.data_ptr(), C.c_float(dt), Zt.data_ptr(), None,
                                     Q.data_ptr(), R.data_ptr(), n, T, xo_ptr, Po.data_ptr(), ll.data_ptr(), None, None, None, None,
                                     None, None, None, ws.data_ptr(), wsn, None)

    assert call(ac._handle) == 0
    torch.cuda.synchronize()
    assert (st == 0).all()
    assert call(ac._handle, wsn=need.value - 1) == -6 and b"workspace" in lib.ac_last_error()  # AC_ERR_WORKSPACE
    for bad_dt in (0.0, -0.01, float("nan"), float("inf")):
        assert call(ac._handle, dt=bad_dt) == -1 and b"dt" in lib.ac_last_error()  # AC_ERR_BAD_ARG
    assert call(ac._handle, predict=0, dt=0.0, u_ptr=None) == 0  # dt and U are not read without the time update
    assert call(ac._handle, n_=-1) == -1 and call(ac._handle, x_ptr=None) == -1 and call(ac._handle, u_ptr=None) == -1
    assert call(ac._handle, st_ptr=None) == -1
    assert call(ac._handle, n_=0) == 0
    assert filt(ac._handle, 0) == 0 and filt(ac._handle, 1) == 0 and filt(ac._handle, -1) == -1
    assert filt(ac._handle, 1, dt=0.0) == -1 and filt(ac._handle, 1, wsn=10) == -6 and filt(ac._handle, 1, xo_ptr=None) == -1
    o = E.ekf_opts()
    assert lib.ac_ekf_measure_f32(ac._handle, C.byref(o), None, n, Z.data_ptr(), None) == -1
    assert lib.ac_ekf_measure_f32(ac._handle, C.byref(o), X.data_ptr(), 0, Z.data_ptr(), None) == 0
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle) == -3 and filt(qd._handle, 1) == -3  # AC_ERR_UNSUPPORTED
    assert lib.ac_ekf_workspace_floats(qd._handle, n, C.byref(need)) == -3
    assert lib.ac_ekf_measure_f32(qd._handle, C.byref(o), X.data_ptr(), n, Z.data_ptr(), None) == -3
    torch.cuda.synchronize()


def test_python_surface(gpu):
    """Aircraft.ekf: numpy in, numpy out; step, update and filter give the ABI's bits; q and r broadcast; one instance as vectors"""
    T, n = 6, 5
    d = E.chain_inputs("poly", n, T_=T)
    ac = d["ac"]
    q, r = E.f32x(E.SIG_Q ** 2), E.f32x(E.SIG_R ** 2)
    f = filter_call(ac, gpu, d, T)
    a = ac.ekf(d["x"], d["P"], q=q, r=r, mag_ned=E.MAG)
    tr = a.filter(np.repeat(d["u"][None], T, axis=0), E.DT, d["Z"], d["masks"])
    assert tr.X.shape == (T, 13, n) and tr.P.shape == (T, 12, 12, n) and tr.nu.shape == (T, 15, n) and tr.ll.shape == (n,)
    assert tr.X.dtype == np.float64 and tr.used.dtype == np.int32
    for k in ("X", "P", "nu", "S", "nis", "ll", "used", "status"):
        assert np.array_equal(getattr(tr, k), f[k].astype(getattr(tr, k).dtype)), k
    assert np.array_equal(a.x, tr.X[-1]) and np.array_equal(a.P, tr.P[-1])
    b = ac.ekf(d["x"], d["P"], q=d["Qd"], r=d["Rd"], mag_ned=E.MAG)  # per instance
    for t in range(T):
        s = b.step(d["u"], E.DT, d["Z"][t], d["masks"][t])
        assert np.array_equal(s.X, tr.X[t]) and np.array_equal(s.P, tr.P[t]) and np.array_equal(s.nis, tr.nis[t])
    up = b.update(d["Z"][-1])
    assert up.X.shape == (13, n) and (up.used == E.ALL).all() and (np.diagonal(up.P) <= np.diagonal(tr.P[-1]) + 1e-12).all()
    one = ac.ekf(d["x"][:, 2], d["P"][:, :, 2], q=q, r=r, mag_ned=E.MAG).step(d["u"][:, 2], E.DT, d["Z"][0][:, 2], int(d["masks"][0][2]))
    assert one.X.shape == (13,) and one.P.shape == (12, 12) and np.array_equal(one.X, tr.X[0][:, 2]) and float(one.nis) == tr.nis[0][2]
    with pytest.raises(ValueError):
        a.step(d["u"], 0.0, d["Z"][0])
    with pytest.raises(ValueError):
        a.step(d["u"], E.DT, d["Z"][0][:14])
    with pytest.raises(ValueError):
        a.filter(np.zeros((T, 7, n)), E.DT, d["Z"], d["masks"][:2])
