"""GPU tests of the unscented Kalman filter beside the EKF bank (ac_ukf_step_f32, ac_ukf_filter_f32, ac_ukf_filter_rec_f32,
Aircraft.ukf) against the float64 restatement tests/ukf_ref.py, by the protocol of tests/test_gpu_ekf.py.

Instances: ekf_ref.inputs cycled to the batch sizes SIZES.  Every output and the workspace sit between guard words.
The bars.  e32 is the host build of the same header (g++, float32) against float64; the device, the host build and float64 all
read THE DEVICE'S OWN workspace (the images of its sigma points; the host build also its factor of P).  An instance is checked
when its e32 is within 2 x the recorded worst (ukf_ref.E32_WORST); at most 5 % of a batch's distinct instances may miss that.  The
device is then held to 8 x the worst e32 of the checked instances of its batch, measure by measure (ukf_ref.hold prints each
figure first).  The sigma points in the workspace are held to 8 x the host build's own e32 against float64."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import ekf_ref as E
from tests import rts_ref as R
from tests import ukf_ref as U
from tests.test_gpu_ekf import batch, dev
from tests.test_gpu_lqr import Guarded, bits_equal
from tests.test_gpu_rts import f64, smooth_call
from tests.test_gpu_rts import structure as rts_structure

pytestmark = pytest.mark.gpu

CASES = [(m, n) for m in E.MODELS[:4] for n in E.SIZES] + [("net_4x128", 65)]
OUT_F = ("X", "P", "nu", "S", "nis", "ll")
OUT_I = ("used", "status")
OPT = ("Xpred", "Ppred", "Abar")
SENTINEL = 12345.0


def ws_layout(addr, n):
    """float offsets of the points [13][25 n], U [7][25 n], the images [13][25 n], L [144][n], the flag [n] in the workspace: each
    on the next 256-byte boundary"""
    off, p = [], int(addr)
    for floats in (13 * U.PTS * n, 7 * U.PTS * n, 13 * U.PTS * n, 144 * n, n):
        p = (p + 255) & ~255
        off.append((p - addr) // 4)
        p += 4 * floats
    return off, (p - addr) // 4


def run(ac, gpu, x, P, u, z, mask, Qd, Rd, predict=True, optional=True, kappa=0.0, dt=E.DT):
    """one ac_ukf_step_f32 call in guarded buffers -> dict of float64 / int arrays (the originals under raw), and the device
    tensors of the workspace parts"""
    import torch

    lib = ac._sync()
    n = x.shape[1]
    X, Pd, Ut, Z, Q, Rr = (dev(a, gpu) for a in (x, P, u, z, Qd, Rd))
    M = None if mask is None else dev(mask, gpu, "i")
    need = C.c_size_t()
    assert lib.ac_ukf_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(X=Guarded((13, n), gpu), P=Guarded((12, 12, n), gpu), nu=Guarded((15, n), gpu), S=Guarded((15, n), gpu),
             nis=Guarded((n,), gpu), ll=Guarded((n,), gpu), used=Guarded((n,), gpu, torch.int32), status=Guarded((n,), gpu, torch.int32),
             ws=Guarded((need.value,), gpu))
    if optional:
        g.update(Xpred=Guarded((13, n), gpu), Ppred=Guarded((12, 12, n), gpu), Abar=Guarded((12, 12, n), gpu))
    o = U.ukf_opts(E.MAG, predict, kappa)
    opt = [g[k].ptr() if optional else None for k in OPT]
    rc = lib.ac_ukf_step_f32(ac._handle, C.byref(o), X.data_ptr(), Pd.data_ptr(), Ut.data_ptr(), C.c_float(dt), Z.data_ptr(),
                             None if M is None else M.data_ptr(), Q.data_ptr(), Rr.data_ptr(), n, g["X"].ptr(), g["P"].ptr(),
                             g["nu"].ptr(), g["S"].ptr(), g["nis"].ptr(), g["ll"].ptr(), g["used"].ptr(), g["status"].ptr(), *opt,
                             g["ws"].ptr(), need.value, ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    off, end = ws_layout(g["ws"].ptr(), n)
    assert end <= need.value
    w = g["ws"].t
    m25 = U.PTS * n
    out = {k: v.np() for k, v in g.items() if k != "ws"}
    out["raw"] = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
    out["ws"] = dict(pts=w[off[0]:off[0] + 13 * m25].view(13, m25), U=w[off[1]:off[1] + 7 * m25].view(7, m25),
                     F=w[off[2]:off[2] + 13 * m25].view(13, m25), L=w[off[3]:off[3] + 144 * n].view(144, n),
                     flag=w[off[4]:off[4] + n].view(torch.int32), all=w)
    return out


def dev_step(ac, gpu, pts, u25, dt=E.DT):
    """ac_step_f32 of the device tensors pts (13, m), u25 (7, m) -> tensor (13, m)"""
    import torch

    lib = ac._sync()
    out = torch.empty_like(pts)
    assert lib.ac_step_f32(ac._handle, pts.data_ptr(), u25.data_ptr(), C.c_float(dt), None, pts.shape[1], out.data_ptr(), ac._stream()) == 0
    torch.cuda.synchronize()
    return out


def same_bits(a, b, keys=OUT_F + OUT_I, cols=slice(None)):
    for k in keys:
        assert np.array_equal(a["raw"][k][..., cols].view(np.int32), b["raw"][k][..., cols].view(np.int32)), k


def structure(out):
    """what holds for every call: P and P- symmetric bit for bit"""
    for k in ("P", "Ppred"):
        if k in out["raw"]:
            P = out["raw"][k].view(np.int32)
            assert np.array_equal(P, P.transpose(1, 0, 2)), f"{k} is not bitwise symmetric"


def cols(t, n, m):
    """the columns of the first m instances of a workspace tensor (rows, 25 n) -> float64 (rows, 25, m)"""
    return t.cpu().numpy().astype(np.float64).reshape(t.shape[0], U.PTS, n)[:, :, :m]


def against_float64(name, d, m, out, mask, predict=True, kappa=0.0):
    """the bars of one step on the batch's distinct instances, from the device's own workspace"""
    n = d["x"].shape[1]
    u_ = slice(0, m)
    x, P, u = d["x"][:, u_], d["P"][..., u_], d["u"][:, u_]
    mk = None if mask is None else mask[u_]
    tail = (d["z"][:, u_], mk, d["Qd"][:, u_], d["Rd"][:, u_], kappa, E.MAG, d["eps"])
    if predict:
        s64, hs = U.sigma(x, P, kappa), U.host_sigma(x, P, u, kappa)
        pts = cols(out["ws"]["pts"], n, m)
        e_host, e_dev = U.err_sig(hs["pts"], s64["pts"]), U.err_sig(pts, s64["pts"])
        same = np.array_equal(pts, hs["pts"])
        print(f"[ukf] {name}: sigma points dev {e_dev.max():.2e} e32 {e_host.max():.2e}; bit-identical to the host build: {same}")
        assert (e_host <= 2 * U.E32_WORST["sig"]).all() and e_dev.max() <= 8 * e_host.max()
        F = cols(out["ws"]["F"], n, m)
        L32, flag = out["ws"]["L"].cpu().numpy()[:, u_], out["ws"]["flag"].cpu().numpy()[u_]
        ref = U.update(x, P, s64["L"], s64["ok"], F, *tail)
        host = U.host_update(x, P, L32, flag, F, *tail)
    else:
        ref = U.update(x, P, None, None, None, *tail, predict_=False)
        host = U.host_update(x, P, None, None, None, *tail, predict_=False)
    got = {k: out[k][..., u_] for k in OUT_F + ("Ppred", "Abar") if k in out}
    U.hold(name, E.errors(got, ref), E.errors(host, ref), m)
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
    structure(out)
    ws = out["ws"]
    # -- the workspace: U replicated, centred positions, the images are the handle's own step of the points, bit for bit
    assert torch.equal(ws["U"], dev(d["u"], gpu).repeat(1, U.PTS)) and (ws["pts"][0:3, :n] == 0).all() and (ws["flag"] == 0).all()
    assert torch.equal(ws["F"], dev_step(ac, gpu, ws["pts"].contiguous(), ws["U"].contiguous()))
    # -- without the optional outputs: the same bits elsewhere
    same_bits(out, run(ac, gpu, *args, optional=False))
    # -- a repeated instance gives the same bits wherever it sits in the batch
    first = np.arange(n) % m
    for k in OUT_F + OUT_I + OPT:
        assert np.array_equal(out["raw"][k].view(np.int32), out["raw"][k][..., first].view(np.int32)), k
    ref = against_float64(f"{name} n={n}", d, m, out, None)
    assert (out["used"] == E.ALL).all() and (out["status"] == 0).all() and ref["S"].min() > 0


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(E.mask_cases(1)))
def test_rows(gpu, case):
    d, m = batch("poly", 65)
    mask = E.mask_cases(65)[case]
    out = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], mask, d["Qd"], d["Rd"])
    structure(out)
    against_float64(f"rows {case}", d, m, out, mask)
    want = E.ALL if mask is None else mask
    assert (out["used"] == want).all() and (out["status"] == 0).all()
    unused = [i for i in range(15) if not (int(np.atleast_1d(want)[0]) >> i) & 1]
    assert (out["raw"]["nu"][unused] == 0).all() and (out["raw"]["S"][unused] == 0).all()
    if case == "none":  # pure prediction
        assert bits_equal(out["raw"]["X"], out["raw"]["Xpred"]) and bits_equal(out["raw"]["P"], out["raw"]["Ppred"])
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


# ---- 3. the measurement update alone, kappa ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_update_only(gpu, name):
    d, m = batch(name, 65)
    out = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"], predict=False)
    structure(out)
    against_float64(f"update only {name}", d, m, out, None, predict=False)
    assert bits_equal(out["raw"]["Xpred"], d["x"]) and bits_equal(out["raw"]["Ppred"], d["P"])
    assert bits_equal(out["raw"]["Abar"], np.repeat(np.eye(12)[:, :, None], 65, axis=2))
    assert (out["ws"]["all"] == SENTINEL).all(), "the workspace is untouched: neither k_ukf_sigma nor a step launch"


def test_kappa_3(gpu):
    d, m = batch("poly", 65)
    out = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"], kappa=3.0)
    structure(out)
    against_float64("kappa 3", d, m, out, None, kappa=3.0)
    zero = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    assert not bits_equal(out["raw"]["P"], zero["raw"]["P"])


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(gpu):
    d, m = batch("poly", 257)
    big = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    for k in (0, 5, 41):
        c = slice(k, k + 1)
        one = run(d["ac"], gpu, d["x"][:, c], d["P"][..., c], d["u"][:, c], d["z"][:, c], None, d["Qd"][:, c], d["Rd"][:, c])
        for pos in (k, k + m, k + 5 * m):  # in a first group, mid-wave, in the last workgroups
            for key in OUT_F + OUT_I + OPT:
                assert np.array_equal(one["raw"][key][..., 0].view(np.int32), big["raw"][key][..., pos].view(np.int32)), (key, k, pos)


# ---- 5. the filter and the smoother on its records -----------------------------------------------------------------------------------------
def filter_call(ac, gpu, d, T, record=True, per_step=True):
    import torch

    lib = ac._sync()
    n = d["x"].shape[1]
    X, Pd, Ut, Z, Q, Rr = (dev(a, gpu) for a in (d["x"], d["P"], np.repeat(d["u"][None], T, axis=0), d["Z"], d["Qd"], d["Rd"]))
    M = dev(d["masks"], gpu, "i")
    need = C.c_size_t()
    assert lib.ac_ukf_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(Xo=Guarded((13, n), gpu), Po=Guarded((12, 12, n), gpu), ll=Guarded((n,), gpu), ws=Guarded((need.value,), gpu))
    if per_step:
        g.update(X=Guarded((T, 13, n), gpu), P=Guarded((T, 12, 12, n), gpu), nu=Guarded((T, 15, n), gpu), S=Guarded((T, 15, n), gpu),
                 nis=Guarded((T, n), gpu), used=Guarded((T, n), gpu, torch.int32), status=Guarded((T, n), gpu, torch.int32))
    if record:
        g.update(Xpred=Guarded((T, 13, n), gpu), Ppred=Guarded((T, 12, 12, n), gpu), Abar=Guarded((T, 12, 12, n), gpu))
    o = U.ukf_opts()
    ptr = lambda k: g[k].ptr() if k in g else None  # noqa: E731
    head = (ac._handle, C.byref(o), X.data_ptr(), Pd.data_ptr(), Ut.data_ptr(), C.c_float(E.DT), Z.data_ptr(), M.data_ptr(), Q.data_ptr(),
            Rr.data_ptr(), n, T, *(ptr(k) for k in ("Xo", "Po", "ll", "X", "P", "nu", "S", "nis", "used", "status")))
    tail = (g["ws"].ptr(), need.value, ac._stream())
    if record:
        rc = lib.ac_ukf_filter_rec_f32(*head, *(ptr(k) for k in OPT), *tail)
    else:
        rc = lib.ac_ukf_filter_f32(*head, *tail)
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    out = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
    out["X0"], out["P0"] = np.ascontiguousarray(d["x"], dtype=np.float32), np.ascontiguousarray(d["P"], dtype=np.float32)
    return out


def test_filter_and_smoother(gpu):
    import torch

    T, n = E.CHAIN_T, 65
    d = E.chain_inputs("poly", n)
    m = min(n, E.chain_inputs("poly")["x"].shape[1])
    ac, orc = d["ac"], d["orc"]
    f = filter_call(ac, gpu, d, T)
    # -- bit-equal to T calls of the step (the records: their optional outputs), ll summed in float32 in step order
    x, P, ll = d["x"], d["P"], None
    for t in range(T):
        o = run(ac, gpu, x, P, d["u"], d["Z"][t], d["masks"][t], d["Qd"], d["Rd"])
        for k in ("X", "P", "nu", "S", "nis", "used", "status") + OPT:
            assert np.array_equal(o["raw"][k].view(np.int32), f[k][t].view(np.int32)), (k, t)
        ll = o["raw"]["ll"] if ll is None else (ll + o["raw"]["ll"]).astype(np.float32)
        x, P = o["raw"]["X"], o["raw"]["P"]
    assert bits_equal(ll, f["ll"]) and bits_equal(f["Xo"], f["X"][-1]) and bits_equal(f["Po"], f["P"][-1])
    assert np.array_equal(f["used"], d["masks"]) and (f["status"] == 0).all()
    # -- without the records, and without the per-step outputs: the same bits elsewhere
    g = filter_call(ac, gpu, d, T, record=False)
    for k in ("Xo", "Po", "ll", "X", "P", "nu", "S", "nis", "used", "status"):
        assert np.array_equal(f[k].view(np.int32), g[k].view(np.int32)), k
    g = filter_call(ac, gpu, d, T, record=False, per_step=False)
    for k in ("Xo", "Po", "ll"):
        assert bits_equal(f[k], g[k]), k
    # -- against the float64 chain; e32 over the host build's own chain (the images of its points from this handle)
    u_ = slice(0, m)
    Qd, Rd, eps = d["Qd"][:, u_], d["Rd"][:, u_], d["eps"]

    def ref_one(x_, P_, u_, z_, mask_, ll_):
        return U.step(orc.state_update, x_, P_, u_, z_, mask_, Qd, Rd, 0.0, E.MAG, eps)

    def host_one(x_, P_, u_, z_, mask_, ll_):
        s = U.host_sigma(x_, P_, u_)
        F = dev_step(ac, gpu, torch.tensor(s["pts32"], device=gpu), torch.tensor(s["U32"], device=gpu))
        return U.host_update(x_, P_, s["L32"], s["flag"], F.cpu().numpy().astype(np.float64).reshape(13, U.PTS, m), z_, mask_, Qd, Rd,
                             0.0, E.MAG, eps, ll_in=ll_)

    args = (d["x"][:, u_], d["P"][..., u_], d["u"][:, u_], d["Z"][..., u_], d["masks"][:, u_])
    ref, host = U.chain(ref_one, *args), U.chain(host_one, *args, host=True)
    got = {k: f[k][..., u_].astype(np.float64) for k in ("X", "P", "nu", "S", "nis", "ll")}
    U.hold("filter", E.chain_errors(got, ref), E.chain_errors(host, ref), m)
    # -- ac_ekf_smooth_f32 on the device's UKF records, by tests/test_gpu_rts.py's protocol
    r64 = f64({k: f[k] for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")}, m)
    sargs = [r64[k] for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")]
    sref, shost = R.smooth(*sargs), R.host_smooth(*sargs)
    out = smooth_call(ac, gpu, f, True, True)
    rts_structure(out, f)
    assert (out["status"] == 0).all() and np.array_equal(out["status"][:, :m], sref["status"])
    R.hold("smoother on the UKF records", R.errors(f64(out, m), sref, r64, True), R.errors(shost, sref, r64, True), m)


def test_step_graph_replay(gpu):
    import torch

    d, m = batch("poly", 65)
    ac = d["ac"]
    X, P, Ut, Z = (dev(d[k], gpu) for k in ("x", "P", "u", "z"))
    kw = dict(q=dev(d["Qd"], gpu), r=dev(d["Rd"], gpu), mag_ned=E.MAG)
    ref = ac.ukf(X, P, **kw).step(Ut, E.DT, Z)
    filt = ac.ukf(X, P, ws=ac.ukf_workspace(65), **kw)
    x0, P0 = filt._X, filt._P
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        filt.step(Ut, E.DT, Z)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    filt._X, filt._P = x0, P0
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = filt.step(Ut, E.DT, Z)
    g.replay()
    torch.cuda.synchronize()
    for k in ("X", "P", "nu", "S", "nis", "ll", "used", "status"):
        assert torch.equal(getattr(ref, k), getattr(out, k)), k
    assert torch.equal(filt.x, out.X)


# ---- 6. status paths (finite inputs or planted values: value paths, nothing here faults) ---------------------------------------------------
def test_status_paths(gpu):
    d, m = batch("poly", 65)
    clean = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"], predict=False)
    # a coordinate with a variance of 1e-36, uncorrelated, measured without noise: the sigma points do not move it in float32, its
    # pivot of Pzz is exactly 0: the row is rejected, the others are applied
    P, Rd = d["P"].copy(), d["Rd"].copy()
    rej = np.zeros(65, bool)
    rej[[2, 17, 64]] = True
    assert (np.abs(d["x"][3, rej]) > 1.0).all()
    P[3][:, rej] = 0.0
    P[:, 3][:, rej] = 0.0
    P[3, 3, rej] = 1e-36
    Rd[3, rej] = 0.0
    out = run(d["ac"], gpu, d["x"], P, d["u"], d["z"], None, d["Qd"], Rd, predict=False)
    structure(out)
    assert (out["status"][rej] == 1).all() and (out["status"][~rej] == 0).all() and (out["used"] == E.ALL).all()
    assert (out["S"][3, rej] == 0).all() and np.isfinite(out["X"]).all() and np.isfinite(out["P"]).all()
    same_bits(out, clean, cols=~rej)
    ref = U.update(d["x"], E.f32x(P), None, None, None, d["z"], None, d["Qd"], Rd, 0.0, E.MAG, d["eps"], predict_=False)
    assert np.array_equal(ref["status"], out["status"])
    # a NaN state in some instances: bit 2, the prediction comes back; a P without a factor in others: value 4, 25 copies of x^ in
    # the workspace, X and P come back unchanged; the others' bits are unchanged
    full = run(d["ac"], gpu, d["x"], d["P"], d["u"], d["z"], None, d["Qd"], d["Rd"])
    x, P = d["x"].copy(), d["P"].copy()
    bad, sing = np.zeros(65, bool), np.zeros(65, bool)
    bad[[7, 20, 64]] = True
    sing[[3, 33]] = True
    x[4, 7], x[8, 20], x[11, 64] = np.nan, np.nan, np.inf
    P[5][:, sing] = 0.0
    P[:, 5][:, sing] = 0.0
    out = run(d["ac"], gpu, x, P, d["u"], d["z"], None, d["Qd"], d["Rd"])
    assert (out["status"][bad] == 2).all() and (out["status"][sing] == 4).all() and (out["status"][~(bad | sing)] == 0).all()
    assert (out["used"][bad | sing] == 0).all()
    for k in ("nu", "S", "nis", "ll"):
        assert (out["raw"][k][..., bad | sing] == 0).all(), k
    assert bits_equal(out["raw"]["X"][:, bad], out["raw"]["Xpred"][:, bad]) and not np.isfinite(out["X"][:, bad]).all(axis=0).any()
    assert bits_equal(out["raw"]["X"][:, sing], x[:, sing]) and bits_equal(out["raw"]["P"][..., sing], P[..., sing])
    assert bits_equal(out["raw"]["Abar"][..., sing], np.repeat(np.eye(12)[:, :, None], 2, axis=2))
    pts = out["ws"]["pts"].cpu().numpy().reshape(13, U.PTS, 65)
    centre = np.ascontiguousarray(x, dtype=np.float32)[:, sing].copy()
    centre[0:3] = 0.0
    assert all(bits_equal(pts[:, j][:, sing], centre) for j in range(U.PTS)) and (out["ws"]["flag"].cpu().numpy() == sing).all()
    same_bits(out, full, cols=~(bad | sing))


# ---- 7. the ABI and the Python surface -----------------------------------------------------------------------------------------------------
def test_ukf_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    d, m = batch("poly", 8)
    ac = d["ac"]
    ac._sync()
    n = 8
    X, P, Ut, Z, Q, Rr = (dev(d[k], gpu) for k in ("x", "P", "u", "z", "Qd", "Rd"))
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    zi = lambda *s: torch.zeros(s, device=gpu, dtype=torch.int32)  # noqa: E731
    Xo, Po, nu, S, nis, ll, used, st = z(13, n), z(12, 12, n), z(15, n), z(15, n), z(n), z(n), zi(n), zi(n)
    need = C.c_size_t()
    assert lib.ac_ukf_workspace_floats(ac._handle, n, C.byref(need)) == 0 and need.value >= n * 25 * 33
    ws = z(need.value)

    def call(h, predict=1, wsn=need.value, dt=E.DT, n_=n, x_ptr=X.data_ptr(), u_ptr=Ut.data_ptr(), st_ptr=st.data_ptr(), kappa=0.0):
        o = U.ukf_opts(E.MAG, predict, kappa)
        return lib.ac_ukf_step_f32(h, C.byref(o), x_ptr, P.data_ptr(), u_ptr, C.c_float(dt), Z.data_ptr(), None, Q.data_ptr(),
                                   Rr.data_ptr(), n_, Xo.data_ptr(), Po.data_ptr(), nu.data_ptr(), S.data_ptr(), nis.data_ptr(),
                                   ll.data_ptr(), used.data_ptr(), st_ptr, None, None, None, ws.data_ptr(), wsn, None)

    def filt(h, T, dt=E.DT, wsn=need.value, xo_ptr=Xo.data_ptr(), rec=False, kappa=0.0):
        o = U.ukf_opts(kappa=kappa)
        Ut_, Zt = Ut.unsqueeze(0).contiguous(), Z.unsqueeze(0).contiguous()
        head = (h, C.byref(o), X.data_ptr(), P.data_ptr(), Ut_.data_ptr(), C.c_float(dt), Zt.data_ptr(), None, Q.data_ptr(), Rr.data_ptr(),
                n, T, xo_ptr, Po.data_ptr(), ll.data_ptr(), None, None, None, None, None, None, None)
        if rec:
            return lib.ac_ukf_filter_rec_f32(*head, None, None, None, ws.data_ptr(), wsn, None)
        return lib.ac_ukf_filter_f32(*head, ws.data_ptr(), wsn, None)

    assert call(ac._handle) == 0
    torch.cuda.synchronize()
    assert (st == 0).all()
    assert call(ac._handle, wsn=need.value - 1) == -6 and b"workspace" in lib.ac_last_error()  # AC_ERR_WORKSPACE
    for bad_dt in (0.0, -0.01, float("nan"), float("inf")):
        assert call(ac._handle, dt=bad_dt) == -1 and b"dt" in lib.ac_last_error()  # AC_ERR_BAD_ARG
    for bad_kappa in (-1.0, float("nan"), float("inf")):
        assert call(ac._handle, kappa=bad_kappa) == -1 and b"kappa" in lib.ac_last_error()
        assert filt(ac._handle, 1, kappa=bad_kappa) == -1
    assert call(ac._handle, predict=0, dt=0.0, u_ptr=None) == 0  # dt and U are not read without the time update
    assert call(ac._handle, n_=-1) == -1 and call(ac._handle, x_ptr=None) == -1 and call(ac._handle, u_ptr=None) == -1
    assert call(ac._handle, st_ptr=None) == -1
    assert call(ac._handle, n_=0) == 0 and call(ac._handle, kappa=3.0) == 0
    for rec in (False, True):
        assert filt(ac._handle, 0, rec=rec) == 0 and filt(ac._handle, 1, rec=rec) == 0 and filt(ac._handle, -1, rec=rec) == -1
        assert filt(ac._handle, 1, dt=0.0, rec=rec) == -1 and filt(ac._handle, 1, wsn=10, rec=rec) == -6
        assert filt(ac._handle, 1, xo_ptr=None, rec=rec) == -1
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle) == -3 and filt(qd._handle, 1) == -3 and filt(qd._handle, 1, rec=True) == -3  # AC_ERR_UNSUPPORTED
    assert lib.ac_ukf_workspace_floats(qd._handle, n, C.byref(need)) == -3
    torch.cuda.synchronize()


def test_python_surface(gpu):
    """Aircraft.ukf: numpy in, numpy out; step, update, filter and smooth give the ABI's bits; noise_stats / fit_noise raise"""
    from aircraft_amd import UKF

    T, n = 6, 5
    d = E.chain_inputs("poly", n, T_=T)
    ac = d["ac"]
    q, r = E.f32x(E.SIG_Q ** 2), E.f32x(E.SIG_R ** 2)
    f = filter_call(ac, gpu, d, T)
    a = ac.ukf(d["x"], d["P"], q=q, r=r, mag_ned=E.MAG)
    assert isinstance(a, UKF) and a.kappa == 0.0
    Us = np.repeat(d["u"][None], T, axis=0)
    tr = a.filter(Us, E.DT, d["Z"], d["masks"], record=True)
    assert tr.X.shape == (T, 13, n) and tr.P.shape == (T, 12, 12, n) and tr.Abar.shape == (T, 12, 12, n) and tr.ll.shape == (n,)
    for k in ("X", "P", "nu", "S", "nis", "ll", "used", "status", "Xpred", "Ppred", "Abar"):
        assert np.array_equal(getattr(tr, k), f[k].astype(getattr(tr, k).dtype)), k
    assert np.array_equal(a.x, tr.X[-1]) and np.array_equal(a.P, tr.P[-1])
    sm = a.smooth(tr, gains=True)
    want = smooth_call(ac, gpu, f, True, True)
    for k in ("X", "P", "X0", "P0", "C", "status"):
        assert np.array_equal(getattr(sm, k), want[k].astype(getattr(sm, k).dtype)), k
    b = ac.ukf(d["x"], d["P"], q=d["Qd"], r=d["Rd"], mag_ned=E.MAG)  # per instance
    for t in range(T):
        s = b.step(d["u"], E.DT, d["Z"][t], d["masks"][t])
        assert np.array_equal(s.X, tr.X[t]) and np.array_equal(s.P, tr.P[t]) and np.array_equal(s.nis, tr.nis[t])
    up = b.update(d["Z"][-1])
    assert up.X.shape == (13, n) and (up.used == E.ALL).all() and (np.diagonal(up.P) <= np.diagonal(tr.P[-1]) + 1e-12).all()
    k3 = ac.ukf(d["x"], d["P"], q=q, r=r, kappa=3.0, mag_ned=E.MAG).step(d["u"], E.DT, d["Z"][0], d["masks"][0])
    o3 = run(ac, gpu, d["x"], d["P"], d["u"], d["Z"][0], d["masks"][0], d["Qd"], d["Rd"], kappa=3.0)
    assert np.array_equal(k3.X, o3["X"]) and np.array_equal(k3.P, o3["P"])
    with pytest.raises(NotImplementedError):
        a.noise_stats(tr, sm, d["Z"])
    with pytest.raises(NotImplementedError):
        a.fit_noise(Us, E.DT, d["Z"])
    with pytest.raises(ValueError):
        a.step(d["u"], 0.0, d["Z"][0])
