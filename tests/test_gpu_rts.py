"""GPU tests of the RTS smoother over the EKF trace (ac_ekf_filter_rec_f32, ac_ekf_smooth_f32, EKF.filter(record=True),
EKF.smooth) against the float64 restatement tests/rts_ref.py.

Instances: the filter chains of ekf_ref.chain_inputs (trims as estimates, seeded covariances, simulated measurements, GPS
every fifth step), cycled to the batch sizes.  The shapes (n, T) cover T = 1 (a copy), the two shortest load-ahead pipelines,
a partial last workgroup and a partial wave.  Every output sits between guard words.

The bars (the protocol of tests/test_gpu_ekf.py).  The device smoother, the float32 host build of the same header and the
float64 restatement all read THE DEVICE'S OWN records from ac_ekf_filter_rec_f32.  e32 is host against float64 per instance and
measure; an instance is checked when its e32 is within 2 x the recorded worst (rts_ref.E32_WORST); at most 5 % of a batch's
distinct instances may miss that.  The device is then held to 8 x the worst e32 of the checked instances of its batch,
measure by measure (rts_ref.hold prints each figure first).  Status must be equal."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import ekf_ref as E
from tests import rts_ref as R
from tests.test_gpu_lqr import Guarded, bits_equal

pytestmark = pytest.mark.gpu

MODELS = ("poly", "default", "real_net")
SHAPES = ((1, 1), (1, 2), (5, 3), (17, 20), (257, 20))
REC = ("X", "P", "Xpred", "Ppred", "Abar")
OUT = ("X", "P", "X0", "P0", "C", "status")


def dev(a, gpu, dtype=None):
    import torch

    return torch.tensor(np.ascontiguousarray(a, dtype=np.int32 if dtype == "i" else np.float32), device=gpu)


_CHAINS = {}


def chain(name, n, T):
    """chain_inputs(name) with T steps (computed once) cycled to n columns, and the number of distinct instances"""
    if (name, T) not in _CHAINS:
        _CHAINS[name, T] = E.chain_inputs(name, T_=T)
    d = dict(_CHAINS[name, T])
    m = d["x"].shape[1]
    for k in ("x", "u", "P", "z", "Qd", "Rd", "truth", "Z", "masks"):
        d[k] = E.cycle(d[k], n)
    return d, min(n, m)


def filter_call(ac, gpu, d, T, record=True, x=None):
    """one ac_ekf_filter_rec_f32 (record) or ac_ekf_filter_f32 call in guarded buffers -> dict of the raw float32 / int32 arrays"""
    import torch

    lib = ac._sync()
    x = d["x"] if x is None else x
    n = x.shape[1]
    X, Pd, U, Z, Q, Rr = (dev(a, gpu) for a in (x, d["P"], np.repeat(d["u"][None], T, axis=0), d["Z"], d["Qd"], d["Rd"]))
    M = dev(d["masks"], gpu, "i")
    need = C.c_size_t()
    assert lib.ac_ekf_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(Xo=Guarded((13, n), gpu), Po=Guarded((12, 12, n), gpu), ll=Guarded((n,), gpu), X=Guarded((T, 13, n), gpu),
             P=Guarded((T, 12, 12, n), gpu), nu=Guarded((T, 15, n), gpu), S=Guarded((T, 15, n), gpu), nis=Guarded((T, n), gpu),
             used=Guarded((T, n), gpu, torch.int32), status=Guarded((T, n), gpu, torch.int32), ws=Guarded((need.value,), gpu))
    if record:
        g.update(Xpred=Guarded((T, 13, n), gpu), Ppred=Guarded((T, 12, 12, n), gpu), Abar=Guarded((T, 12, 12, n), gpu))
    o = E.ekf_opts()
    head = (ac._handle, C.byref(o), X.data_ptr(), Pd.data_ptr(), U.data_ptr(), C.c_float(E.DT), Z.data_ptr(), M.data_ptr(), Q.data_ptr(),
            Rr.data_ptr(), n, T, *(g[k].ptr() for k in ("Xo", "Po", "ll", "X", "P", "nu", "S", "nis", "used", "status")))
    tail = (g["ws"].ptr(), need.value, ac._stream())
    if record:
        rc = lib.ac_ekf_filter_rec_f32(*head, *(g[k].ptr() for k in ("Xpred", "Ppred", "Abar")), *tail)
    else:
        rc = lib.ac_ekf_filter_f32(*head, *tail)
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    out = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
    out["X0"], out["P0"] = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(d["P"], dtype=np.float32)
    return out


def smooth_call(ac, gpu, rec, initial=True, gains=True):
    """one ac_ekf_smooth_f32 call on the records `rec` (dict of float32 arrays) in guarded buffers -> dict of the raw arrays"""
    import torch

    lib = ac._sync()
    T, n = rec["X"].shape[0], rec["X"].shape[2]
    a = [dev(rec[k], gpu) if initial else None for k in ("X0", "P0")] + [dev(rec[k], gpu) for k in REC]
    g = dict(X=Guarded((T, 13, n), gpu), P=Guarded((T, 12, 12, n), gpu), status=Guarded((T, n), gpu, torch.int32))
    if initial:
        g.update(X0=Guarded((13, n), gpu), P0=Guarded((12, 12, n), gpu))
    if gains:
        g.update(C=Guarded((T, 12, 12, n), gpu))
    ptr = lambda k: g[k].ptr() if k in g else None  # noqa: E731
    rc = lib.ac_ekf_smooth_f32(ac._handle, *(None if t is None else t.data_ptr() for t in a), n, T, ptr("X"), ptr("P"), ptr("X0"),
                               ptr("P0"), ptr("C"), ptr("status"), ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    out = {k: None for k in OUT}
    out.update({k: v.t.cpu().numpy() for k, v in g.items()})
    return out


def same_bits(a, b, keys=OUT, cols=slice(None)):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k][..., cols].view(np.int32), b[k][..., cols].view(np.int32)), k


def f64(d, m=None):
    return {k: None if v is None else (v.astype(np.float64) if v.dtype == np.float32 else v)[..., :m] for k, v in d.items()}


def structure(out, rec):
    """what holds for every call: P^s symmetric bit for bit, the last node the filtered one bit for bit"""
    P = out["P"].view(np.int32)
    assert np.array_equal(P, P.transpose(0, 2, 1, 3)), "P^s is not bitwise symmetric"
    if out["P0"] is not None:
        assert np.array_equal(out["P0"].view(np.int32), out["P0"].view(np.int32).transpose(1, 0, 2))
    assert bits_equal(out["X"][-1], rec["X"][-1]) and bits_equal(out["P"][-1], rec["P"][-1])


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", SHAPES, ids=[f"n{n}-T{T}" for n, T in SHAPES])
@pytest.mark.parametrize("name", MODELS)
def test_smoother_against_float64(gpu, name, n, T):
    d, m = chain(name, n, T)
    ac = d["ac"]
    rec = filter_call(ac, gpu, d, T)
    assert (rec["status"] == 0).all()
    r64 = f64({k: rec[k] for k in REC + ("X0", "P0")}, m)
    first = np.arange(n) % m
    full = None
    for initial in (True, False):
        args = [r64[k] for k in REC] + ([r64["X0"], r64["P0"]] if initial else [])
        ref, host = R.smooth(*args), R.host_smooth(*args)
        for gains in (True, False):
            out = smooth_call(ac, gpu, rec, initial, gains)
            structure(out, rec)
            if gains:
                full = out
                if not initial:
                    assert (out["C"][0] == 0).all()
            else:
                same_bits(out, full, keys=("X", "P", "X0", "P0", "status"))  # without the gains: the same bits elsewhere
            # a repeated instance gives the same bits wherever it sits in the batch
            for k in OUT:
                if out[k] is not None:
                    assert np.array_equal(out[k].view(np.int32), out[k][..., first].view(np.int32)), k
            assert np.array_equal(out["status"][:, :m], ref["status"]) and np.array_equal(host["status"], ref["status"])
            assert (out["status"] == 0).all()
            got = f64(out, m)
            R.hold(f"{name} n={n} T={T} initial={initial} gains={gains}", R.errors(got, ref, r64, initial),
                   R.errors(host if gains else {k: host[k] for k in ("X", "P", "X0", "P0")}, ref, r64, initial), m)


# ---- 2. the records ---------------------------------------------------------------------------------------------------------------------
def test_records_are_the_steps_optional_outputs(gpu):
    from tests.test_gpu_ekf import run

    n, T = 17, 6
    d, m = chain("poly", n, T)
    ac = d["ac"]
    rec, plain = filter_call(ac, gpu, d, T), filter_call(ac, gpu, d, T, record=False)
    for k in ("Xo", "Po", "ll", "X", "P", "nu", "S", "nis", "used", "status"):
        assert np.array_equal(rec[k].view(np.int32), plain[k].view(np.int32)), k
    x, P = d["x"], d["P"]
    for t in range(T):
        o = run(ac, gpu, x, P, d["u"], d["Z"][t], d["masks"][t], d["Qd"], d["Rd"])
        for k in ("Xpred", "Ppred", "Abar"):
            assert np.array_equal(o["raw"][k].view(np.int32), rec[k][t].view(np.int32)), (k, t)
        x, P = o["raw"]["X"], o["raw"]["P"]


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(gpu):
    n, T = 257, 20
    d, m = chain("poly", n, T)
    ac = d["ac"]
    rec = filter_call(ac, gpu, d, T)
    big = smooth_call(ac, gpu, rec)
    for k in (0, 5, 41 % m):
        one = smooth_call(ac, gpu, {key: np.ascontiguousarray(v[..., k:k + 1]) for key, v in rec.items()})
        for pos in (k, k + m, k + 5 * m):  # in a first group, mid-wave, in the last workgroups
            for key in OUT:
                assert np.array_equal(one[key][..., 0].view(np.int32), big[key][..., pos].view(np.int32)), (key, k, pos)


# ---- 4. status paths (finite inputs or planted NaNs: value paths, nothing here faults) ---------------------------------------------------
def test_status_paths(gpu):
    n, T = 17, 20
    d, m = chain("poly", n, T)
    ac = d["ac"]
    clean_rec = filter_call(ac, gpu, d, T)
    clean = smooth_call(ac, gpu, clean_rec)
    rec = {k: v.copy() for k, v in clean_rec.items()}
    rec["Ppred"][12][:, :, 3] *= -1.0            # not positive definite: link 12 of instance 3
    rec["Abar"][7][3, 4, 16] = np.nan            # a NaN record: link 7 of instance 16 (the last one)
    rec["Ppred"][5][2, 2, 9] = 0.0               # a zero pivot: link 5 of instance 9
    out = smooth_call(ac, gpu, rec)
    want = np.zeros((T, n), np.int32)
    want[12, 3], want[7, 16], want[5, 9] = R.NOT_PD, R.NONFINITE, R.NOT_PD
    assert np.array_equal(out["status"], want)
    r64 = f64({k: rec[k] for k in REC + ("X0", "P0")})
    ref = R.smooth(*[r64[k] for k in REC], r64["X0"], r64["P0"])
    assert np.array_equal(ref["status"], want)
    for k, i in ((12, 3), (7, 16), (5, 9)):
        assert bits_equal(out["X"][k - 1][:, i], rec["X"][k - 1][:, i]) and bits_equal(out["P"][k - 1][:, :, i], rec["P"][k - 1][:, :, i])
        assert (out["C"][k][:, :, i] == 0).all() and (out["C"][k - 1][:, :, i] != 0).any()
        assert not bits_equal(out["P"][k - 2][:, :, i], rec["P"][k - 2][:, :, i])  # smoothed again further back
        assert bits_equal(out["P"][k:, :, :, i], clean["P"][k:, :, :, i])            # and untouched after the link
    assert np.isfinite(out["X"]).all() and np.isfinite(out["P"]).all() and np.isfinite(out["C"]).all()
    others = np.ones(n, bool)
    others[[3, 16, 9]] = False
    same_bits(out, clean, cols=others)
    got = f64(out)
    e = R.errors({k: got[k] for k in ("X", "P", "X0", "P0")}, ref, r64, True)
    host = R.host_smooth(*[r64[k] for k in REC], r64["X0"], r64["P0"])
    R.hold("status paths", e, R.errors({k: host[k] for k in ("X", "P", "X0", "P0")}, ref, r64, True), m)
    # a filter whose prediction was not finite (its status bit 2 at every step): every link reports its operands, the nodes
    # are the filtered ones bit for bit, and the neighbours are untouched
    x = d["x"].copy()
    x[4, 6] = np.nan
    bad_rec = filter_call(ac, gpu, d, T, x=x)
    assert (bad_rec["status"][:, 6] == 2).all() and (np.delete(bad_rec["status"], 6, axis=1) == 0).all()
    out = smooth_call(ac, gpu, bad_rec)
    assert (out["status"][:, 6] == R.NONFINITE).all() and (np.delete(out["status"], 6, axis=1) == 0).all()
    assert bits_equal(out["X"][..., 6], bad_rec["X"][..., 6]) and bits_equal(out["P"][..., 6], bad_rec["P"][..., 6])
    assert bits_equal(out["X0"][:, 6], bad_rec["X0"][:, 6]) and bits_equal(out["P0"][..., 6], bad_rec["P0"][..., 6])
    assert (out["C"][..., 6] == 0).all()
    others = np.arange(n) != 6
    same_bits(out, clean, cols=others)


# ---- 5. the ABI and the Python surface -----------------------------------------------------------------------------------------------------
def test_smooth_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    n, T = 8, 3
    d, m = chain("poly", n, T)
    ac = d["ac"]
    rec = filter_call(ac, gpu, d, T)
    t = {k: dev(rec[k], gpu) for k in REC + ("X0", "P0")}
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    o = dict(Xs=z(T, 13, n), Ps=z(T, 12, 12, n), Xs0=z(13, n), Ps0=z(12, 12, n), Cg=z(T, 12, 12, n),
             status=torch.full((T, n), -1, device=gpu, dtype=torch.int32))

    def call(h, n_=n, T_=T, **kw):
        p = {k: v.data_ptr() for k, v in {**t, **o}.items()}
        p.update(kw)
        return lib.ac_ekf_smooth_f32(h, p["X0"], p["P0"], p["X"], p["P"], p["Xpred"], p["Ppred"], p["Abar"], n_, T_, p["Xs"], p["Ps"],
                                     p["Xs0"], p["Ps0"], p["Cg"], p["status"], None)

    assert call(ac._handle) == 0
    torch.cuda.synchronize()
    assert (o["status"] == 0).all()
    assert call(ac._handle, n_=-1) == -1 and call(ac._handle, T_=-1) == -1  # AC_ERR_BAD_ARG
    for k in ("X", "P", "Xpred", "Ppred", "Abar", "Xs", "Ps", "status"):
        assert call(ac._handle, **{k: None}) == -1, k
    for k in ("X0", "P0", "Xs0", "Ps0"):
        assert call(ac._handle, **{k: None}) == -1 and b"together" in lib.ac_last_error(), k
    assert call(ac._handle, X0=None, P0=None, Xs0=None, Ps0=None) == 0 and call(ac._handle, Cg=None) == 0
    assert call(ac._handle, Xs=t["X"].data_ptr()) == -1 and b"overlaps" in lib.ac_last_error()
    assert call(ac._handle, Ps=t["Ppred"].data_ptr() + 4 * n) == -1 and call(ac._handle, Cg=t["Abar"].data_ptr()) == -1
    o["status"].fill_(-1)
    assert call(ac._handle, n_=0) == 0 and call(ac._handle, T_=0) == 0 and call(ac._handle, n_=0, Xs=None) == 0
    torch.cuda.synchronize()
    assert (o["status"] == -1).all()  # nothing was launched
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle) == -3  # AC_ERR_UNSUPPORTED
    torch.cuda.synchronize()


def test_smooth_graph_replay(gpu):
    import torch

    n, T = 65, 6
    d, m = chain("poly", n, T)
    ac = d["ac"]
    kw = dict(q=dev(d["Qd"], gpu), r=dev(d["Rd"], gpu), mag_ned=E.MAG)
    bank = ac.ekf(dev(d["x"], gpu), dev(d["P"], gpu), **kw)
    trace = bank.filter(dev(np.repeat(d["u"][None], T, axis=0), gpu), E.DT, dev(d["Z"], gpu), dev(d["masks"], gpu, "i"), record=True)
    ref = bank.smooth(trace, gains=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bank.smooth(trace, gains=True)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = bank.smooth(trace, gains=True)
    g.replay()
    torch.cuda.synchronize()
    for k in OUT:
        assert torch.equal(getattr(ref, k), getattr(out, k)), k


def test_python_surface(gpu):
    """EKF.filter(record=True) and EKF.smooth: numpy in, numpy out; tensors stay tensors; the ABI's bits; one instance as vectors;
    traces without records are rejected"""
    import torch

    T, n = 6, 5
    d, m = chain("poly", n, T)
    ac = d["ac"]
    q, r = E.f32x(E.SIG_Q ** 2), E.f32x(E.SIG_R ** 2)
    rec = filter_call(ac, gpu, d, T)
    want = smooth_call(ac, gpu, rec)
    U = np.repeat(d["u"][None], T, axis=0)
    a = ac.ekf(d["x"], d["P"], q=q, r=r, mag_ned=E.MAG)
    tr = a.filter(U, E.DT, d["Z"], d["masks"], record=True)
    for k in REC + ("X0", "P0"):
        assert getattr(tr, k).dtype == np.float64 and np.array_equal(getattr(tr, k), rec[k].astype(np.float64)), k
    plain = ac.ekf(d["x"], d["P"], q=q, r=r, mag_ned=E.MAG).filter(U, E.DT, d["Z"], d["masks"])
    assert plain.Xpred is None and plain.Ppred is None and plain.Abar is None and plain.X0 is None and plain.P0 is None
    assert np.array_equal(plain.X, tr.X) and np.array_equal(plain.P, tr.P) and np.array_equal(plain.ll, tr.ll)
    with pytest.raises(ValueError):
        a.smooth(plain)
    s = a.smooth(tr, gains=True)
    assert s.X.shape == (T, 13, n) and s.P.shape == (T, 12, 12, n) and s.X0.shape == (13, n) and s.C.shape == (T, 12, 12, n)
    assert s.X.dtype == np.float64 and s.status.dtype == np.int32
    for k in OUT:
        assert np.array_equal(getattr(s, k), want[k].astype(getattr(s, k).dtype)), k
    s2 = a.smooth(tr, initial=False)
    assert s2.X0 is None and s2.P0 is None and s2.C is None and np.array_equal(s2.X, s.X) and np.array_equal(s2.P, s.P)
    # tensors in, tensors out
    b = ac.ekf(dev(d["x"], gpu), dev(d["P"], gpu), q=dev(d["Qd"], gpu), r=dev(d["Rd"], gpu), mag_ned=E.MAG)
    tt = b.filter(dev(U, gpu), E.DT, dev(d["Z"], gpu), dev(d["masks"], gpu, "i"), record=True)
    st = b.smooth(tt, gains=True)
    for k in OUT:
        v = getattr(st, k)
        assert isinstance(v, torch.Tensor) and v.is_cuda and np.array_equal(v.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    # one instance as vectors
    one = ac.ekf(d["x"][:, 2], d["P"][:, :, 2], q=q, r=r, mag_ned=E.MAG)
    t1 = one.filter(U[:, :, 2], E.DT, d["Z"][:, :, 2], d["masks"][:, 2], record=True)
    assert t1.Xpred.shape == (T, 13) and t1.Abar.shape == (T, 12, 12) and t1.X0.shape == (13,)
    s1 = one.smooth(t1, gains=True)
    assert s1.X.shape == (T, 13) and s1.P.shape == (T, 12, 12) and s1.P0.shape == (12, 12) and s1.status.shape == (T,)
    assert np.array_equal(s1.X, s.X[:, :, 2]) and np.array_equal(s1.P, s.P[..., 2]) and np.array_equal(s1.C, s.C[..., 2])
    with pytest.raises(ValueError):
        a.smooth(t1)  # wrong shapes for this bank
