"""GPU tests of the EM statistics for the EKF's noise variances (ac_ekf_em_f32, EKF.noise_stats, EKF.set_noise, EKF.fit_noise;
DESIGN.md §4.17) against the float64 restatement tests/em_ref.py.

Instances: the filter chains of tests/test_gpu_rts.py (ekf_ref.chain_inputs cycled to the batch sizes).  The shapes (n, T) cover
a single node, the shortest load-ahead, a partial group, a chunk boundary (kEmChunk + 1), several chunks with a partial last
one, and a partial last workgroup.  Every output sits between guard words.

The bars (the protocol of tests/test_gpu_rts.py).  The device, the float32 host build of the same header and the float64
restatement all read THE DEVICE'S OWN records (ac_ekf_filter_rec_f32) and smoothed trace (ac_ekf_smooth_f32).  e32 is host
against float64 per instance and measure; an instance is checked when its e32 is within 2 x the recorded worst
(em_ref.E32_WORST); at most 5 % of a batch's distinct instances may miss that.  The device is then held to 8 x the worst e32
of the checked instances of its batch, measure by measure (em_ref.hold prints each figure first).  Status and counts must be
equal."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import ekf_ref as E
from tests import em_ref as M
from tests.test_gpu_lqr import Guarded, bits_equal
from tests.test_gpu_rts import chain, dev, filter_call, smooth_call

pytestmark = pytest.mark.gpu

MODELS = ("poly", "default", "real_net")
CH = _lib.EM_CHUNK
SHAPES = ((1, 1), (1, 2), (5, 3), (17, CH + 1), (3, 2 * CH + 5), (257, 20))
OUT = ("Qsum", "Rsum", "nq", "nr", "status", "Qn", "Rn")


def em_opts(floor=0.0):
    o = _lib.EkfEmOpts()
    o.mag_ned[:] = [float(v) for v in E.MAG]
    o.floor_rel = floor
    return o


def em_call(ac, gpu, rec, sm, d, new=True, floor=0.0):
    """one ac_ekf_em_f32 call on the device's records `rec` and smoothed trace `sm` in guarded buffers -> dict of the raw arrays"""
    import torch

    lib = ac._sync()
    T, n = rec["Xpred"].shape[0], rec["Xpred"].shape[2]
    a = [dev(v, gpu) for v in (rec["Xpred"], rec["Ppred"], sm["X"], sm["P"], d["Z"])] + [dev(rec["used"], gpu, "i"), dev(d["Qd"], gpu), dev(d["Rd"], gpu)]
    need = C.c_size_t()
    assert lib.ac_ekf_em_workspace_floats(ac._handle, n, T, C.byref(need)) == 0
    g = dict(Qsum=Guarded((12, n), gpu), Rsum=Guarded((15, n), gpu), nq=Guarded((n,), gpu, torch.int32), nr=Guarded((15, n), gpu, torch.int32),
             status=Guarded((T, n), gpu, torch.int32), ws=Guarded((need.value,), gpu))
    if new:
        g.update(Qn=Guarded((12, n), gpu), Rn=Guarded((15, n), gpu))
    ptr = lambda k: g[k].ptr() if k in g else None  # noqa: E731
    o = em_opts(floor)
    rc = lib.ac_ekf_em_f32(ac._handle, C.byref(o), *(t.data_ptr() for t in a), n, T, *(ptr(k) for k in OUT), g["ws"].ptr(), need.value,
                           ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    out = {k: None for k in OUT}
    out.update({k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"})
    return out


def records(name, n, T, gpu):
    """the chain, the device's records and its smoothed trace (without the initial node, as EKF.fit_noise smooths)"""
    d, m = chain(name, n, T)
    rec = filter_call(d["ac"], gpu, d, T)
    assert (rec["status"] == 0).all()
    return d, m, rec, smooth_call(d["ac"], gpu, rec, initial=False, gains=False)


def refs(rec, sm, d, m, eps):
    """float64 and the host build on the first m columns of the device's records"""
    a = [v.astype(np.float64)[..., :m] for v in (rec["Xpred"], rec["Ppred"], sm["X"], sm["P"], np.asarray(d["Z"], np.float32))]
    a += [rec["used"][..., :m], d["Qd"][:, :m], d["Rd"][:, :m]]
    return M.noise_stats(*a, eps=eps), M.host_noise_stats(*a, eps=eps)


def same_bits(a, b, keys=OUT, cols=slice(None)):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert np.array_equal(a[k][..., cols].view(np.int32), b[k][..., cols].view(np.int32)), k


def as64(out, m):
    return {k: out[k][..., :m].astype(np.float64) for k in ("Qsum", "Rsum")}


# ---- 1. against float64 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T", SHAPES, ids=[f"n{n}-T{T}" for n, T in SHAPES])
@pytest.mark.parametrize("name", MODELS)
def test_statistics_against_float64(gpu, name, n, T):
    d, m, rec, sm = records(name, n, T, gpu)
    ac = d["ac"]
    out = em_call(ac, gpu, rec, sm, d)
    ref, host = refs(rec, sm, d, m, d["eps"])
    # a repeated instance gives the same bits wherever it sits in the batch
    first = np.arange(n) % m
    for k in OUT:
        assert np.array_equal(out[k].view(np.int32), out[k][..., first].view(np.int32)), k
    for k in ("status", "nq", "nr"):
        assert np.array_equal(out[k][..., :m], ref[k]) and np.array_equal(host[k], ref[k]), k
    assert (out["status"] == 0).all() and (out["nq"] == T).all()
    # without Qn, Rn: the same bits elsewhere
    same_bits(em_call(ac, gpu, rec, sm, d, new=False), out, keys=("Qsum", "Rsum", "nq", "nr", "status"))
    M.hold(f"{name} n={n} T={T}", M.errors(as64(out, m), ref), M.errors(host, ref), m)
    # the new variances: the means, at least the floor
    for s, c, v, old in (("Qsum", out["nq"][None], "Qn", d["Qd"]), ("Rsum", out["nr"], "Rn", d["Rd"])):
        with np.errstate(all="ignore"):
            want = np.where(c > 0, np.maximum(out[s].astype(np.float64) / np.maximum(c, 1), 1e-4 * old), old)
        assert np.allclose(out[v], want, rtol=3e-7, atol=0), v
        none = np.broadcast_to(c == 0, out[v].shape)
        assert bits_equal(out[v][none], np.asarray(old, np.float32)[none]), v  # nothing counted: the input bit for bit


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_batch(gpu):
    n, T = 257, 20
    d, m, rec, sm = records("poly", n, T, gpu)
    ac = d["ac"]
    big = em_call(ac, gpu, rec, sm, d)
    for k in (0, 5, 41 % m):
        cut = lambda v: np.ascontiguousarray(v[..., k:k + 1])  # noqa: E731
        one = em_call(ac, gpu, {key: cut(v) for key, v in rec.items()}, {key: cut(v) for key, v in sm.items() if v is not None},
                      {key: cut(d[key]) for key in ("Z", "Qd", "Rd")})
        for pos in (k, k + m, k + 5 * m):  # in a first group, mid-wave, in the last workgroups
            for key in OUT:
                assert np.array_equal(one[key][..., 0].view(np.int32), big[key][..., pos].view(np.int32)), (key, k, pos)


# ---- 3. status paths (finite inputs or planted NaNs: value paths, nothing here faults) ---------------------------------------------------
def test_status_paths(gpu):
    n, T = 17, CH + 1
    d, m, rec, sm = records("poly", n, T, gpu)
    ac = d["ac"]
    clean = em_call(ac, gpu, rec, sm, d)
    rec, sm = {k: v.copy() for k, v in rec.items()}, {k: v.copy() for k, v in sm.items() if v is not None}
    used = rec["used"]
    rec["Ppred"][12][:, :, 3] *= -1.0        # not positive definite: node 12 of instance 3 is out of Q, its R terms stay
    sm["P"][7][3, 4, 16] = np.nan            # a NaN record: node 7 of instance 16 (the last one) adds nothing
    rec["Ppred"][CH][2, 2, 9] = 0.0          # a zero pivot in the second chunk: node kEmChunk of instance 9
    used[:, 5] &= ~(1 << 9)                  # the airspeed row of instance 5 is never used
    out = em_call(ac, gpu, rec, sm, d)
    want = np.zeros((T, n), np.int32)
    want[12, 3], want[7, 16], want[CH, 9] = M.NOT_PD, M.NONFINITE, M.NOT_PD
    assert np.array_equal(out["status"], want)
    ref, host = refs(rec, sm, d, n, d["eps"])
    for k in ("status", "nq", "nr"):
        assert np.array_equal(out[k], ref[k]) and np.array_equal(host[k], ref[k]), k
    assert out["nq"][3] == T - 1 and out["nq"][16] == T - 1 and out["nq"][9] == T - 1
    assert bits_equal(out["Rsum"][:, 3], clean["Rsum"][:, 3]) and np.array_equal(out["nr"][:, 3], clean["nr"][:, 3])
    assert (out["nr"][6:, 16] == T - 1).all() and (out["Rsum"][6:, 16] < clean["Rsum"][6:, 16]).all()
    assert out["nr"][9, 5] == 0 and out["Rsum"][9, 5] == 0 and bits_equal(out["Rn"][9, 5], np.float32(d["Rd"][9, 5]))
    assert np.isfinite(out["Qsum"]).all() and np.isfinite(out["Rsum"]).all()
    others = np.ones(n, bool)
    others[[3, 16, 9, 5]] = False
    same_bits(out, clean, cols=others)
    M.hold("status paths", M.errors(as64(out, n), ref), M.errors(host, ref), m)


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------------------
def test_em_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    n, T = 8, 3
    d, m, rec, sm = records("poly", n, T, gpu)
    ac = d["ac"]
    t = dict(Xpred=dev(rec["Xpred"], gpu), Ppred=dev(rec["Ppred"], gpu), Xs=dev(sm["X"], gpu), Ps=dev(sm["P"], gpu), Z=dev(d["Z"], gpu),
             used=dev(rec["used"], gpu, "i"), Qd=dev(d["Qd"], gpu), Rd=dev(d["Rd"], gpu))
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    zi = lambda *s: torch.full(s, -1, device=gpu, dtype=torch.int32)  # noqa: E731
    need = C.c_size_t()
    assert lib.ac_ekf_em_workspace_floats(ac._handle, n, T, C.byref(need)) == 0
    o = dict(Qsum=z(12, n), Rsum=z(15, n), nq=zi(n), nr=zi(15, n), status=zi(T, n), Qn=z(12, n), Rn=z(15, n), ws=z(need.value))

    def call(h, n_=n, T_=T, floor=0.0, ws_floats=need.value, **kw):
        p = {k: v.data_ptr() for k, v in {**t, **o}.items()}
        p.update(kw)
        op = em_opts(floor)
        return lib.ac_ekf_em_f32(h, C.byref(op), p["Xpred"], p["Ppred"], p["Xs"], p["Ps"], p["Z"], p["used"], p["Qd"], p["Rd"], n_, T_,
                                 p["Qsum"], p["Rsum"], p["nq"], p["nr"], p["status"], p["Qn"], p["Rn"], p["ws"], ws_floats, None)

    assert call(ac._handle) == 0
    torch.cuda.synchronize()
    assert (o["status"] == 0).all() and (o["nq"] == T).all()
    assert call(ac._handle, n_=-1) == -1 and call(ac._handle, T_=-1) == -1  # AC_ERR_BAD_ARG
    for k in ("Xpred", "Ppred", "Xs", "Ps", "Z", "used", "Qd", "Rd", "Qsum", "Rsum", "nq", "nr", "status"):
        assert call(ac._handle, **{k: None}) == -1, k
    assert call(ac._handle, Qn=None) == 0 and call(ac._handle, Rn=None) == 0 and call(ac._handle, Qn=None, Rn=None) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(ac._handle, floor=bad) == -1 and b"floor_rel" in lib.ac_last_error()
    assert call(ac._handle, Qsum=t["Qd"].data_ptr()) == -1 and b"overlaps" in lib.ac_last_error()
    assert call(ac._handle, Rn=t["Rd"].data_ptr() + 4 * n) == -1 and call(ac._handle, status=t["used"].data_ptr()) == -1
    assert call(ac._handle, ws=t["Ps"].data_ptr()) == -1
    assert call(ac._handle, ws=None) == -6 and call(ac._handle, ws_floats=need.value - 1) == -6  # AC_ERR_WORKSPACE
    torch.cuda.synchronize()
    for k in ("nq", "nr", "status"):
        o[k].fill_(-1)
    assert call(ac._handle, n_=0) == 0 and call(ac._handle, n_=0, Qsum=None) == 0
    torch.cuda.synchronize()
    assert (o["status"] == -1).all() and (o["nq"] == -1).all() and (o["nr"] == -1).all()  # nothing was launched
    # T = 0: zero sums and counts, Qn, Rn the inputs bit for bit
    o["Qsum"].fill_(7.0)
    assert call(ac._handle, T_=0) == 0 and call(ac._handle, T_=0, Xpred=None, status=None) == 0
    torch.cuda.synchronize()
    assert (o["Qsum"] == 0).all() and (o["Rsum"] == 0).all() and (o["nq"] == 0).all() and (o["nr"] == 0).all() and (o["status"] == -1).all()
    assert torch.equal(o["Qn"], t["Qd"]) and torch.equal(o["Rn"], t["Rd"])
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle) == -3 and lib.ac_ekf_em_workspace_floats(qd._handle, n, T, C.byref(need)) == -3  # AC_ERR_UNSUPPORTED
    torch.cuda.synchronize()


def bank_of(d, gpu, tensors=True, q=None, r=None):
    ac = d["ac"]
    q, r = d["Qd"] if q is None else q, d["Rd"] if r is None else r
    if tensors:
        return ac.ekf(dev(d["x"], gpu), dev(d["P"], gpu), q=dev(q, gpu), r=dev(r, gpu), mag_ned=E.MAG)
    return ac.ekf(d["x"], d["P"], q=q, r=r, mag_ned=E.MAG)


def test_em_graph_replay(gpu):
    import torch

    n, T = 65, CH + 3
    d, m = chain("poly", n, T)
    bank = bank_of(d, gpu)
    Z = dev(d["Z"], gpu)
    trace = bank.filter(dev(np.repeat(d["u"][None], T, axis=0), gpu), E.DT, Z, dev(d["masks"], gpu, "i"), record=True)
    sm = bank.smooth(trace, initial=False)
    ws = d["ac"].ekf_em_workspace(n, T)
    args = [bank._rows(v, (T,) + lead, rows, "x") for v, lead, rows in ((trace.Xpred, (), 13), (trace.Ppred, (12,), 12), (sm.X, (), 13), (sm.P, (12,), 12))]
    ref = bank._noise_stats(*args, Z, trace.used, T, 0.0, ws)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bank._noise_stats(*args, Z, trace.used, T, 0.0, ws)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = bank._noise_stats(*args, Z, trace.used, T, 0.0, ws)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(ref, out):
        assert torch.equal(a, b)


# ---- 5. the Python surface ------------------------------------------------------------------------------------------------------------
def test_python_surface(gpu):
    """EKF.q, EKF.r, set_noise, noise_stats: numpy in, numpy out; tensors stay tensors; the ABI's bits; one instance as vectors"""
    import torch

    T, n = CH + 2, 5
    d, m, rec, sm = records("poly", n, T, gpu)
    ac = d["ac"]
    want = em_call(ac, gpu, rec, sm, d)
    U = np.repeat(d["u"][None], T, axis=0)
    a = bank_of(d, gpu, tensors=False, q=E.f32x(E.SIG_Q ** 2), r=E.f32x(E.SIG_R ** 2))
    assert a.q.shape == (12, n) and a.r.shape == (15, n) and a.q.dtype == np.float64 and np.array_equal(a.q, d["Qd"]) and np.array_equal(a.r, d["Rd"])
    tr = a.filter(U, E.DT, d["Z"], d["masks"], record=True)
    s = a.smooth(tr, initial=False)
    st = a.noise_stats(tr, s, d["Z"])
    assert st.Qsum.dtype == np.float64 and st.nq.dtype == np.int32 and st.status.shape == (T, n) and st.q.shape == (12, n) and st.nr.shape == (15, n)
    for k, v in zip(OUT, (st.Qsum, st.Rsum, st.nq, st.nr, st.status, st.q, st.r)):
        assert np.array_equal(v, want[k].astype(v.dtype)), k
    assert np.array_equal(a.q, d["Qd"])  # noise_stats does not change the bank
    a.set_noise(q=st.q)
    assert np.array_equal(a.q, st.q) and np.array_equal(a.r, d["Rd"])
    a.set_noise(r=2 * E.SIG_R ** 2)
    assert np.array_equal(a.r, np.repeat(E.f32x(2 * E.SIG_R ** 2)[:, None], n, axis=1)) and np.array_equal(a.q, st.q)
    with pytest.raises(ValueError):
        a.set_noise(r=np.zeros(15))
    with pytest.raises(ValueError):
        a.noise_stats(a.filter(U, E.DT, d["Z"], d["masks"]), s, d["Z"])  # a trace without records
    # tensors in, tensors out
    b = bank_of(d, gpu)
    Zt = dev(d["Z"], gpu)
    tt = b.filter(dev(U, gpu), E.DT, Zt, dev(d["masks"], gpu, "i"), record=True)
    sb = b.noise_stats(tt, b.smooth(tt, initial=False), Zt)
    for k, v in zip(OUT, (sb.Qsum, sb.Rsum, sb.nq, sb.nr, sb.status, sb.q, sb.r)):
        assert isinstance(v, torch.Tensor) and v.is_cuda and np.array_equal(v.cpu().numpy().view(np.int32), want[k].view(np.int32)), k
    assert isinstance(b.q, torch.Tensor) and b.q.is_cuda
    # one instance as vectors
    one = ac.ekf(d["x"][:, 2], d["P"][:, :, 2], q=E.SIG_Q ** 2, r=E.SIG_R ** 2, mag_ned=E.MAG)
    assert one.q.shape == (12,) and one.r.shape == (15,)
    t1 = one.filter(U[:, :, 2], E.DT, d["Z"][:, :, 2], d["masks"][:, 2], record=True)
    s1 = one.noise_stats(t1, one.smooth(t1, initial=False), d["Z"][:, :, 2])
    assert s1.Qsum.shape == (12,) and s1.nr.shape == (15,) and s1.status.shape == (T,) and s1.nq.shape == ()
    assert np.array_equal(s1.Qsum, st.Qsum[:, 2]) and np.array_equal(s1.Rsum, st.Rsum[:, 2]) and np.array_equal(s1.r, st.r[:, 2])
    with pytest.raises(ValueError):
        a.noise_stats(t1, s, d["Z"])  # wrong shapes for this bank


def wrong_start():
    """variances wrong by 16 x either way (sigma by 4 x), as examples/ekf_tune_noise.py starts"""
    return (E.f32x(E.SIG_Q ** 2 * np.where(np.arange(12) % 2 == 0, 16.0, 1 / 16.0)),
            E.f32x(E.SIG_R ** 2 * np.where(np.arange(15) % 2 == 0, 1 / 16.0, 16.0)))


def test_fit_noise_is_the_hand_written_loop(gpu):
    T, n, ITERS = CH + 2, 9, 3
    d, m = chain("poly", n, T)
    ac = d["ac"]
    U = np.repeat(d["u"][None], T, axis=0)
    q0, r0 = wrong_start()
    a = bank_of(d, gpu, tensors=False, q=q0, r=r0)
    x0, P0 = a.x.copy(), a.P.copy()
    fit = a.fit_noise(U, E.DT, d["Z"], d["masks"], iters=ITERS)
    assert np.array_equal(a.x, x0) and np.array_equal(a.P, P0)  # the estimate is what it was on entry
    assert np.array_equal(a.q, fit.q) and np.array_equal(a.r, fit.r) and fit.ll.shape == (ITERS + 1, n)
    q, r, ll = np.repeat(q0[:, None], n, axis=1), np.repeat(r0[:, None], n, axis=1), []
    for _ in range(ITERS):
        b = bank_of(d, gpu, tensors=False, q=q, r=r)
        tr = b.filter(U, E.DT, d["Z"], d["masks"], record=True)
        st = b.noise_stats(tr, b.smooth(tr, initial=False), d["Z"])
        ll.append(tr.ll)
        q, r = st.q, st.r
    ll.append(bank_of(d, gpu, tensors=False, q=q, r=r).filter(U, E.DT, d["Z"], d["masks"]).ll)
    assert np.array_equal(fit.q, q) and np.array_equal(fit.r, r) and np.array_equal(fit.ll, np.stack(ll))
    assert np.array_equal(fit.nq, st.nq) and np.array_equal(fit.nr, st.nr) and np.array_equal(fit.status, st.status)
    # update=("r",) leaves q alone
    c = bank_of(d, gpu, tensors=False, q=q0, r=r0)
    only = c.fit_noise(U, E.DT, d["Z"], d["masks"], iters=1, update=("r",))
    assert np.array_equal(only.q, np.repeat(q0[:, None], n, axis=1)) and not np.array_equal(only.r, np.repeat(r0[:, None], n, axis=1))


def test_fit_noise_shared_and_likelihood(gpu):
    """share=True gives identical columns; from the mis-scaled start the summed log-likelihood rises, on the device as in the
    pooled float64 loop on the host over the same logs (em_ref.em_iteration), which it is held against and not against truth:
    the gain in ll and the fitted sigma within 1 %.  (Per iteration the float32 filter's ll is within 9e-6 (1 + |ll|) and the
    statistic within 1e-5 of float64, ekf_ref / em_ref E32_WORST; an EM step contracts, so four iterations stay two orders of
    magnitude inside 1 %.)"""
    T, n, ITERS = 40, 42, 4
    d, m = chain("poly", n, T)
    U = np.repeat(d["u"][None], T, axis=0)
    q0, r0 = wrong_start()
    a = bank_of(d, gpu, tensors=False, q=q0, r=r0)
    fit = a.fit_noise(U, E.DT, d["Z"], d["masks"], iters=ITERS, share=True)
    assert (fit.q == fit.q[:, :1]).all() and (fit.r == fit.r[:, :1]).all()
    ll = fit.ll.sum(axis=1)
    print("[em] shared fit, device: summed ll per iteration " + " ".join(f"{v:.0f}" for v in ll))
    assert ll[-1] > ll[0]
    # the float64 pooled loop on the same logs
    q, r, ref = np.repeat(q0[:, None], n, axis=1), np.repeat(r0[:, None], n, axis=1), []
    for _ in range(ITERS):
        st, l, _ = M.em_iteration(d["orc"].step_sens, d["x"], d["P"], d["u"], d["Z"], d["masks"], q, r, E.MAG, d["eps"])
        ref.append(float(l.sum()))
        q, r = M.pooled(st, q, r)
    ref.append(float(M.filter_run(d["orc"].step_sens, d["x"], d["P"], d["u"], d["Z"], d["masks"], q, r, E.MAG, d["eps"])["ll"].sum()))
    print("[em] shared fit, float64: summed ll per iteration " + " ".join(f"{v:.0f}" for v in ref))
    assert ref[-1] > ref[0]
    # the device's loop follows the reference loop: the gain in ll within 1 %, the fitted sigma within 1 %
    assert abs((ll[-1] - ll[0]) / (ref[-1] - ref[0]) - 1) <= 1e-2
    assert np.abs(np.sqrt(fit.q[:, 0] / q[:, 0]) - 1).max() <= 1e-2 and np.abs(np.sqrt(fit.r[:, 0] / r[:, 0]) - 1).max() <= 1e-2
