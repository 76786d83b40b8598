"""GPU tests of the batched eigenvalues and flight modes (ac_eig_f32, ac_modes_f32, Aircraft.eig / modes)
against the float64 restatement tests/modes_ref.py.

The bars.  e32 is the host build of the same header (g++; float32 in and out) against float64 eigvals of the same float32 matrix, as
the matching distance modes_ref.err_eig.  The host / float64 pair is first held to 2 x the recorded worst
(modes_ref.E32_WORST) on the batch; the device is then held to 8 x the BATCH'S WORST host e32 (a single instance's e32 is one
draw of a rounding error and can be arbitrarily small; the batch's worst is its scale).  End to end from (x, u) the scale is
the chain e32 (modes_ref.chain_e32), with at most 5 % of a batch left out by their own chain e32.  Every output sits between
guard words; n <= 257."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import lqr_ref as L
from tests import modes_ref as M
from tests.test_gpu_lqr import Guarded, bits_equal

pytestmark = pytest.mark.gpu


def dev_eig(ac, gpu, Mx, max_iters=0, want_iters=True):
    """one ac_eig_f32 call in guarded buffers -> lam, status, iters, (wr, wi) as modes_ref.host_eig returns them"""
    import torch

    lib = ac._sync()
    m, n = Mx.shape[0], Mx.shape[2]
    Mt = torch.tensor(np.ascontiguousarray(Mx, dtype=np.float32), device=gpu)
    g = dict(wr=Guarded((m, n), gpu), wi=Guarded((m, n), gpu), st=Guarded((n,), gpu, torch.int32), it=Guarded((n,), gpu, torch.int32))
    rc = lib.ac_eig_f32(ac._handle, Mt.data_ptr(), m, int(max_iters), n, g["wr"].ptr(), g["wi"].ptr(), g["st"].ptr(),
                        g["it"].ptr() if want_iters else None, ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    wr, wi = g["wr"].t.cpu().numpy(), g["wi"].t.cpu().numpy()
    return wr.astype(np.float64) + 1j * wi, g["st"].np(), g["it"].np(), (wr, wi)


def dev_solver(ac, gpu):
    return lambda Mx, max_iters: dev_eig(ac, gpu, Mx, max_iters)


@pytest.fixture(scope="module")
def ac_poly():
    return L.grid("poly")[0]


def against_host(ac, gpu, Mx, which, tag):
    """the device on a batch of matrices: statuses, the e32 bars, the canonical order; -> device error / batch's worst host e32"""
    ref = M.eigvals(Mx)
    h_lam, h_st, h_it, (h_wr, h_wi) = M.host_eig(Mx)
    e32 = M.err_eig(h_lam, ref)
    assert (h_st == 0).all() and (e32 <= 2 * M.E32_WORST[which]).all(), ("e32 condition", tag, e32.max())
    lam, st, it, (wr, wi) = dev_eig(ac, gpu, Mx)
    assert np.array_equal(st, h_st), (tag, st)
    err = M.err_eig(lam, ref)
    same = bits_equal(wr, h_wr) and bits_equal(wi, h_wi) and np.array_equal(it, h_it)
    ratio = err.max() / e32.max() if e32.max() > 0 else float(err.max() > 0)
    print(f"[modes] {tag}: host e32 {e32.max():.2e}, device {err.max():.2e} ({ratio:.2f} x), bit-identical to the host build: {same}")
    assert (err <= 8 * e32.max()).all(), (tag, err.max(), e32.max())
    M.check_order(wr, wi)
    return ratio


# ---- 1. ac_eig_f32 on the case sets ----------------------------------------------------------------------------------------------
CASE_SETS = {"C1": M.c1, "C2": M.c2, "C3": M.c3}


@pytest.mark.parametrize("which", sorted(CASE_SETS))
def test_eig_case_sets(gpu, ac_poly, which):
    for label, (Mx, dt) in CASE_SETS[which]().items():
        against_host(ac_poly, gpu, Mx, which, f"{which} {label}")


def test_eig_textbook(gpu, ac_poly):
    """C4: the exact expectations, statuses and iteration counts the host build meets"""
    M.check_textbook(dev_solver(ac_poly, gpu))
    M.check_balancing(dev_solver(ac_poly, gpu))


@pytest.mark.parametrize("m", range(1, 14))
def test_eig_shapes(gpu, ac_poly, m):
    """C5: every order, every batch size of lqr_ref.SIZES (tails of the wave included)"""
    for n in L.SIZES:
        against_host(ac_poly, gpu, M.c5(m, n), "C5", f"C5 m={m} n={n}")


# ---- 2. bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 13])
def test_eig_bits_do_not_depend_on_the_batch(gpu, ac_poly, m):
    Mx = M.c5(m, 257)
    lam, st, it, (wr, wi) = dev_eig(ac_poly, gpu, Mx)
    for i in (0, 63, 64, 200, 256):  # alone
        l1, s1, i1, (r1, j1) = dev_eig(ac_poly, gpu, Mx[:, :, i:i + 1])
        assert bits_equal(r1[:, 0], wr[:, i]) and bits_equal(j1[:, 0], wi[:, i]) and s1[0] == st[i] and i1[0] == it[i], i
    # repeated instances at other positions, next to NaN and Inf instances
    order = np.array([5, 200, 5, 17, 200, 5] * 11)[:65]
    B = Mx[:, :, order].copy()
    B[0, 0, 3], B[m - 1, m - 1, 64] = np.nan, np.inf
    lam2, st2, it2, (wr2, wi2) = dev_eig(ac_poly, gpu, B)
    bad = np.zeros(65, bool)
    bad[[3, 64]] = True
    assert (st2[bad] == 3).all() and (it2[bad] == 0).all() and np.isnan(wr2[:, bad]).all() and np.isnan(wi2[:, bad]).all()
    assert bits_equal(wr2[:, ~bad], wr[:, order[~bad]]) and bits_equal(wi2[:, ~bad], wi[:, order[~bad]])
    assert np.array_equal(st2[~bad], st[order[~bad]]) and np.array_equal(it2[~bad], it[order[~bad]])
    # iters is optional; the cap gives status 1 and NaN for the whole instance
    lam3, st3, _, (wr3, wi3) = dev_eig(ac_poly, gpu, Mx[:, :, :5], want_iters=False)
    assert bits_equal(wr3, wr[:, :5]) and np.array_equal(st3, st[:5])
    lam4, st4, it4, (wr4, wi4) = dev_eig(ac_poly, gpu, Mx[:, :, :65], max_iters=1)
    assert (st4 == 1).all() and np.isnan(wr4).all() and np.isnan(wi4).all()


# ---- 3. ac_modes_f32 end to end ----------------------------------------------------------------------------------------------------
def run_modes(ac, gpu, x, u, K=None, coords=M.FLIGHT, dt=M.DT, max_iters=0, export=True):
    """one ac_modes_f32 call in guarded buffers -> dict"""
    import torch

    lib = ac._sync()
    n = x.shape[1]
    X, U = (torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=gpu) for a in (x, u))
    Kt = None if K is None else torch.tensor(np.ascontiguousarray(K, dtype=np.float32), device=gpu)
    need = C.c_size_t()
    assert lib.ac_modes_workspace_floats(ac._handle, n, C.byref(need)) == 0
    g = dict(A=Guarded((12, 12, n), gpu), B=Guarded((12, 7, n), gpu), wr=Guarded((12, n), gpu), wi=Guarded((12, n), gpu),
             sg=Guarded((12, n), gpu), om=Guarded((12, n), gpu), st=Guarded((n,), gpu, torch.int32),
             it=Guarded((n,), gpu, torch.int32), ws=Guarded((need.value,), gpu))
    o = _lib.ModesOpts()
    o.coords, o.max_iters = M.coords_mask(coords), int(max_iters)
    rc = lib.ac_modes_f32(ac._handle, C.byref(o), X.data_ptr(), U.data_ptr(), C.c_float(dt), None if Kt is None else Kt.data_ptr(), n,
                          g["A"].ptr() if export else None, g["B"].ptr() if export else None, g["wr"].ptr(), g["wi"].ptr(),
                          g["sg"].ptr(), g["om"].ptr(), g["st"].ptr(), g["it"].ptr(), g["ws"].ptr(), need.value, ac._stream())
    assert rc == 0, _lib.load().ac_last_error()
    torch.cuda.synchronize()
    for v in g.values():
        v.check()
    out = {k: v.t.cpu().numpy() for k, v in g.items() if k != "ws"}
    m = len(coords)
    out["lam"] = out["wr"][:m].astype(np.float64) + 1j * out["wi"][:m]
    out["s"] = out["sg"][:m].astype(np.float64) + 1j * out["om"][:m]
    out["raw"] = np.stack([out["wr"], out["wi"], out["sg"], out["om"]])
    out["X"], out["U"] = X, U
    return out


MODES_CASES = [(name, loop, sel) for name in M.CHAIN_MODELS for loop, sel in M.CHAIN_LOOPS]


@pytest.mark.parametrize("name,loop,sel", MODES_CASES, ids=[f"{a}-{b}-{c}" for a, b, c in MODES_CASES])
def test_modes_against_float64(gpu, name, loop, sel):
    ac, orc, xg, ug = L.grid(name)
    n, m0 = 65, xg.shape[1]
    x, u = L.cycle(xg, n), L.cycle(ug, n)
    coords = M.COORDS[sel]
    design = ac.lqr((x, u), M.DT, q=L.SELECTIONS[sel])
    K = None
    if loop == "closed":
        K = design.K
    d = run_modes(ac, gpu, x, u, K, coords)
    # -- the exported linearisation is ac_lqr_f32's, bit for bit; without the export the eigenvalues are the same bits
    assert bits_equal(d["A"], design.A) and bits_equal(d["B"], design.B)
    d2 = run_modes(ac, gpu, x, u, K, coords, export=False)
    assert bits_equal(d2["raw"], d["raw"]) and np.array_equal(d2["st"], d["st"]) and np.array_equal(d2["it"], d["it"])
    # -- a repeated instance gives the same bits wherever it sits; rows >= m are 0
    first = np.arange(n) % m0
    assert bits_equal(d["raw"], d["raw"][..., first]) and np.array_equal(d["it"], d["it"][first])
    assert (d["raw"][:, len(coords):] == 0).all()
    # -- the chain bar on the distinct instances
    u_ = np.arange(m0)
    ok = np.ones(m0, bool) if K is None else np.asarray(design.converged)[u_]
    Kc = None if K is None else np.where(ok, K[..., u_], 0.0)
    e, es, lam64, s64 = M.chain_e32(orc, x[:, u_], u[:, u_], Kc, coords)
    keep = ok & (e <= 2 * M.E32_WORST["chain"]) & (es <= 2 * M.E32_WORST["chain_s"])
    assert (~keep).sum() <= 0.05 * m0, ("e32 condition: left out", int((~keep).sum()), "of", m0, e.max(), es.max())
    assert (d["st"][u_][keep] == 0).all()
    err, errs = M.err_eig(d["lam"][:, u_], lam64), M.err_s(d["s"][:, u_], s64, M.DT)
    print(f"[modes] {name} {loop} {sel}: kept {keep.sum()}/{m0}; chain e32 {e[keep].max():.2e} device {err[keep].max():.2e}; "
          f"s dt chain {es[keep].max():.2e} device {errs[keep].max():.2e}; QR iterations per eigenvalue {d['it'].mean() / len(coords):.2f}")
    assert (err[keep] <= 8 * e[keep].max()).all(), ("eigenvalues", err[keep].max(), e[keep].max())
    assert (errs[keep] <= 8 * es[keep].max()).all(), ("s", errs[keep].max(), es[keep].max())
    # -- sigma, omega against the device's own eigenvalues; the order
    fs, fo = M.sigma_form_err(d["raw"][..., u_][..., keep], len(coords), M.DT)
    assert (fs <= 1).all() and (fo <= 1).all(), (fs.max(), fo.max())
    M.check_order(d["wr"][:len(coords)], d["wi"][:len(coords)])
    if loop == "closed":
        assert (np.abs(d["lam"][:, u_][:, keep]) < 1).all()


def test_modes_tails_and_planted_nans(gpu):
    ac, orc, xg, ug = L.grid("poly")
    ref = run_modes(ac, gpu, L.cycle(xg, 257), L.cycle(ug, 257))
    for n in L.SIZES:
        d = run_modes(ac, gpu, L.cycle(xg, n), L.cycle(ug, n))
        assert bits_equal(d["raw"], ref["raw"][..., :n]) and np.array_equal(d["st"], ref["st"][:n]), n
        assert bits_equal(d["A"], ref["A"][..., :n])
    x, u = L.cycle(xg, 65).copy(), L.cycle(ug, 65).copy()
    x[4, 7], u[1, 20], x[8, 64] = np.nan, np.nan, np.inf
    bad = np.zeros(65, bool)
    bad[[7, 20, 64]] = True
    d = run_modes(ac, gpu, x, u)
    assert (d["st"][bad] == 3).all() and (d["it"][bad] == 0).all() and np.isnan(d["raw"][:, :8][..., bad]).all()
    assert (d["raw"][:, 8:] == 0).all()
    assert bits_equal(d["raw"][..., ~bad], ref["raw"][..., :65][..., ~bad]) and (d["st"][~bad] == 0).all()
    capped = run_modes(ac, gpu, x, u, max_iters=1)
    assert (capped["st"][~bad] == 1).all() and np.isnan(capped["raw"][:, :8]).all()


def test_modes_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    ac, orc, xg, ug = L.grid("poly")
    ac._sync()
    n = 8
    X = torch.tensor(L.cycle(xg, n), dtype=torch.float32, device=gpu)
    U = torch.tensor(L.cycle(ug, n), dtype=torch.float32, device=gpu)
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    out = z(4, 12, n)
    S, it = torch.zeros(n, dtype=torch.int32, device=gpu), torch.zeros(n, dtype=torch.int32, device=gpu)
    need = C.c_size_t()
    assert lib.ac_modes_workspace_floats(ac._handle, n, C.byref(need)) == 0 and need.value >= n * 501
    ws = z(need.value)

    def call(h, coords=0, max_iters=0, wsn=need.value, dt=M.DT, n_=n, x_ptr=X.data_ptr(), wr_ptr=out[0].data_ptr()):
        o = _lib.ModesOpts()
        o.coords, o.max_iters = coords, max_iters
        return lib.ac_modes_f32(h, C.byref(o), x_ptr, U.data_ptr(), C.c_float(dt), None, n_, None, None, wr_ptr, out[1].data_ptr(),
                                out[2].data_ptr(), out[3].data_ptr(), S.data_ptr(), it.data_ptr(), ws.data_ptr(), wsn, None)

    assert call(ac._handle) == 0 and call(ac._handle, coords=0xFFF) == 0 and call(ac._handle, n_=0) == 0
    torch.cuda.synchronize()
    assert (S == 0).all()
    assert call(ac._handle, wsn=need.value - 1) == -6  # AC_ERR_WORKSPACE
    for kw in (dict(coords=0xEF0), dict(coords=0x1EF8), dict(max_iters=-1), dict(dt=0.0), dict(dt=float("nan")), dict(n_=-1),
               dict(x_ptr=None), dict(wr_ptr=None), dict(wr_ptr=X.data_ptr())):  # (the last: an output on an input)
        assert call(ac._handle, **kw) == -1, kw
    qd = Quadrotor()
    qd._sync()
    assert call(qd._handle) == -3 and lib.ac_modes_workspace_floats(qd._handle, n, C.byref(need)) == -3  # AC_ERR_UNSUPPORTED
    Mt, w = z(3, 3, n), z(2, 3, n)

    def eig(m=3, max_iters=0, n_=n, m_ptr=Mt.data_ptr(), wr_ptr=w[0].data_ptr()):
        return lib.ac_eig_f32(qd._handle, m_ptr, m, max_iters, n_, wr_ptr, w[1].data_ptr(), S.data_ptr(), None, None)

    assert eig() == 0 and eig(n_=0) == 0
    for kw in (dict(m=0), dict(m=14), dict(max_iters=-1), dict(n_=-1), dict(m_ptr=None), dict(wr_ptr=None), dict(wr_ptr=Mt.data_ptr())):
        assert eig(**kw) == -1, kw
    torch.cuda.synchronize()


# ---- 4. the Python surface --------------------------------------------------------------------------------------------------------
def test_modes_python_surface(gpu):
    import torch

    ac, orc, xg, ug = L.grid("poly")
    trim = ac.trim(np.linspace(30.0, 50.0, 5), turn_rate=0.1)
    assert trim.converged.all()
    a = ac.modes(trim, M.DT)
    b = ac.modes((trim.x, trim.u), M.DT, coords=M.FLIGHT, max_iters=30)
    assert a.lam.shape == (8, 5) and a.lam.dtype == np.complex128 and a.s.dtype == np.complex128 and a.coords == M.FLIGHT
    assert a.converged.all() and a.dt == M.DT and a.A.shape == (12, 12, 5) and a.B.shape == (12, 7, 5)
    for k in ("lam", "s", "wn", "zeta", "rho", "unstable", "A", "B", "status", "iterations"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    assert np.array_equal(a.rho, np.abs(a.lam).max(axis=0)) and np.array_equal(a.unstable, (np.abs(a.lam) > 1).sum(axis=0))
    assert np.allclose(a.wn, np.abs(a.s)) and np.allclose(a.zeta, -a.s.real / np.abs(a.s), equal_nan=True)
    assert (M.err_s(a.s, M.s_of(a.lam, M.DT), M.DT) <= 1e-6).all()
    one = ac.modes((trim.x[:, 2], trim.u[:, 2]), M.DT)
    assert one.lam.shape == (8,) and np.array_equal(one.lam, a.lam[:, 2]) and int(one.status) == 0
    # tensors stay on the device
    X, U = (torch.tensor(v, dtype=torch.float32, device=gpu) for v in (trim.x, trim.u))
    t = ac.modes((X, U), M.DT, coords="all")
    assert t.lam.is_cuda and t.lam.dtype == torch.complex64 and t.lam.shape == (12, 5) and t.rho.shape == (5,)
    full = ac.modes(trim, M.DT, coords="all")
    assert np.array_equal(t.lam.cpu().numpy().astype(np.complex128), full.lam)
    assert len(ac.modes(trim, M.DT, coords="path").coords) == 11
    # closed loop: an LqrResult, or its K; a design for another dt is refused
    res = ac.lqr(trim, M.DT)
    c1, c2 = ac.modes(trim, M.DT, gains=res), ac.modes(trim, M.DT, gains=res.K)
    assert np.array_equal(c1.lam, c2.lam) and (c1.rho < 1).all() and (c1.unstable == 0).all()
    assert np.abs(c1.rho - L.rho(res.A, res.B, res.K, L.Q8)).max() <= 1e-5
    with pytest.raises(ValueError):
        ac.modes(trim, 0.02, gains=res)
    # Aircraft.eig
    Mx = M.c5(6, 9)
    lam, st = ac.eig(Mx)
    assert lam.shape == (6, 9) and lam.dtype == np.complex128 and (st == 0).all()
    l1, s1 = ac.eig(Mx[:, :, 4])
    assert l1.shape == (6,) and np.array_equal(l1, lam[:, 4]) and int(s1) == 0
    lt, stt = ac.eig(torch.tensor(Mx, dtype=torch.float32, device=gpu))
    assert lt.is_cuda and lt.dtype == torch.complex64 and np.array_equal(lt.cpu().numpy().astype(np.complex128), lam)


def test_modes_graph_replay(gpu):
    import torch

    ac, orc, xg, ug = L.grid("poly")
    n = 65
    X = torch.tensor(L.cycle(xg, n), dtype=torch.float32, device=gpu)
    U = torch.tensor(L.cycle(ug, n), dtype=torch.float32, device=gpu)
    K = ac.lqr((X, U), M.DT, q=L.Q12).K
    ref = ac.modes((X, U), M.DT, gains=K, coords="all")
    ws = ac.modes_workspace(n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.modes((X, U), M.DT, gains=K, coords="all", ws=ws)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = ac.modes((X, U), M.DT, gains=K, coords="all", ws=ws)
    g.replay()
    torch.cuda.synchronize()
    for k in ("lam", "s", "rho", "unstable", "A", "B", "status", "iterations"):
        assert torch.equal(getattr(ref, k), getattr(out, k)), k
    assert bool(out.converged.all())
