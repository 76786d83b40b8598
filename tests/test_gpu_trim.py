"""GPU tests of the steady-flight trim (ac_trim_f32, Aircraft.trim): every converged trim of every model
against the float64 oracle's own f, the getters' angles against z, coverage against the same LM restated in float64,
determinism across batch sizes and iteration counts, graph replay, steady flight under the integrator, the error codes
and the glide-polar example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import trim_ref as T
from tests.helpers import ROOT, make_aircraft, make_oracle

pytestmark = pytest.mark.gpu

MODELS = {  # name -> make_aircraft arguments
    "default": dict(model="default"),
    "linear": dict(model="linear"),
    "poly": dict(model="poly"),
    "real_net": dict(model="nn"),
    "net_4x128": dict(model="nn", hidden=(128, 128, 128, 128)),
    "net_3x64_valu": dict(model="nn", hidden=(64, 64, 64), use_mfma=False),
}
NETS = ("real_net", "net_4x128", "net_3x64_valu")
SYNTHETIC_NETS = ("net_4x128", "net_3x64_valu")


def problem(name, seed=0):
    """The grid of the issue: V x turn rate x beta x flaps, random psi.  The linear model trims its turns in mode 1
    (held rudder 0, beta solved).  -> list of (lateral, kwargs for trim, target (7, n), uhold (7, n))"""
    cases = T.grid(seed=seed)
    out = []
    for lateral in (0, 1):
        sel = [c for c in cases if (name == "linear" and c[1] != 0.0) == (lateral == 1)]
        if not sel:
            continue
        V, psid, beta, fl, psi = (np.array(v) for v in zip(*sel))
        kw = dict(psi=psi, turn_rate=psid, flaps=fl)
        if lateral:
            kw["rudder"] = np.zeros(len(sel))
        else:
            kw["beta"] = beta
        n = len(sel)
        tg = np.stack([np.zeros(n), np.zeros(n), np.full(n, -200.0), V, psi, psid, np.zeros(n) if lateral else beta])
        uh = np.zeros((7, n))
        uh[6] = fl
        tg, uh = (np.float32(a).astype(np.float64) for a in (tg, uh))
        out.append((lateral, V, kw, tg, uh))
    return out


# ---- 1. truth check ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_trim_converged_instances_satisfy_oracle(gpu, name):
    ac = make_aircraft(**MODELS[name])
    orc = make_oracle(ac)
    total = conv = 0
    for lateral, V, kw, tg, uh in problem(name):
        res = ac.trim(V, **kw)
        ok = res.converged
        total += len(ok)
        conv += int(ok.sum())
        assert set(np.unique(res.status)) <= {0, 1, 2}
        # every instance, converged or not: the reported residual is the float64 residual at the returned (x, u)
        r_all = T.residual_at(orc, res.x, res.u, res.z, tg, lateral)
        assert (np.abs(res.residual - r_all) <= 1e-3 + 1e-4 * np.abs(r_all)).all(), np.abs(res.residual - r_all).max()
        r = r_all[:, ok]
        print(f"[trim] {name} lateral={lateral}: {ok.sum()}/{len(ok)} converged, status counts "
              f"{np.bincount(res.status, minlength=4).tolist()}, worst float64 |r_v| {np.abs(r[:3]).max(initial=0):.2e} "
              f"|r_w| {np.abs(r[3:]).max(initial=0):.2e}")
        assert np.abs(r[:3]).max(initial=0) <= 1e-3 and np.abs(r[3:]).max(initial=0) <= 1e-3
        # the getters (ac_aero_f32) give back V, beta, psi and the alpha, theta, phi of z
        x = res.x[:, ok]
        if not ok.any():
            continue
        Vg = np.asarray(ac.airspeed(x))
        assert np.abs(Vg / tg[3, ok] - 1).max() <= 1e-5
        be = res.z[5, ok] if lateral else tg[6, ok]
        ang = lambda a, b: np.abs((a - b + np.pi) % (2 * np.pi) - np.pi).max()  # noqa: E731
        assert ang(np.asarray(ac.beta(x)), be) <= 1e-5
        assert ang(np.asarray(ac.psi(x)), tg[4, ok]) <= 1e-5
        assert ang(np.asarray(ac.alpha(x)), res.z[0, ok]) <= 1e-5
        assert ang(np.asarray(ac.theta(x)), res.z[1, ok]) <= 1e-5
        assert ang(np.asarray(ac.phi(x)), res.z[2, ok]) <= 1e-5
    # The synthetic-weight nets (MlpData.synthetic) are random functions, not airframes: they have no steady flight in the
    # bounds, and the float64 restatement finds none either (test_trim_coverage_against_float64).  Every physical model
    # trims most of the grid; the rest are flapped high-speed glides that would need theta below -60 deg (status 2).
    if name not in SYNTHETIC_NETS:
        assert conv >= total // 2, (name, conv, total)


# ---- 2. coverage against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODELS))
def test_trim_coverage_against_float64(gpu, name):
    ac = make_aircraft(**MODELS[name])
    orc = make_oracle(ac)
    need = covered = 0
    worse = []
    for lateral, V, kw, tg, uh in problem(name, seed=1):
        res = ac.trim(V, **kw)
        z0 = T.default_guess(tg[3], tg[5], ac.opts.aircraft_config.glide_ratio)
        lo, hi = ac.trim_bounds(lateral)
        z64, r64, c64 = T.lm(orc, np.float32(z0).astype(np.float64), tg, uh, lateral, lo, hi, iters=200)
        both = c64 & res.converged
        need += int(c64.sum())
        covered += int(both.sum())
        worse += [(lateral, i, res.status[i]) for i in np.where(c64 & ~res.converged)[0]]
        dz = np.abs(res.z[:, both] - z64[:, both])
        assert dz[[0, 1, 2]].max(initial=0) <= 1e-4 and dz[[3, 4]].max(initial=0) <= 1e-3, dz.max(axis=1)
        assert dz[5].max(initial=0) <= (1e-4 if lateral else 1e-3)
    print(f"[trim] {name}: float64 LM converged on {need}; GPU on {covered} of those; GPU worse on {worse}")
    if name in NETS:
        assert covered >= 0.98 * need
    else:
        assert covered == need, worse


# ---- 3. determinism ---------------------------------------------------------------------------------------------------------------
def test_trim_bit_identical_across_batches_and_iterations(gpu):
    import torch

    for name in ("poly", "real_net"):
        ac = make_aircraft(**MODELS[name])
        rng = np.random.default_rng(5)
        N = 4096
        V = torch.tensor(rng.uniform(25, 70, N), dtype=torch.float32, device=gpu)
        psid = torch.tensor(rng.uniform(-0.15, 0.15, N), dtype=torch.float32, device=gpu)
        psi = torch.tensor(rng.uniform(-3, 3, N), dtype=torch.float32, device=gpu)
        full = ac.trim(V, turn_rate=psid, psi=psi)
        again = ac.trim(V, turn_rate=psid, psi=psi)
        for a, b in zip(full.__dict__.values(), again.__dict__.values()):
            assert torch.equal(a, b)
        for n in (1, 63, 64, 65):
            part = ac.trim(V[-n:], turn_rate=psid[-n:], psi=psi[-n:])
            for a, b in zip(full.__dict__.values(), part.__dict__.values()):
                assert torch.equal(a[..., -n:], b)
        longer = ac.trim(V, turn_rate=psid, psi=psi, iters=60)
        c = full.converged
        assert int(c.sum()) > N // 2
        for a, b in zip(full.__dict__.values(), longer.__dict__.values()):
            assert torch.equal(a[..., c], b[..., c])  # frozen after convergence


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------------------
def test_trim_graph_replay(gpu):
    import torch

    for name in ("poly", "real_net"):
        ac = make_aircraft(**MODELS[name])
        V = torch.linspace(25, 70, 512, device=gpu)
        psid = torch.linspace(-0.15, 0.15, 512, device=gpu)
        ref = ac.trim(V, turn_rate=psid)
        ws = ac.trim_workspace(512)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ac.trim(V, turn_rate=psid, ws=ws)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ac.trim(V, turn_rate=psid, ws=ws)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(ref.__dict__.values(), out.__dict__.values()):
            assert torch.equal(a, b)


# ---- 5. steady flight under integration ---------------------------------------------------------------------------------------------
def test_trim_is_steady_under_rollout(gpu):
    ac = make_aircraft("poly")
    orc = make_oracle(ac)
    V = np.linspace(35.0, 60.0, 26)
    res = ac.trim(V)
    ok = res.converged
    assert ok.all(), res.status
    _, A, _, _ = orc.step_sens(res.x, res.u, 0.01)
    stable = np.array([np.abs(np.linalg.eigvals(A[:, :, i])).max() <= 1 + 1e-6 for i in range(len(V))])
    print(f"[trim] poly straight glides 35-60 m/s: {stable.sum()} of {len(V)} trims have no eigenvalue beyond 1 + 1e-6")
    assert stable.sum() >= 1
    x, u = res.x[:, stable], res.u[:, stable]
    Xt = ac.rollout(x, np.repeat(u[None], 100, axis=0), 0.01)

    def body_v(X):
        return T.rot(T.qconj(X[6:10] / np.linalg.norm(X[6:10], axis=0)), X[3:6])

    vb0 = body_v(x)
    for k in range(1, 101):
        assert np.abs(body_v(Xt[k]) - vb0).max() <= 0.05, k
        assert np.abs(Xt[k][10:13] - x[10:13]).max() <= 1e-3, k


# ---- 6. error codes -------------------------------------------------------------------------------------------------------------------
def test_trim_error_codes(gpu):
    import torch

    from aircraft_amd import Quadrotor

    lib = _lib.load()
    ac = make_aircraft("poly")
    ac._sync()
    n = 8
    buf = lambda r: torch.zeros((r, n), device=gpu)  # noqa: E731
    tg, uh, z0, X, U, Z, R = buf(7), buf(7), buf(6), buf(13), buf(7), buf(6), buf(6)
    tg[3] = 40.0
    S = torch.zeros(n, dtype=torch.int32, device=gpu)
    need = C.c_size_t()
    assert lib.ac_trim_workspace_floats(ac._handle, n, C.byref(need)) == 0 and need.value >= n * 350
    ws = torch.zeros(need.value, device=gpu)
    o = _lib.TrimOpts()
    o.lateral, o.tol_v, o.tol_w = 0, 1e-4, 1e-4
    lo, hi = ac.trim_bounds(0)
    o.lo[:], o.hi[:] = list(lo), list(hi)

    def call(h, opts, iters=5, wsn=need.value):
        return lib.ac_trim_f32(h, C.byref(opts), tg.data_ptr(), uh.data_ptr(), z0.data_ptr(), iters, n, X.data_ptr(), U.data_ptr(),
                               Z.data_ptr(), R.data_ptr(), S.data_ptr(), ws.data_ptr(), wsn, None)

    assert call(ac._handle, o) == 0
    torch.cuda.synchronize()
    assert call(ac._handle, o, wsn=need.value - 1) == -6  # AC_ERR_WORKSPACE
    assert call(ac._handle, o, iters=0) == -1  # AC_ERR_BAD_ARG
    bad = _lib.TrimOpts.from_buffer_copy(o)
    bad.lo[1], bad.hi[1] = 0.5, -0.5
    assert call(ac._handle, bad) == -1
    bad = _lib.TrimOpts.from_buffer_copy(o)
    bad.lateral = 2
    assert call(ac._handle, bad) == -1
    q = Quadrotor()
    q._sync()
    assert call(q._handle, o) == -3  # AC_ERR_UNSUPPORTED
    assert lib.ac_trim_workspace_floats(q._handle, n, C.byref(need)) == -3
    torch.cuda.synchronize()


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------
def test_glide_polar_example(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "glide_polar.py"), "--model", "poly", "--speeds", "8"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "best glide" in r.stdout, r.stdout[-2000:]
