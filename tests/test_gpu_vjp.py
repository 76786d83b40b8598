"""GPU tests of the reverse mode (ac_step_vjp_f32, ac_rollout_vjp_f32, ac_state_derivative_vjp_f32) and of
aircraft_amd.autodiff: per-unit VJPs against the float64 oracle's exact Jacobians, the rollout's reverse recurrence against
a float64 chain of those Jacobians at the GPU's own saved nodes, fused route against composed route, autograd end to end,
determinism and hipGraph capture, and the differentiable-rollout example."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import ROOT, f32_exact, make_aircraft, make_oracle, parity_report, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

MODELS = {  # name -> make_aircraft arguments
    "default": dict(model="default", stall_scaling=True),
    "linear": dict(model="linear"),
    "poly": dict(model="poly"),
    "real_net": dict(model="nn"),
    "net_3x64": dict(model="nn", hidden=(64, 64, 64)),
    "net_4x128": dict(model="nn", hidden=(128, 128, 128, 128)),
}


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def make(name, substeps=1, normalise=True):
    if name == "quad":
        from aircraft_amd import Quadrotor
        from oracle import Oracle

        q = Quadrotor()
        q.physical_integration_substeps = substeps
        q.normalise = normalise
        return q, Oracle(q.airframe_dict(), "quad", None, substeps=substeps, normalise=normalise, epsilon=q.epsilon,
                         gravity=q.gravity)
    ac = make_aircraft(substeps=substeps, normalise=normalise, **MODELS[name])
    return ac, make_oracle(ac)


def units(name, n, seed):
    if name == "quad":
        from tests.test_gpu_quadrotor import quad_units

        X, U4 = quad_units(n, seed=seed)
        U = np.zeros((7, n)); U[:4] = U4
    else:
        X, U = synthetic_units(n, seed=seed, flaps=True)
        X, U = f32_exact(X), f32_exact(U)
    lam = f32_exact(np.random.default_rng(seed + 1).normal(size=(13, n)))
    return X, U, lam


def oracle_step_vjp(orc, X, U, dt, lam, nc):
    _, A, B, c = orc.step_sens(X, U, dt)
    J = np.concatenate([A, B[:, :nc], c[:, None, :]], axis=1)
    return np.einsum("in,izn->zn", lam, J)


# ---- 1. step VJP against the oracle, per unit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("name", list(MODELS) + ["quad"])
def test_step_vjp_matches_oracle_per_unit(gpu, name, substeps):
    ac, orc = make(name, substeps=substeps)
    nc = ac.num_controls
    errs = []
    for n, seed in ((1, 1), (63, 2), (64, 3), (65, 4), (130, 5), (4096, 6)):
        X, U, lam = units(name, n, seed)
        dt = 0.01 if n != 130 else f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, n))  # per-unit dt
        dtd = dev(dt, gpu) if np.ndim(dt) else dt
        Xb, Ub, db = ac.step_vjp(dev(X, gpu), dev(U[:nc], gpu), dtd, dev(lam, gpu))
        got = np.concatenate([host(Xb), host(Ub), host(db)[None]], axis=0)
        want = oracle_step_vjp(orc, X, U, dt, lam, nc)
        err = unit_max_rel(got, want)
        errs.append(err)
        assert np.array_equal(host(Xb)[:3], lam[:3])  # p never enters f: x_bar[0..2] = lam[0..2]
    fused = name in ("default", "linear", "poly")
    assert ac.last_launch()[0] == ("k_step_vjp" if fused else "k_vjp_contract")
    err = np.concatenate(errs)
    parity_report("step_vjp", model=name, substeps=substeps, worst_unit_max_rel=float(err.max()),
                  frac_2e5=float((err < 2e-5).mean()), units=int(err.size))
    assert check_unit_bars(err, fused)


def check_unit_bars(err, fused):
    """Composed route: every unit < 2e-5.  Fused route (the reverse sweep in fp32): every unit < 1e-4 and >= 99 % < 2e-5 —
    measured worst 8.4e-5 on 1 of 4096 random units."""
    if not fused:
        assert err.max() < 2e-5, (int(err.argmax()), float(err.max()))
        return True
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert (err < 2e-5).mean() >= 0.99, float((err < 2e-5).mean())
    return True


@pytest.mark.parametrize("name", ["default", "poly", "real_net", "quad"])
def test_state_derivative_vjp_matches_oracle(gpu, name):
    ac, orc = make(name)
    nc = ac.num_controls
    X, U, w = units(name, 777, 11)
    Xb, Ub = ac.state_derivative_vjp(dev(X, gpu), dev(U[:nc], gpu), dev(w, gpu))
    _, Fx, Fu = orc.state_derivative_sens(X, U)
    want = np.einsum("in,izn->zn", w, np.concatenate([Fx, Fu[:, :nc]], axis=1))
    err = unit_max_rel(np.concatenate([host(Xb), host(Ub)]), want)
    assert check_unit_bars(err, name in ("default", "poly"))
    assert not host(Xb)[:3].any()


# ---- 2. rollout VJP against a float64 chain at the GPU's own nodes ------------------------------------------------------------
ROLLOUT_DT = {"default": 0.002, "linear": 0.002}  # (their crude fits leave RK4's stability region at dt = 0.01 near trim)


def rollout_problem(name, B, H, seed, gpu, substeps=1):
    """-> ac, oracle, the GPU's trajectory (H+1, 13, B), U, cotangent G, dt"""
    import torch

    from tests.helpers import near_trim_problem

    ac, orc = make(name, substeps=substeps)
    X0, U = near_trim_problem(B, H, seed=seed)  # trajectories that stay inside the flight envelope
    U = f32_exact(U)
    rng = np.random.default_rng(seed)
    dt = ROLLOUT_DT.get(name, 0.01)
    Xtraj = ac.rollout(dev(f32_exact(X0), gpu), dev(U, gpu), dt)
    G = f32_exact(rng.normal(size=(H + 1, 13, B)) * 1e-2)
    torch.cuda.synchronize()
    return ac, orc, Xtraj, U, G, dt


def chain_vjp(orc, Xn, U, G, dt):
    """float64 reverse recurrence with the oracle's exact Jacobians at the nodes Xn (H+1, 13, B)"""
    H1, _, B = Xn.shape
    H = H1 - 1
    _, A, Bm, c = orc.step_sens(Xn[:H].transpose(1, 0, 2).reshape(13, H * B), U.transpose(1, 0, 2).reshape(7, H * B), dt)
    A = A.reshape(13, 13, H, B); Bm = Bm.reshape(13, 7, H, B); c = c.reshape(13, H, B)
    lam = G[H].copy(); Ub = np.zeros((H, 7, B)); db = np.zeros(B)
    for k in range(H - 1, -1, -1):
        Ub[k] = np.einsum("ib,ijb->jb", lam, Bm[:, :, k])
        db += np.einsum("ib,ib->b", lam, c[:, k])
        lam = G[k] + np.einsum("ib,ijb->jb", lam, A[:, :, k])
    return lam, Ub, db


def instance_rel(got, want):
    """per instance: max |got - want| / max |want| over x0_bar, every node's u_bar and dt_bar"""
    g = np.concatenate([got[0], got[1].transpose(1, 0, 2).reshape(-1, got[0].shape[1]), got[2][None]])
    w = np.concatenate([want[0], want[1].transpose(1, 0, 2).reshape(-1, want[0].shape[1]), want[2][None]])
    return unit_max_rel(g, w)


@pytest.mark.parametrize("name", ["poly", "default", "real_net"])
def test_rollout_vjp_matches_float64_chain(gpu, name):
    from tests.helpers import conditioning

    B, H = 256, 20
    ac, orc, Xtraj, U, G, dt = rollout_problem(name, B, H, seed=61, gpu=gpu)
    x0b, ub, db = ac.rollout_vjp(Xtraj, dev(U, gpu), dt, dev(G, gpu))
    got = (host(x0b), host(ub), host(db))
    want = chain_vjp(orc, host(Xtraj), U, G, dt)
    err = instance_rel(got, want)
    parity_report("rollout_vjp", model=name, worst=float(err.max()), p99=float(np.quantile(err, 0.99)),
                  frac_2e5=float((err < 2e-5).mean()))
    assert np.isfinite(want[0]).all()
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert (err < 2e-5).mean() >= 0.98
    loose = np.flatnonzero(err >= 2e-5)
    if loose.size:  # the instances outside 2e-5 go on record with how much a one-ulp perturbation of x0 moves the reference
        _, cond = conditioning(orc, host(Xtraj)[0][:, loose], U[:, :, loose], dt)
        parity_report("rollout_vjp_loose", model=name, instances=loose.tolist(), err=err[loose].tolist(), conditioning=cond.tolist())
    assert ac.last_launch()[0] == ("k_vjp_recur" if name == "real_net" else "k_rollout_vjp")


@pytest.mark.parametrize("substeps", [1, 3])
def test_rollout_vjp_ragged_tile_and_substeps(gpu, substeps):
    """B = 70: two tiles, the second of 6 instances; three sub-steps per node through the LDS column."""
    ac, orc, Xtraj, U, G, dt = rollout_problem("poly", 70, 3, seed=63, gpu=gpu, substeps=substeps)
    x0b, ub, db = ac.rollout_vjp(Xtraj, dev(U, gpu), dt, dev(G, gpu))
    assert ac.last_launch()[:2] == ("k_rollout_vjp", 2)
    want = chain_vjp(orc, host(Xtraj), U, G, dt)
    err = instance_rel((host(x0b), host(ub), host(db)), want)
    parity_report("rollout_vjp_ragged", model="poly", substeps=substeps, worst=float(err.max()), frac_2e5=float((err < 2e-5).mean()))
    assert err.max() < 1e-4, (int(err.argmax()), float(err.max()))
    assert (err < 2e-5).mean() >= 0.98


@pytest.mark.parametrize("name", ["poly", "real_net"])
def test_rollout_vjp_zero_horizon(gpu, name):
    """H = 0 on the fused and the composed route: X[0] = x0, the cotangent passes through and dt does not enter."""
    import torch

    ac, _ = make(name)
    X = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    G = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    x0b, ub, db = ac.rollout_vjp(X, torch.zeros((0, 7, 70), device=gpu), 0.01, G)
    assert torch.equal(x0b, G[0]) and ub.shape == (0, ac.num_controls, 70) and not db.any()


# ---- 3. fused route equals composed route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("name", ["default", "linear", "poly"])
def test_fused_route_equals_composed_route(gpu, name, substeps):
    ac, _ = make(name, substeps=substeps)
    X, U, lam = units(name, 1000, 71)
    args = (dev(X, gpu), dev(U, gpu), 0.01, dev(lam, gpu))
    ac.vjp_route = "fused"
    fused = [host(t) for t in ac.step_vjp(*args)]
    assert ac.last_launch()[0] == "k_step_vjp"
    ac.vjp_route = "composed"
    comp = [host(t) for t in ac.step_vjp(*args)]
    assert ac.last_launch()[0] == "k_vjp_contract"
    err = unit_max_rel(np.concatenate([fused[0], fused[1], fused[2][None]]), np.concatenate([comp[0], comp[1], comp[2][None]]))
    parity_report("vjp_fused_vs_composed", model=name, substeps=substeps, worst=float(err.max()))
    assert check_unit_bars(err, True)
    if substeps == 1:
        B, H = 128, 12
        ac2, _, Xtraj, U2, G, dt = rollout_problem(name, B, H, seed=72, gpu=gpu)
        r = {}
        for route in ("fused", "composed"):
            ac2.vjp_route = route
            r[route] = [host(t) for t in ac2.rollout_vjp(Xtraj, dev(U2, gpu), dt, dev(G, gpu))]
        assert check_unit_bars(instance_rel(r["fused"], r["composed"]), True)


def test_forced_fused_route_refused_for_mlp(gpu):
    from aircraft_amd import AircraftHipError

    ac, _ = make("real_net")
    X, U, lam = units("real_net", 8, 1)
    ac.vjp_route = "fused"
    with pytest.raises(AircraftHipError, match="UNSUPPORTED"):
        ac.step_vjp(dev(X, gpu), dev(U, gpu), 0.01, dev(lam, gpu))
    ac.vjp_route = "composed"
    ws = ac.vjp_workspace("step", 8)
    from aircraft_amd import _lib
    import ctypes as C
    import torch

    small = torch.empty(10, device=gpu)
    rc = _lib.load().ac_step_vjp_f32(ac._handle, dev(X, gpu).data_ptr(), dev(U, gpu).data_ptr(), C.c_float(0.01), None, 8,
                                     dev(lam, gpu).data_ptr(), small.data_ptr(), small.data_ptr(), None, small.data_ptr(), 10,
                                     None)
    assert rc == -6 and ws.numel() == 8 * 286


# ---- 4. autograd end to end -----------------------------------------------------------------------------------------------------
def test_autograd_rollout_and_step_equal_explicit_wrappers(gpu):
    import torch

    from aircraft_amd import autodiff

    for name in ("poly", "real_net"):
        ac, orc, Xtraj, U, G, dt0 = rollout_problem(name, 64, 10, seed=81, gpu=gpu)
        x0 = Xtraj[0].clone().requires_grad_(True)
        Ut = dev(U, gpu).requires_grad_(True)
        dt = torch.tensor(0.01, device=gpu, requires_grad=True)
        X = autodiff.rollout(ac, x0, Ut, dt)
        assert X.grad_fn is not None and torch.equal(X.detach(), Xtraj)
        Gt = dev(G, gpu)
        gx0, gU, gdt = torch.autograd.grad((X * Gt).sum(), (x0, Ut, dt))
        x0b, ub, db = ac.rollout_vjp(Xtraj, dev(U, gpu), 0.01, Gt)
        assert torch.equal(gx0, x0b) and torch.equal(gU, ub) and torch.equal(gdt, db.sum())
        # step, per-unit dt
        x = Xtraj[3].clone().requires_grad_(True)
        u = dev(U[3], gpu).requires_grad_(True)
        dts = torch.full((64,), 0.01, device=gpu).requires_grad_(True)
        y = autodiff.step(ac, x, u, dts)
        lam = torch.randn_like(y)
        gx, gu, gd = torch.autograd.grad((y * lam).sum(), (x, u, dts))
        xb, ub1, db1 = ac.step_vjp(x.detach(), u.detach(), dts.detach(), lam)
        assert torch.equal(gx, xb) and torch.equal(gu, ub1) and torch.equal(gd, db1)
        # state_derivative
        xd = autodiff.state_derivative(ac, x, u)
        w = torch.randn_like(xd)
        gx2, gu2 = torch.autograd.grad((xd * w).sum(), (x, u))
        xb2, ub2 = ac.state_derivative_vjp(x.detach(), u.detach(), w)
        assert torch.equal(gx2, xb2) and torch.equal(gu2, ub2)


def test_autograd_needs_input_grad_dtype_and_double_backward(gpu):
    import torch

    from aircraft_amd import autodiff

    ac, _ = make("poly")
    X, U, _ = units("poly", 32, 91)
    x = torch.from_numpy(X).to(gpu)                       # float64 in: float64 out and float64 gradients
    u = torch.from_numpy(U).to(gpu).requires_grad_(True)
    y = autodiff.step(ac, x, u, 0.01)
    assert y.dtype == torch.float64 and y.requires_grad
    (gu,) = torch.autograd.grad(y.sum(), (u,))
    assert gu.dtype == torch.float64 and gu.shape == u.shape
    x.requires_grad_(True)
    y = autodiff.step(ac, x, u.detach(), 0.01)
    gx, gu2 = torch.autograd.grad(y.sum(), (x, u), allow_unused=True)
    assert gx is not None and gu2 is None
    Ut = torch.from_numpy(np.repeat(U[None], 5, axis=0)).float().to(gpu).requires_grad_(True)
    Xr = autodiff.rollout(ac, x.detach().float(), Ut, 0.01)
    g = torch.autograd.grad(Xr[-1].pow(2).sum(), Ut, create_graph=True)[0]
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---- 5. determinism and graph capture ------------------------------------------------------------------------------------------
def test_vjp_repeats_bit_identical_and_graph_capture(gpu):
    import torch

    for name in ("poly", "real_net"):
        ac, _, Xtraj, U, G, _ = rollout_problem(name, 256, 8, seed=101, gpu=gpu)
        Ud, Gd = dev(U, gpu), dev(G, gpu)
        ref = ac.rollout_vjp(Xtraj, Ud, 0.01, Gd)
        again = ac.rollout_vjp(Xtraj, Ud, 0.01, Gd)
        assert all(torch.equal(a, b) for a, b in zip(ref, again))
        ws = ac.vjp_workspace("rollout", 256, 8)  # the composed route's workspace: allocated before the capture
        assert (ws is None) == (name == "poly")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ac.rollout_vjp(Xtraj, Ud, 0.01, Gd, ws=ws)  # warm-up on the capture stream
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = ac.rollout_vjp(Xtraj, Ud, 0.01, Gd, ws=ws)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, out))


# ---- 6. the example ---------------------------------------------------------------------------------------------------------------
def test_differentiable_rollout_example_reduces_loss(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "differentiable_rollout.py"), "--batch", "64", "--iters", "30"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    losses = [float(line.split("loss=")[1].split()[0]) for line in r.stdout.splitlines() if "loss=" in line]
    assert len(losses) == 30 and np.all(np.isfinite(losses))
    assert losses[-1] < 0.9 * losses[0], losses
