"""The solver with the control-rate term modelled exactly: ILQR(rate_weight=) and GoalAcquisition(rate="exact") on the `default`
model, B = 8, H = 12.

 * one `iterate` with alphas = [1.0] against a float64 restatement of the same sweep — the oracle's linearisation, the float64
   rate recursion, the float64 closed loop and the float64 cost (tests/riccati_rate_ref.py) — under the closed-loop clause:
   the accepted cost of every instance within 1e-5, or within 8 x what a one-ulp perturbation of x0 does to the restatement;
 * cost histories never increase; rate="frozen" is the solver built without the argument, bit for bit;
 * the sweep with rate_weight captured into a graph replays to the eager result."""
import numpy as np
import pytest

import ilqr_oracle as io
from tests import riccati_rate_ref as rr
from tests.helpers import block_rel_err, f32_exact, make_aircraft, make_oracle, near_trim_problem, parity_report

pytestmark = pytest.mark.gpu

B, H = 8, 12
DT = float(np.float32(0.01))
RATE_W = [4000.0, 4000.0, 4000.0, 0.0, 0.0, 0.0, 100.0]


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def problem():
    """Gliders near trim at 20 .. 26 m/s (where explicit RK4 with dt = 0.01 is inside its stability region for the default
    model's pitch damping), perturbed surface deflections that differ from node to node, a previous control per instance."""
    X0, U = near_trim_problem(B, H, seed=6)
    V = np.linalg.norm(X0[3:6], axis=0)
    X0[3:6] *= (20.0 + 6.0 * (V - V.min()) / max(V.max() - V.min(), 1e-9)) / V
    rng = np.random.default_rng(12)
    U = U + rng.normal(0, 0.1, U.shape) * (np.arange(7) < 3)[None, :, None]
    up = U[0] + rng.normal(0, 0.1, (7, B)) * (np.arange(7) < 3)[:, None]
    return f32_exact(X0), f32_exact(U), f32_exact(up)


def quad_cost():
    from aircraft_amd.control import QuadraticCost

    T = H * DT
    cost = QuadraticCost.goal((23.0 * T, 0.2), w_goal=1.0, height=-200.0, w_height=1.0, w_lateral_speed=0.5, r=0.5, reg=1.0)
    cost.q = [0, 0, 1e-2, 0, 0, 0, 0, 0, 0, 0, 0.2, 0.2, 0.2]
    cost.x_ref = [0, 0, -200.0] + [0] * 10
    return cost


def sweep_f64(orc, cost, w, x0, U, up):
    """One sweep with alpha = 1 in float64 -> (accepted cost (B,), cost of the iterate (B,), candidate cost (B,))"""
    X = orc.rollout(x0, U, DT)
    flat = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2).reshape(a.shape[1], -1))  # noqa: E731
    _, A, Bm, _ = orc.step_sens(flat(X[:-1]), flat(U), DT)
    A = A.reshape(13, 13, H, B).transpose(2, 0, 1, 3); Bm = Bm.reshape(13, 7, H, B).transpose(2, 0, 1, 3)
    g, h = rr.quad_rate_model(np.float64, w, U, up)
    K, Kp, kff, dV, _ = rr.backward_rate_np(np.float64, cost, X, U, A, Bm, g, h)
    Xc, Uc, _ = rr.forward_rate(orc, cost, x0, X, U, K, Kp, kff, [1.0], DT)
    J0 = io.cost(cost, X, U) + rr.quad_rate_cost(np.float64, w, U, up)
    Jc = io.cost(cost, Xc, Uc) + rr.quad_rate_cost(np.float64, w, Uc, up)
    ok = np.isfinite(Jc) & (Jc < J0)
    return np.where(ok, Jc, J0), J0, Jc, dV


def test_one_sweep_matches_the_float64_restatement(gpu):
    from aircraft_amd.control import ILQR

    ac = make_aircraft("default", normalise=True)
    orc = make_oracle(ac)
    cost = quad_cost()
    X0, U, up = problem()
    il = ILQR(system=ac, dt=DT, num_nodes=H, cost=cost, alphas=[1.0], rate_weight=RATE_W)
    assert il.rate_weight == RATE_W
    Xd, Ud, hist = il.solve(dev(X0, gpu), dev(U, gpu), iters=1, u_prev=dev(up, gpu))
    assert ac.last_launch()[0] == "k_ilqr_accept"
    h = hist.cpu().numpy().astype(np.float64)
    Ja, J0, Jc, dV = sweep_f64(orc, cost, RATE_W, X0, U, up)
    rng = np.random.default_rng(0)
    devn = np.zeros(B)
    for _ in range(3):
        Jp = sweep_f64(orc, cost, RATE_W, X0 * (1.0 + 1e-7 * rng.choice([-1.0, 1.0], X0.shape)), U, up)[0]
        devn = np.maximum(devn, np.abs(Jp - Ja) / np.abs(Ja))
    bar = np.maximum(1e-5, 8.0 * devn)
    e0, e1 = np.abs(h[0] - J0) / np.abs(J0), np.abs(h[1] - Ja) / np.abs(Ja)
    parity_report("rate_sweep[default]", worst_iterate=float(e0.max()), worst_accepted=float(e1.max()), bar_max=float(bar.max()),
                  reference_deviation_max=float(devn.max()), improved=int((Jc < J0).sum()), decrease_min=float(((J0 - Ja) / J0).min()))
    print(f"rate_sweep: iterate {e0.max():.2e} accepted {e1.max():.2e} bar {bar.max():.2e} decrease {((J0 - Ja) / J0).min():.2e} .. {((J0 - Ja) / J0).max():.2e}")
    # conditions on the float64 side: the step is accepted on every instance and the rate term is a real part of the objective
    assert (Jc < J0).all() and ((J0 - Ja) / J0).min() > 1e-3
    assert (rr.quad_rate_cost(np.float64, RATE_W, U, up) > 1e-2 * J0).all()
    assert (e0 <= 1e-5).all(), ("cost of the iterate", e0)
    assert (e1 <= bar).all(), ("accepted cost", e1, bar)
    # the accepted pair is dynamically consistent, and the rate term is in trajectory_cost
    assert block_rel_err(Xd.cpu().numpy(), il.rollout(dev(X0, gpu), Ud).cpu().numpy()) < 1e-5
    plain = ILQR(system=ac, dt=DT, num_nodes=H, cost=cost, alphas=[1.0])
    il._u_prev = None
    diff = (il.trajectory_cost(Xd, Ud) - plain.trajectory_cost(Xd, Ud)).cpu().numpy()
    want = rr.quad_rate_cost(np.float64, RATE_W, Ud.cpu().numpy().astype(np.float64))
    assert np.abs(diff - want).max() <= 1e-4 * np.abs(h[1]).max()


def test_histories_never_increase(gpu):
    """The line search accepts only improvements of the exact objective (1e-6: the slack of tests/test_gpu_ilqr.py)."""
    import torch
    from aircraft_amd.control import ILQR, GoalAcquisition

    ac = make_aircraft("default", normalise=True)
    X0, U, up = problem()
    il = ILQR(system=ac, dt=DT, num_nodes=H, cost=quad_cost(), rate_weight=RATE_W)
    X, Uo, hist = il.solve(dev(X0, gpu), dev(U, gpu), iters=6, u_prev=dev(up, gpu))
    h = hist.cpu().numpy()
    assert h.shape == (7, B) and np.isfinite(h).all() and bool(torch.isfinite(X).all())
    assert (np.diff(h, axis=0) <= 1e-6 * np.abs(h[:-1]) + 1e-6).all()
    assert (h[-1] < h[0]).all()
    rng = np.random.default_rng(12)
    goal = f32_exact(np.stack([rng.uniform(2.5, 3.2, B), rng.uniform(-0.3, 0.3, B)]))
    hs = {}
    for name, kw in (("exact", dict(rate="exact")), ("frozen", dict(rate="frozen")), ("default", dict())):
        ga = GoalAcquisition(system=ac, goal=goal, dt=DT, num_nodes=H, vx_max=25.0, w_al=4.0, alphas=(1.0, 0.5, 0.1), reg=1.0, **kw)
        Xg, Ug, hg = ga.solve(dev(X0, gpu), dev(U, gpu), iters=6)
        hs[name] = hg
        hh = hg.cpu().numpy()
        assert np.isfinite(hh).all() and bool(torch.isfinite(Xg).all())
        assert (np.diff(hh, axis=0) <= 1e-6 * np.abs(hh[:-1]) + 1e-6).all(), name
        print(f"goal[{name}] first {hh[0].mean():.4e} last {hh[-1].mean():.4e}")
    assert torch.equal(hs["frozen"], hs["default"]), "rate='frozen' is not the solver built without the argument"
    assert not torch.equal(hs["exact"], hs["frozen"])
    assert (hs["exact"][-1] < hs["exact"][0]).float().mean() > 0.5


def test_sweep_with_rate_weight_is_graph_capturable(gpu):
    from aircraft_amd.control import ILQR, RecedingHorizon

    ac = make_aircraft("default", normalise=True)
    X0, U, _ = problem()
    il = ILQR(system=ac, dt=DT, num_nodes=H, cost=quad_cost(), alphas=(1.0, 0.5, 0.1), rate_weight=RATE_W)
    U0 = dev(U, gpu)
    he = RecedingHorizon(il, overlap=8, iterations=2).allocate(dev(X0, gpu), U0).run(3, record=True)
    hg = RecedingHorizon(il, overlap=8, iterations=2).allocate(dev(X0, gpu), U0).capture().run(3, record=True)
    assert he.shape == (3 * 4 + 1, 13, B)
    assert block_rel_err(hg.cpu().numpy(), he.cpu().numpy()) < 1e-6
