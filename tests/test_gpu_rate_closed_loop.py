"""The closed loop with the gains on the previous control (ac_rollout_policy_rate_f32, Policy::Kp in csrc/ac_ilqr.hpp):

    u_k = clip(U_k + alpha k_k + Kx_k (x - Xnom_k) + Kp_k (u_applied_{k-1} - U_{k-1})),   the Kp term zero at k = 0,

on every engine of tests/rollout_matrix.py that has a policy kernel and on every analytic model, B = 20, n_alpha = 3, against the
float64 restatement riccati_rate_ref.forward_rate over the oracle's state_update.  Bar: the project's closed-loop clause — every
instance within 1e-5 at every node, or within 8 x what a one-ulp perturbation of x0 does to the float64 restatement.  Conditions
on the inputs, asserted on the float64 side: a control is clipped (so the POST-clip previous control matters), and the result
with Kp differs from the result with Kp = 0 by more than 100 x the bar."""
import numpy as np
import pytest

from tests import riccati_rate_ref as rr
from tests.helpers import check_against_conditioning, f32_exact, instance_err, parity_report
from tests.test_gpu_rollout_engines import (CLOSED_IDS, CLOSED_SEEDS, DT, STATE_TOL, closed_loop_problem, context, control_box,
                                            dev, f64, one_step_error)

pytestmark = pytest.mark.gpu

B, NA = 20, 3


def draw_kp(H, seed):
    """as closed_loop_problem draws K: 0.3 N(0, 1), fp32-exact"""
    return f32_exact(0.3 * np.random.default_rng(seed).standard_normal((H, 7, 7, B)))


def conditioning_rate(orc, cost, X0, Xnom, U, K, Kp, kff, alphas, eps=1e-7, draws=3, seed=0):
    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        Xr, Ur, clipped = rr.forward_rate(orc, cost, X0, Xnom, U, K, Kp, kff, alphas, DT)
        worst = np.zeros(Xr.shape[-1])
        for _ in range(draws):
            Xp, _, _ = rr.forward_rate(orc, cost, X0 * (1.0 + eps * rng.choice([-1.0, 1.0], X0.shape)), Xnom, U, K, Kp, kff, alphas, DT)
            worst = np.maximum(worst, np.nan_to_num(instance_err(Xp, Xr), nan=np.inf))
    return Xr, Ur, clipped, worst


@pytest.mark.parametrize("key", CLOSED_IDS)
def test_closed_loop_with_previous_control_gains(gpu, key):
    import torch
    from aircraft_amd.control import ILQR, QuadraticCost

    c = context(key)
    ac, orc, H, row = c["ac"], c["orc"], c["H"], c["row"]
    lo, hi = control_box(key)
    il = ILQR(system=ac, dt=DT, num_nodes=H, cost=QuadraticCost(u_min=lo, u_max=hi))
    X0, U, K, kff, alphas = closed_loop_problem(c, B, NA, CLOSED_SEEDS[(B, NA)])
    Kp = draw_kp(H, 977)
    Ud, X0d, Kd, kd = dev(U, gpu), dev(X0, gpu), dev(K, gpu), dev(kff, gpu)
    Xnom_d = ac.rollout(X0d, Ud, DT)
    Xc, Uc = il.forward(X0d, Xnom_d, Ud, Kd, kd, alphas=alphas, Kp=dev(Kp, gpu))
    launch = ac.last_launch()
    assert launch[0] == (row.policy_kernel if row else "k_rollout_policy"), launch
    again = il.forward(X0d, Xnom_d, Ud, Kd, kd, alphas=alphas, Kp=dev(Kp, gpu))
    assert torch.equal(again[0], Xc) and torch.equal(again[1], Uc), "a repeat of the call differs"
    # Kp = 0 is ac_rollout_policy_f32, bit for bit
    plain = il.forward(X0d, Xnom_d, Ud, Kd, kd, alphas=alphas)
    zero = il.forward(X0d, Xnom_d, Ud, Kd, kd, alphas=alphas, Kp=torch.zeros((H, 7, 7, B), device=gpu))
    assert torch.equal(zero[0], plain[0]) and torch.equal(zero[1], plain[1]), "Kp = 0 differs from ac_rollout_policy_f32"
    Xc, Uc, Xnom = f64(Xc), f64(Uc), f64(Xnom_d)
    assert Xc.shape == (H + 1, 13, NA * B) and np.isfinite(Xc).all() and np.isfinite(Uc).all()
    assert np.array_equal(Xc[0], np.tile(X0, (1, NA)))
    assert (Uc >= np.asarray(lo)[:, None]).all() and (Uc <= np.asarray(hi)[:, None]).all()
    # float64 side: the reference, its conditioning, and the two conditions on the inputs
    Xr, Ur, clipped, cond = conditioning_rate(orc, il.cost, X0, Xnom, U, K, Kp, kff, alphas)
    X0r, _, _ = rr.forward_rate(orc, il.cost, X0, Xnom, U, K, None, kff, alphas, DT)
    bar = np.maximum(STATE_TOL, 8.0 * cond)
    effect = instance_err(Xr, X0r)
    rows = slice(0, 4) if key == "quad" else slice(0, 3)
    moving = ((Ur[:, rows] > np.asarray(lo)[rows][:, None]) & (Ur[:, rows] < np.asarray(hi)[rows][:, None])).mean()
    clipped = clipped[rows].any(axis=0)   # on the rows that move (the others are pinned by a box of zero width)
    name = f"policy_rate[{key}-{B}x{NA}]"
    parity_report(name, kernel=launch[0], clipped_instances=int(clipped.sum()), inside=float(moving), kp_effect_max=float(effect.max()),
                  bar_max=float(bar.max()), reference_deviation_max=float(cond.max()), one_step_max=one_step_error(orc, Xc, Uc))
    assert clipped.any() and moving > 0.5, (name, "the clip is not exercised", int(clipped.sum()), float(moving))
    assert effect.max() > 100.0 * bar.max(), (name, "Kp does not matter on these inputs", float(effect.max()), float(bar.max()))
    assert one_step_error(orc, Xc, Uc) < STATE_TOL
    err, _ = check_against_conditioning(name + "[chained]", Xc, Xr, cond, STATE_TOL)
    print(f"{name} kernel {launch[0]} worst {err.max():.2e} cond {cond.max():.2e} Kp effect {effect.max():.2e} clipped {int(clipped.sum())}/{NA * B}")
    # the plain law is NOT what ran: the GPU result sits with the Kp reference, not with the Kp = 0 one
    assert instance_err(Xc, X0r).max() > 50.0 * bar.max()
