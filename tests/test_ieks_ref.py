"""The float64 restatement of the iterated extended Kalman smoother (tests/ieks_ref.py) pinned by properties, so that the parity
tests compare against something that is itself checked: the pass plus smoother is the Gauss-Newton step of the MAP cost to first
order (against the dense linearised least-squares problem, at two scales); a noise-free log about its own truth is a fixed point;
the iteration descends on the chains of every fixed-wing model and ends below the EKF + RTS trajectory, with decisions whose
margins a float32 cost cannot overturn; mutated restatements fail; the distance of the converged trajectory from exact
stationarity.  No GPU and no host build here."""
import numpy as np
import pytest

from tests import ekf_ref as E
from tests import ieks_ref as I

GN_SCALES = (0.5, 0.25)
MUTATIONS = ("drop_c", "at_prediction", "no_q", "d0_zero")


# ---- 1. the Gauss-Newton step ------------------------------------------------------------------------------------------------------
def gauss_newton_check(pass_fn, name):
    big, small = (I.gn_mismatch(pass_fn, I.gn_case(name, s)) for s in GN_SCALES)
    print(f"[ieks gn] {name}: {big} -> {small}")
    assert (small < big).all(), (big, small)
    assert ((big / small >= 1.5) & (big / small <= 2.5)).all(), big / small


@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_pass_and_smoother_are_the_gauss_newton_step(name):
    """T = 3: X^s [-] Xbar equals the solution of the dense linearised problem (prior, process and measurement rows in the
    deviations of all 4 nodes) to first order: the relative mismatch halves when every deviation is halved (theory: ratio 2)."""
    gauss_newton_check(I.pass_, name)


# ---- 3. the fixed point ------------------------------------------------------------------------------------------------------------
def fixed_point_case(name, T_=5, m=4):
    d = E.chain_inputs(name, T_=T_)
    cut = lambda a: a[..., :m]  # noqa: E731
    orc, u, eps = d["orc"], cut(d["u"]), d["eps"]
    X = [cut(d["truth"])]
    for _ in range(T_):
        X.append(orc.state_update(X[-1], u, E.DT))
    X = np.stack(X)
    Z = np.stack([E.h(x, E.MAG, eps) for x in X[1:]])
    return dict(orc=orc, eps=eps, X0=X[0], P0=cut(d["P"]), Xbar=X, U=np.repeat(u[None], T_, axis=0), Z=Z, Qd=cut(d["Qd"]), Rd=cut(d["Rd"]))


def fixed_point_check(name, **mut):
    """noise-free Z from an exact rollout, prior mean = truth, nominal = truth: J and the step are at rounding level"""
    c = fixed_point_case(name)
    r = I.solve(c["orc"], c["X0"], c["P0"], c["Xbar"], c["U"], c["Z"], None, c["Qd"], c["Rd"], 1, eps=c["eps"], **mut)
    F, A = I.linearise(c["orc"], c["Xbar"], c["U"])
    sm = I.smooth(I.pass_(c["X0"], c["P0"], c["Xbar"], F, A, c["Z"], None, c["Qd"], c["Rd"], E.MAG, c["eps"], **mut))
    Xs, Ps = I.nodes(sm), np.concatenate([sm["P0"][None], sm["P"]])
    step = np.stack([E.boxminus(Xs[k], c["Xbar"][k]) for k in range(Xs.shape[0])])
    sd = np.sqrt(Ps[:, np.arange(12), np.arange(12)])
    print(f"[ieks fixed point] {name}: J {r['cost'][0].max():.2e}, step/sigma {np.abs(step / sd).max():.2e}, alpha {np.unique(r['alpha'])}")
    # float64: 1e-16 relative on positions of 1e2 - 1e3 m against sigmas of 1e-2 m is 1e-11 sigma; squared and summed, J < 1e-18
    assert r["cost"][0].max() < 1e-16
    assert np.abs(step / sd).max() < 1e-8
    assert (r["cost"][1] <= r["cost"][0]).all() and r["cost"][1].max() < 1e-16
    assert (((r["status"] & I.NO_DECREASE) != 0) | (r["alpha"][0] > 0)).all()


@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_truth_of_a_noise_free_log_is_a_fixed_point(name):
    fixed_point_check(name)


# ---- 4. descent --------------------------------------------------------------------------------------------------------------------
_SOLVED = {}


def solved(name, **mut):
    key = (name, tuple(sorted(mut)))
    if key not in _SOLVED:
        d = I.descent_inputs(name)
        _SOLVED[key] = I.solve(d["orc"], d["X0"], d["P"], d["Xfilt"], d["U"], d["Z"], d["masks"], d["Qd"], d["Rd"], I.DESCENT_ITERS,
                               eps=d["eps"], **mut)
    return _SOLVED[key]


def descent_check(name, **mut):
    d, r = I.descent_inputs(name), solved(name, **mut)
    c = r["cost"]
    Jekf = I.cost(d["X0"], d["P"], d["Xekf"], I.images(d["orc"], d["Xekf"], d["U"]), d["Z"], d["masks"], d["Qd"], d["Rd"], E.MAG, d["eps"])["J"]
    print(f"[ieks descent] {name}: J {c[0].max():.3e} -> {c[-1].max():.3e} (EKF + RTS {Jekf.max():.3e}); alpha {[np.unique(a).tolist() for a in r['alpha']]}; "
          f"least margin / J(0) {(r['margin'] / c[:-1]).min(1)}")
    assert (np.diff(c, axis=0) <= 0).all()
    assert (r["alpha"][0] > 0).all()
    assert (c[-1] < Jekf).all()
    assert (r["status"] == 0).all()
    # no decision of the reference is within reach of a float32 cost (the GPU test leaves such instances out: none here)
    assert (r["margin"] >= 1e-4 * c[:-1]).all()


@pytest.mark.parametrize("name", E.MODELS)
def test_iteration_descends_below_the_ekf_rts_trajectory(name):
    """x0 offset by 3 sigma of a wide P0 (ieks_ref.descent_inputs), from the filtered trajectory: the cost never rises, every
    instance accepts a step in iteration 1, the final J is strictly below the J of the EKF + RTS trajectory, and every accept
    decision has a margin of at least 1e-4 J(0)."""
    descent_check(name)


# ---- 6. mutated restatements fail ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", MUTATIONS)
def test_mutated_restatement_fails(which):
    """each mutation (c_k dropped from d-; nu and H at Xbar[k+1] [+] d- with the recursion still started from d-; Qd omitted; the
    recursion started from d = 0) is caught by the Gauss-Newton property (tests/test_host_ieks.py applies the same four to copies
    of the header)"""
    with pytest.raises(AssertionError):
        gauss_newton_check(lambda *a: I.pass_(*a, **{which: True}), "poly")


@pytest.mark.parametrize("which", ("drop_c", "no_q", "d0_zero"))
def test_mutated_restatement_is_no_fixed_point_or_no_descent(which):
    """...and by the fixed point (a c_k that is dropped or a start from 0 does not matter AT the fixed point: descent catches them)"""
    caught = 0
    for check in (lambda: fixed_point_check("poly", **{which: True}), lambda: descent_check("poly", **{which: True})):
        try:
            check()
        except AssertionError:
            caught += 1
    assert caught >= 1, which


# ---- distance from exact stationarity -------------------------------------------------------------------------------------------------
def test_converged_trajectory_is_nearly_stationary():
    """|grad J| by central differences at the trajectory the iteration ends on, relative to the same norm at the EKF + RTS
    trajectory (DESIGN.md §5 records the figure).  The first-order re-basing of the chart leaves the fixed point stationary to
    second order in the deviations only, so this is small, not zero."""
    d = I.descent_inputs("poly")
    cut = lambda a: a[..., :4]  # noqa: E731
    r = I.solve(d["orc"], cut(d["X0"]), cut(d["P"]), cut(d["Xfilt"]), cut(d["U"]), cut(d["Z"]), cut(d["masks"]), cut(d["Qd"]), cut(d["Rd"]),
                6, eps=d["eps"])
    a = (d["orc"], cut(d["X0"]), cut(d["P"]))
    b = (cut(d["U"]), cut(d["Z"]), cut(d["masks"]), cut(d["Qd"]), cut(d["Rd"]), E.MAG, d["eps"])
    g_map, g_ekf = I.grad_norm(*a, r["Xbar"], *b), I.grad_norm(*a, cut(d["Xekf"]), *b)
    print(f"[ieks stationarity] |grad J| MAP {g_map} / EKF + RTS {g_ekf} = {g_map / g_ekf}")
    assert (g_map < 0.1 * g_ekf).all()
