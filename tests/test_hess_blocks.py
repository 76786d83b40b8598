"""CPU tests of the per-block metric the second-order tests hold the GPU Hessian to (tests/helpers.py::hess_block_rel):
the checker's own noise per block is far below the bar, and the metric flags a wrong block wherever the block is above
its floor.  Needs only the float64 oracle."""
import numpy as np
import pytest

from tests.helpers import (HESS_BLOCK_BAR, HESS_FLOOR, HESS_GROUPS, QUAD_HESS_GROUPS, f32_exact,
                           hess_block_conditioning, hess_block_norms, hess_block_pairs, hess_block_rel, make_aircraft,
                           make_oracle, oracle_step_hessian, parity_report, synthetic_units)

MODELS = {
    "default": dict(model="default", stall_scaling=True),
    "linear": dict(model="linear"),
    "poly": dict(model="poly"),
    "nn": dict(model="nn"),
    "4x128": dict(model="nn", hidden=(128, 128, 128, 128)),
    "3x64": dict(model="nn", hidden=(64, 64, 64)),
}


def _case(name, n=96):
    """(oracle, X, U, dt, lam, groups, bar) with the GPU tests' own inputs"""
    if name == "quad":
        from aircraft_amd import Quadrotor
        from oracle import Oracle
        from tests.test_gpu_quadrotor import pad7, quad_units

        q = Quadrotor()
        q.normalise = True
        q.com = np.array([0.02, -0.01, 0.03])
        orc = Oracle(q.airframe_dict(), "quad", None, substeps=1, normalise=True, epsilon=q.epsilon, gravity=q.gravity)
        X, U = quad_units(64, seed=9)
        lam = f32_exact(np.random.default_rng(3).normal(size=(13, 64)))
        return orc, X, pad7(U), 0.02, lam, QUAD_HESS_GROUPS, HESS_BLOCK_BAR
    kw = dict(MODELS[name])
    ac = make_aircraft(kw.pop("model"), normalise=True, **kw)
    X, U = synthetic_units(n, seed=31, flaps=True)
    lam = f32_exact(np.random.default_rng(131).normal(size=(13, n)))
    return make_oracle(ac), f32_exact(X), f32_exact(U), 0.01, lam, HESS_GROUPS, HESS_BLOCK_BAR


CASES = list(MODELS) + ["quad"]
KINK = 1e-2  # rad


@pytest.mark.parametrize("name", CASES)
def test_checker_noise_per_block_is_below_bar_over_30(name):
    """oracle_step_hessian at h = 1e-5 against h = 1e-6, every block pair of every smooth unit: within bar / 30.  Smooth:
    the reference resolves its blocks (per-block conditioning under a one-ulp input perturbation below bar / 30), and the
    angle of attack and the sideslip are at least KINK rad from the |.| kinks of the stall scaling at 0 (next to one the
    third derivatives are large and the difference step's truncation grows: alpha = 7e-4 rad gives 2e-5 at h = 1e-5; the
    GPU tests fall back to h = 1e-7 there, tests/test_gpu_fuzz.py)."""
    orc, X, U, dt, lam, groups, bar = _case(name)
    H5 = oracle_step_hessian(orc, X, U, dt, lam)
    H6 = oracle_step_hessian(orc, X, U, dt, lam, h=1e-6)
    noise = hess_block_rel(H6, H5, HESS_FLOOR, groups)
    cond = hess_block_conditioning(orc, X, U, dt, lam, want=H5, floor=HESS_FLOOR, groups=groups)
    smooth = np.all([c <= bar / 30 for c in cond.values()], axis=0)
    if name != "quad":
        angles = orc.aero(X, U)[4:6]
        smooth &= (np.abs(angles) > KINK).all(axis=0)
    assert smooth.mean() >= 0.75, (name, float(smooth.mean()))
    worst = {k: float(v[smooth].max()) for k, v in noise.items()}
    parity_report(f"hess_checker_noise[{name}]", bar=bar, floor=HESS_FLOOR, smooth_units=int(smooth.sum()), units=int(smooth.size),
                  worst=max(worst.values()), worst_block=max(worst, key=worst.get))
    assert max(worst.values()) <= bar / 30, (name, {k: v for k, v in worst.items() if v > bar / 30})
    # blocks that are zero in the model come out zero at both steps (the quadrotor's velocity rows)
    norms, whole = hess_block_norms(H5, groups)
    for k, v in norms.items():
        if not v.any():
            assert not hess_block_norms(H6, groups)[0][k].any(), (name, k)


def _mutate(H, groups, a, b, kind, bar):
    M = H.copy()
    halves = [(groups[a], groups[b])] + ([(groups[b], groups[a])] if a != b else [])
    for sa, sb in halves:  # both halves: the mutant stays symmetric
        if kind == "zero":
            M[sa, sb] = 0.0
        elif kind == "negate":
            M[sa, sb] = -H[sa, sb]
        else:
            M[sa, sb] = H[sa, sb] * (1.0 + 10.0 * bar)
    return M


@pytest.mark.parametrize("name", CASES)
def test_metric_flags_every_wrong_block(name):
    """Each of the 21 block pairs (15 for the quadrotor) in turn zeroed, negated or scaled by 1 + 10 x bar: flagged (error
    above the bar) on every unit where that block is above the floor, and no other block moves.  A whole-unit norm misses
    most of these (the dt row and column dominate it): this pins the power of the metric the GPU tests use."""
    orc, X, U, dt, lam, groups, bar = _case(name)
    H = oracle_step_hessian(orc, X, U, dt, lam)
    norms, whole = hess_block_norms(H, groups)
    base = hess_block_rel(H, H, HESS_FLOOR, groups)
    assert all(not v.any() for v in base.values())
    pairs = hess_block_pairs(groups)
    assert len(pairs) == len(groups) * (len(groups) + 1) // 2
    checked = 0
    for a, b in pairs:
        key = f"{a}-{b}"
        live = norms[key] > HESS_FLOOR * whole
        for kind in ("zero", "negate", "scale"):
            M = _mutate(H, groups, a, b, kind, bar)
            assert np.array_equal(M, M.transpose(1, 0, 2)) == np.array_equal(H, H.transpose(1, 0, 2))
            err = hess_block_rel(M, H, HESS_FLOOR, groups)
            assert (err[key][live] > bar).all(), (name, key, kind, float(err[key][live].min()))
            assert all(not err[k].any() for k in err if k != key), (name, key, kind)
        checked += int(live.any())
    # every block is populated somewhere, except the ones the model makes zero (the quadrotor's velocity blocks)
    zero = {k for k, v in norms.items() if not v.any()}
    assert checked == len(pairs) - len(zero), (name, checked, zero)
    assert zero == ({"v-v", "v-q", "v-w", "v-thrust"} if name == "quad" else set())


def test_zero_block_is_held_to_the_floor():
    """A block the reference makes exactly zero must come out below bar x floor x ||H_ref||: the quadrotor's velocity rows."""
    orc, X, U, dt, lam, groups, bar = _case("quad")
    H = oracle_step_hessian(orc, X, U, dt, lam)
    whole = np.sqrt((H ** 2).sum(axis=(0, 1)))
    for scale, flagged in ((0.5, False), (2.0, True)):
        M = H.copy()
        M[3, 10] = M[10, 3] = scale * bar * HESS_FLOOR * whole / np.sqrt(2.0)
        err = hess_block_rel(M, H, HESS_FLOOR, groups)["v-w"]
        assert ((err > bar) == flagged).all(), (scale, float(err.min()), float(err.max()))


def test_conditioning_helper_matches_a_direct_perturbation():
    """hess_block_conditioning is the per-block deviation of the reference under a relative one-ulp perturbation of x and u
    (its own draws, restated), in the same metric; and it is small where the dynamics do not amplify."""
    orc, X, U, dt, lam, groups, bar = _case("poly", n=24)
    H = oracle_step_hessian(orc, X, U, dt, lam)
    cond = hess_block_conditioning(orc, X, U, dt, lam, want=H, floor=HESS_FLOOR, draws=1, seed=7)
    rng = np.random.default_rng(7)
    Xp = X * (1.0 + 1e-7 * rng.choice([-1.0, 1.0], X.shape))
    Up = U * (1.0 + 1e-7 * rng.choice([-1.0, 1.0], U.shape))
    direct = hess_block_rel(oracle_step_hessian(orc, Xp, Up, dt, lam), H, HESS_FLOOR)
    assert set(cond) == set(direct) and len(cond) == 21
    for k in cond:
        assert np.array_equal(cond[k], direct[k]), k
    assert np.median(np.concatenate(list(cond.values()))) < 1e-5
