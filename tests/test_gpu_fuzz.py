"""Seeded differential sweep: random (model, sub-steps, normalise, stall scaling, dt, batch size) configurations, every
entry point of the step path against the float64 oracle.  Catches interactions the targeted parity tests do not pair
up (e.g. stall scaling x sub-stepped sensitivities x per-unit dt on a ragged batch)."""
import numpy as np
import pytest

from tests.helpers import (HESS_BLOCK_BAR, HESS_FLOOR, block_rel_err, check_hess_blocks, f32_exact, hess_block_conditioning,
                           hess_block_rel, make_aircraft, make_oracle, oracle_step_hessian, rel_fro, unit_max_rel, synthetic_units)

pytestmark = pytest.mark.gpu

# (model, hidden widths, use_mfma): the last two are the "MFMA off" flavour on the tiled vector-ALU engines (8 units per wave for
# the sensitivity kernels, 64 / 8 / 4 for the forward kernels and rollouts)
MODELS = [("default", None, True), ("linear", None, True), ("poly", None, True), ("nn", None, True), ("nn", (48, 40), True),
          ("nn", (64, 64, 64), True), ("nn", (64, 64, 64), False), ("nn", (24, 32), False)]


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


@pytest.mark.parametrize("seed", range(16))
def test_random_configuration(gpu, seed):
    rng = np.random.default_rng(1000 + seed)
    model, hidden, use_mfma = MODELS[seed % len(MODELS)]
    substeps = int(rng.choice([1, 1, 2, 3]))
    normalise = bool(rng.integers(2))
    stall = bool(rng.integers(2))
    n = int(rng.choice([1, 15, 17, 63, 65, 250, 1025]))
    dt = float(rng.choice([0.005, 0.01, 0.02]))
    ac = make_aircraft(model, hidden=hidden, substeps=substeps, normalise=normalise, stall_scaling=stall, use_mfma=use_mfma)
    orc = make_oracle(ac)
    X, U = synthetic_units(n, seed=seed, flaps=bool(rng.integers(2)))
    tag = f"{model}{hidden}{'' if use_mfma else ' mfma-off'} substeps={substeps} normalise={normalise} stall={stall} n={n} dt={dt}"
    Xd, Ud = dev(X, gpu), dev(U, gpu)
    # derivative and step
    xd = ac.state_derivative(Xd, Ud).cpu().numpy()
    want = orc.state_derivative(X, U)
    assert np.abs(xd - want).max() / max(np.abs(want).max(), 1.0) < 5e-6, tag
    per_unit = bool(rng.integers(2))
    dts = f32_exact(rng.uniform(0.5 * dt, 1.5 * dt, n)) if per_unit else dt
    xn = ac.state_update(Xd, Ud, dev(dts, gpu) if per_unit else dt).cpu().numpy()
    assert block_rel_err(xn, orc.state_update(X, U, dts)) < 5e-6, tag
    # sensitivities
    Xn, A, Bm, c = ac.step_sens(Xd, Ud, dev(dts, gpu) if per_unit else dt)
    Xr, Ar, Br, cr = orc.step_sens(X, U, dts)
    assert block_rel_err(Xn.cpu().numpy(), Xr) < 5e-6, tag
    assert rel_fro(A.cpu().numpy(), Ar) < 2e-5 and rel_fro(Bm.cpu().numpy(), Br) < 1e-4 and rel_fro(c.cpu().numpy(), cr) < 1e-4, tag
    for g_, w_ in ((A, Ar), (Bm, Br), (c, cr)):  # and every unit on its own (max norm)
        assert unit_max_rel(g_.cpu().numpy(), w_).max() < 1e-4, tag
    # second-order blocks (one RK4 sub-step only)
    if substeps == 1 and n <= 250:
        lam = f32_exact(rng.normal(size=(13, n)))
        Hm = ac.step_hess(Xd, Ud, dev(dts, gpu) if per_unit else dt, dev(lam, gpu)).cpu().numpy().astype(np.float64)
        Hr = oracle_step_hessian(orc, X, U, dts, lam)
        num = np.sqrt(((Hm - Hr) ** 2).sum(axis=(0, 1))); den = np.sqrt((Hr ** 2).sum(axis=(0, 1)))
        rel = num / np.maximum(den, 1e-30)
        # every block pair of every unit on its own, within the bar or 8 x the unit's per-block conditioning
        cond = hess_block_conditioning(orc, X, U, dts, lam, want=Hr, floor=HESS_FLOOR)
        eb = hess_block_rel(Hm, Hr, HESS_FLOOR)
        Hr7 = None
        if rel.max() >= 1e-3 or any((v > np.maximum(HESS_BLOCK_BAR, 8.0 * cond[k])).any() for k, v in eb.items()):
            # The CHECKER differentiates exact Jacobians by central differences with h = 1e-5: a unit whose alpha or beta passes
            # through 0 inside that step (the |.| kinks of the stall scaling) gets a wrong reference, not a wrong kernel —
            # tools/fuzz_diag.py, round 3: seeds 157, 214, 302, 463 disagree by 3e-2 .. 1 at h = 1e-5 and by < 1e-6 at h = 1e-7.
            # Such units are re-checked against the finer step (per unit, and per block below).
            Hr7 = oracle_step_hessian(orc, X, U, dts, lam, h=1e-7)
            num7 = np.sqrt(((Hm - Hr7) ** 2).sum(axis=(0, 1))); den7 = np.sqrt((Hr7 ** 2).sum(axis=(0, 1)))
            rel = np.minimum(rel, num7 / np.maximum(den7, 1e-30))
            assert (rel >= 1e-3).sum() == 0 and (num / np.maximum(den, 1e-30) >= 1e-3).sum() <= max(2, n // 50), tag
        assert rel.max() < 1e-3, tag
        check_hess_blocks(f"fuzz_hess_blocks[seed={seed}]", Hm, Hr, HESS_BLOCK_BAR, route=tag, cond=cond, alt=Hr7, populated=0.0)
    # a short rollout from the same states
    H = 6
    Uh = f32_exact(np.tile(U[None], (H, 1, 1)))
    traj = ac.rollout(Xd, dev(Uh, gpu), dt).cpu().numpy()
    assert block_rel_err(traj, orc.rollout(X, Uh, dt)) < 2e-5, tag
