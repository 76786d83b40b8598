"""CPU tests of the envelope test infrastructure (tests/envelope_ref.py, oracle/ilqr_oracle.py::envelope_al_terms): the
float64 reference is the gradient, the Gauss-Newton curvature and the update rule of the loss it states; every case of the GPU
matrix meets the e32 and the margin condition and carries every branch; the metric flags each listed mistake wherever that
mistake reaches and nowhere else - while the whole-tensor lines the suite had before pass a reference without its beta row,
without its alpha row and without its height row."""
import numpy as np
import pytest

import ilqr_oracle as io
from tests import envelope_ref as er
from tests.helpers import f32_exact, make_oracle

FLAG = 1e-5      # the largest bar the e32 condition allows: a mutant must be above it wherever it reaches
W = er.W


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_terms_add_up_to_envelope_al_and_restatement_is_the_oracle():
    c = er.parent(3)
    orc = er._oracle()
    n = 40
    X, lam = c["X"][:, :, :n], c["lam"][:, :, :n]
    for lm in (lam, None):
        t = io.envelope_al_terms(orc, X, er.LO, er.HI, W, lm)
        cost, grad, curv, sv, rows = io.envelope_al(orc, X, er.LO, er.HI, W, lm)
        assert np.allclose(t["terms"].sum(axis=(0, 1)), cost, rtol=1e-13, atol=0)
        assert np.allclose(t["grad"].sum(axis=1), grad, rtol=1e-13, atol=1e-300) and np.allclose(t["curv"].sum(axis=1), curv, rtol=1e-13, atol=1e-300)
        assert np.array_equal(np.maximum(0, t["up"]) - np.maximum(0, t["dn"]), sv) and np.array_equal(t["rows"], rows)
        assert np.allclose(t["sabs"], np.abs(t["summands"]).sum(axis=0)) and (t["sabs"] >= np.abs(t["terms"]) * (1 - 1e-15)).all()
    # the dtype-generic restatement, run in float64, is the oracle's rows and Jacobian (this licenses its e32) ...
    r64, J64 = er.rows_np(np.float64, c["X"])
    assert np.abs(r64 - c["rows"]).max() <= 1e-12 * np.abs(c["rows"]).max()
    for r in range(4):
        assert np.abs(J64[:, r] - c["Jx"][:, r]).max() <= 1e-12 * np.abs(c["Jx"][:, r]).max() + 1e-11 * (r == 0)
    assert er.zeros_kept(J64, c["Jx"])
    # ... the speed row's attitude columns are what a cancellation of terms of ~2 V^2 leaves: 2 eps sum_i dr_i / dq
    assert np.abs(c["Jx"][:, 0, 6:10]).max() < 1e-3 and np.abs(c["Jx"][:, 0, 3:6]).max() > 100
    # ... and the penalty arithmetic on them is envelope_al_terms'
    for lam_on in (True, False):
        ref, a64 = er.reference(c, None, "both", lam_on), er.restated(c, None, "both", lam_on, dtype=np.float64)
        assert er.term_err(a64["cost"], ref["cost"], ref["S_abs"]).max() < 1e-12
        assert max(v.max() for v in er.grad_err(a64["grad"] - ref["grad"].sum(axis=1), ref["grad"]).values()) < 1e-10
        assert max(v.max() for v in er.curv_err(a64["curv"] - ref["curv"].sum(axis=1), ref["curv"]).values()) < 1e-10
        lamc = np.zeros_like(c["lam"]) if not lam_on else c["lam"]
        assert er.lam_err(er.al_np(np.float64, c["rows"], c["Jx"], er.LO, er.HI, W, lamc)["new"], io.envelope_al_update(c["rows"], er.LO, er.HI, W, lamc)).max() < 1e-14
        assert np.allclose(a64["excess"], io.envelope_excess(c["rows"], er.LO, er.HI), rtol=1e-14)


def test_row_gradient_is_the_central_difference_of_the_row_cost():
    """per row: 2 w (up - dn) grad g_r against central differences of that row's own terms in v and q, at every node, away from
    the kinks (the margin condition keeps every row value 1e-4 of its scale off a shifted bound)"""
    c = er.parent(2)
    orc = er._oracle()
    n = 24
    X, lam = np.array(c["X"][:, :, :n]), c["lam"][:, :, :n]
    t = io.envelope_al_terms(orc, X, er.LO, er.HI, W, lam)
    row_cost = lambda Xq: io.envelope_al_terms(orc, Xq, er.LO, er.HI, W, lam)["summands"].sum(axis=(0, 1))  # noqa: E731  (4, n)
    worst = np.zeros(4)
    for k in range(X.shape[0]):
        for j in range(3, 10):
            h = 1e-4 if j < 6 else 1e-6
            Xp, Xm = X.copy(), X.copy()
            Xp[k, j] += h; Xm[k, j] -= h
            fd = (row_cost(Xp) - row_cost(Xm)) / (2 * h)
            for r in range(4):
                scale = np.abs(t["grad"][k, r, 3:10]).max()
                if scale > 0:
                    worst[r] = max(worst[r], np.abs(t["grad"][k, r, j] - fd[r]).max() / scale)
    print("row gradient vs central differences, worst / the row's largest entry at the node:", worst)
    assert (worst < 2e-6).all(), worst
    assert np.array_equal(t["grad"][:, 3, 2], 2 * W * (np.maximum(0, t["up"][:, 3]) - np.maximum(0, t["dn"][:, 3])))
    assert not t["grad"][:, :3, :3].any() and not t["grad"][:, :, 10:].any() and not t["grad"][:, 3, 3:].any()


def test_curvature_penalty_special_case_and_update_rule():
    c = er.parent(3)
    t = er.reference(c)
    J = c["Jx"]
    active = (t["up"] > 0).astype(float) + (t["dn"] > 0)
    assert active.max() == 2
    assert np.allclose(t["curv"], 2 * W * np.einsum("krb,kkrib,krjb->krijb".replace("kkrib", "krib"), active, J, J), rtol=1e-14, atol=0)
    # zero multipliers: the plain penalty w sum viol^2 with its one-sided violation
    z = er.reference(c, lam_on=False)
    rows = c["rows"]
    lo, hi = er.LO[None, :, None], er.HI[None, :, None]
    viol = np.where(rows > hi, rows - hi, np.where(rows < lo, rows - lo, 0.0))
    assert np.allclose(z["cost"], W * (viol ** 2).sum(axis=(0, 1)), rtol=1e-14)
    assert np.allclose(z["grad"].sum(axis=1), 2 * W * np.einsum("krb,krjb->kjb", viol, J), rtol=1e-13, atol=1e-300)
    zz = io.envelope_al_terms(None, c["X"], er.LO, er.HI, W, np.zeros_like(c["lam"]), rows_jx=(rows, J))
    assert all(np.array_equal(zz[k], z[k]) for k in ("summands", "grad", "curv"))
    # the update is max(0, 2 w x the shifted one-sided violation)
    new = io.envelope_al_update(rows, er.LO, er.HI, W, c["lam"])
    assert np.allclose(new, np.maximum(0.0, 2 * W * np.concatenate([t["up"], t["dn"]], axis=1)), rtol=1e-13, atol=1e-12)
    assert (new >= 0).all() and (new == 0).any()


# ---- the GPU matrix ----------------------------------------------------------------------------------------------------------------------
def test_every_gpu_case_meets_the_e32_condition():
    worst = {}
    for name, e32 in er.gpu_case_e32():
        assert e32 <= er.E32_MAX, (name, e32)
        fam = name.split("[")[0].split(".")[0] + ("." + name.rsplit(".", 2)[-2] + "." + name.rsplit(".", 1)[-1] if name.startswith("model") else "")
        worst[fam] = max(worst.get(fam, 0.0), e32)
    print("e32 per family:", {k: f"{v:.2e}" for k, v in worst.items()})


def _cases():
    return [(f"parent[H{H}]", er.parent(H)) for H in (1, 2, 3, 7)] + [(f"candidates[{Bl}x3-H{H}]", er.candidates(Bl, H)) for Bl in er.COST_BL for H in er.COST_H]


def test_every_gpu_case_meets_the_margin_condition_and_the_active_sets_agree():
    for name, c in _cases():
        n = c["X"].shape[2]
        scale = np.abs(c["rows"]).max(axis=(0, 2))[None, :3, None]
        for lam_on in (True, False):
            t, f = er.reference(c, lam_on=lam_on), er.restated(c, lam_on=lam_on)
            for key in ("up", "dn"):
                assert (np.abs(t[key][:, :3]) >= er.MARGIN * scale).all(), (name, key, "a row value within the margin of a shifted bound")
                assert np.array_equal(t[key] > 0, f[key] > 0), (name, key, "the fp32 restatement's active set differs")
        assert n >= 1 and c["X"].dtype == np.float64 and np.array_equal(c["X"], f32_exact(c["X"])) and np.array_equal(c["lam"], f32_exact(c["lam"]))
        # the height row is exact: z, the bounds and lam / 2w are fp32 numbers whose sums are fp32 numbers
        lamc = np.tile(c["lam"], (1, 1, n // c["lam"].shape[2]))
        for v in (c["rows"][:, 3] - er.HI[3] + lamc[:, 3] / (2 * W), er.LO[3] - c["rows"][:, 3] + lamc[:, 7] / (2 * W)):
            assert np.array_equal(v, f32_exact(v)) and np.array_equal(2 * W * v, f32_exact(2 * W * v))


def test_every_gpu_case_carries_every_branch():
    for name, c in _cases():
        n = c["X"].shape[2]
        if n < 65:       # a narrow candidate batch is joined by its 257-wide parent (tests/cost_terms_ref.py's rule)
            continue
        for first in (None, 65):
            inv = er.inventory(c, first)
            assert all(v >= 2 for v in inv.values()), (name, first, inv)
    inv = er.inventory(er.candidates(5, 3))
    assert inv["upper active"] >= 2 and inv["lower active"] >= 2, inv


# ---- mutations ------------------------------------------------------------------------------------------------------------------------------
def evaluate(c, lo, hi, lam, mut=None, drop=None, repeat=False):
    """cost (B,), gradient (Hn, 13, B), curvature (Hn, 13, 13, B; terminal node zero), new multipliers (Hn, 8, B) and excess (B,)
    in float64 from the case's rows and Jacobian, with one mistake switched on"""
    rows, J = c["rows"], c["Jx"]
    Hn, _, B = rows.shape
    lam = np.zeros((Hn, 8, B)) if lam is None else (np.repeat(lam, B // lam.shape[2], axis=2) if repeat else np.tile(lam, (1, 1, B // lam.shape[2])))
    lh, ll = lam[:, :4], (lam[:, :4] if mut == "lower multipliers from the upper rows" else lam[:, 4:])
    sh, sl = lh / (2 * W), ll / (2 * W)
    lo, hi = np.asarray(lo)[None, :, None], np.asarray(hi)[None, :, None]
    up, dn = rows - hi + sh, lo - rows + sl
    vh, vl = np.maximum(0, up), np.maximum(0, dn)
    on = np.ones(4); on[drop] = 0 if drop is not None else 1
    on3 = on[None, :, None]
    const = 0.0 if mut == "constant term dropped" else sh ** 2 + sl ** 2
    cost = W * (on3 * (vh ** 2 + vl ** 2 - const)).sum(axis=(0, 1))
    v = vh + vl if mut == "lower side's sign flipped" else vh - vl
    grad = 2 * W * np.einsum("krb,krjb->kjb", on3 * v, J)
    act = (vh > 0).astype(float) + (vl > 0)
    if mut == "two active sides counted as one":
        act = np.minimum(act, 1.0)
    curv = 2 * W * np.einsum("krb,krib,krjb->kijb", on3 * act, J, J)
    if mut != "curvature at the terminal node":
        curv[-1] = 0
    new = np.concatenate([np.maximum(0, lh + 2 * W * (rows - hi)), np.maximum(0, ll + 2 * W * (lo - rows))], axis=1)
    if drop is not None:
        new[:, [drop, 4 + drop]] = lam[:, [drop, 4 + drop]]
    span = (hi - lo)[0, :, 0]
    sc = np.where((span > 0) & (span < 1e30) & (mut != "excess not scaled by the span"), 1.0 / span, 1.0)
    exc = np.where(on3 > 0, np.maximum(rows - hi, lo - rows) * sc[None, :, None], -np.inf)
    return dict(cost=cost, grad=grad, curv=curv, new=new, excess=np.maximum(exc.max(axis=(0, 1)), 0.0))


def metric(c, m, row, side, lam_on=True):
    """{quantity: error array} of an evaluation m against the reference of the run (row, side)"""
    ref = er.reference(c, row, side, lam_on)
    n = c["X"].shape[2]
    rc = ref["curv"].copy(); rc[-1] = 0
    out = {"cost": er.term_err(m["cost"], ref["cost"], ref["S_abs"]),
           **{f"grad.{g}": v for g, v in er.grad_err(m["grad"] - ref["grad"].sum(axis=1), ref["grad"]).items()},
           **{f"curv.{g}": v for g, v in er.curv_err(m["curv"] - rc.sum(axis=1), rc).items()}}
    lamc = (np.tile(ref["lam"], (1, 1, n // ref["lam"].shape[2])) if lam_on else np.zeros((c["X"].shape[0], 8, n)))
    out["new"] = er.lam_err(m["new"], io.envelope_al_update(c["rows"], ref["lo"], ref["hi"], W, lamc))
    out["excess"] = er.excess_err(m["excess"], io.envelope_excess(c["rows"], ref["lo"], ref["hi"]))
    return out


RUNS = [(f"{er.ROWS[r]}.{s}", r, s) for r in range(4) for s in ("up", "lo", "both")] + [("all", None, "both")]
MUTANTS = [(f"{er.ROWS[r]} row dropped", dict(drop=r), {"cost", "grad", "curv", "new", "excess"}) for r in range(4)] + [
    ("lower side's sign flipped", {}, {"grad"}),
    ("lower multipliers from the upper rows", {}, {"cost", "grad", "curv", "new"}),
    ("constant term dropped", {}, {"cost"}),
    ("two active sides counted as one", {}, {"curv"}),
    ("curvature at the terminal node", {}, {"curv"}),
    ("excess not scaled by the span", {}, {"excess"})]


def test_the_evaluator_without_a_mistake_is_the_reference():
    c = er.parent(3)
    for label, row, side in RUNS:
        lo, hi, m = er.run_bounds(row, side)
        e = metric(c, evaluate(c, lo, hi, c["lam"] * m[None, :, None]), row, side)
        assert all(v.max() < 1e-12 for v in e.values()), (label, {k: v.max() for k, v in e.items()})


@pytest.mark.parametrize("name,kw,reaches", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_metric_flags_the_mistake_where_it_reaches_and_nowhere_else(name, kw, reaches):
    """Each mistake, applied to the float64 reference: in the runs with one row bounded every entry of the metric is exactly
    zero or above 1e-5 (an entry the mistake reaches is flagged, the others do not move); it reaches the quantities listed and
    no other.  Two things are not asked: the speed row's q group and vq / qq blocks are held to its v scale (the exception),
    so its own d/dq (3e-4 against 140) is below the flag; and with all rows bounded an entry where a larger row is violated too
    is held to that row's scale - there the run must flag the mistake somewhere, not everywhere."""
    c = er.parent(3)
    hit = set()
    for label, row, side in RUNS:
        if "drop" in kw and row not in (None, kw["drop"]):
            continue
        lo, hi, m = er.run_bounds(row, side)
        e = metric(c, evaluate(c, lo, hi, c["lam"] * m[None, :, None], mut=name, **kw), row, side)
        for key, v in e.items():
            q = key.split(".")[0]
            moved = v > 1e-12
            if not moved.any():
                continue
            assert q in reaches, (name, label, key, "moved, and should not have")
            if row is None or (row == 0 and key in ("grad.q", "curv.vq", "curv.qq")):
                hit |= {q} if (v > FLAG).any() else set()
                continue
            # (the height row is exact, its bar on the card is 0: whatever moves is flagged - one fp32 ulp above the bound included)
            assert row == 3 or (v[moved] > FLAG).all(), (name, label, key, "an entry it reaches is below the flag:", float(v[moved].min()))
            hit.add(q)
    assert hit >= reaches - {"excess"} or hit == reaches, (name, "reached only", hit)


def test_metric_flags_candidates_mapped_by_division():
    """column o of a candidate batch reads instance o % Bl; o / reps is flagged on every column whose multipliers differ"""
    c = er.candidates(5, 3)
    good = evaluate(c, er.LO, er.HI, c["lam"])
    bad = evaluate(c, er.LO, er.HI, c["lam"], repeat=True)
    e = metric(c, bad, None, "both")["cost"]
    same = np.arange(15) % 5 == np.arange(15) // 3
    assert metric(c, good, None, "both")["cost"].max() < 1e-12
    assert (e[same] < 1e-12).all() and (e[~same] > FLAG).all() and (~same).sum() >= 10, e


# ---- what the whole-tensor lines of tests/test_gpu_ilqr.py let through --------------------------------------------------------------------------
OLD_BOUNDS = ((45.0 ** 2, 60.0 ** 2), (-0.01, 0.01), (-0.02, 0.03), (-1e30, -199.5))


def old_inputs(B=40, H=12):
    """the states of test_envelope_penalty_kernels_match_numpy / test_envelope_al_kernels_match_numpy, restated on the CPU: the
    same initial states and controls (tests/test_gpu_ilqr.py::setup, synthetic_problem(B, H, seed=3) x 0.3) rolled out by the
    float64 oracle instead of the GPU, and the AL test's multipliers"""
    from aircraft_amd.synthetic import quat_from_euler, quat_rotate
    from tests.helpers import synthetic_problem

    rng = np.random.default_rng(3)
    X0 = np.zeros((13, B)); X0[2] = -200.0
    V = rng.uniform(50, 65, B); al = np.deg2rad(rng.uniform(-1, 1, B)); be = np.deg2rad(rng.uniform(-1, 1, B))
    vb = np.stack([V * np.cos(al) * np.cos(be), V * np.sin(be), V * np.sin(al) * np.cos(be)])
    q = quat_from_euler(np.deg2rad(rng.uniform(-5, 5, B)), np.deg2rad(rng.uniform(-2, 2, B)), np.deg2rad(rng.uniform(-5, 5, B)))
    X0[3:6] = quat_rotate(q, vb); X0[6:10] = q; X0[10:13] = rng.normal(0, 0.02, (3, B))
    _, Us = synthetic_problem(B, H, seed=3)
    X = f32_exact(er._oracle().rollout(f32_exact(X0), f32_exact(0.3 * Us), 0.01))
    rng = np.random.default_rng(8)
    lam0 = f32_exact(rng.uniform(0, 1, (H + 1, 8, B)) * (rng.uniform(0, 1, (H + 1, 8, B)) < 0.5) * np.array([50.0, 0.2, 0.05, 2.0] * 2)[None, :, None])
    lam0[:, 7] = 0.0
    return X, lam0


def test_the_old_whole_tensor_lines_miss_a_dropped_row_and_the_row_metric_does_not():
    """On the inputs of the two older GPU tests the whole-tensor lines on cost and gradient pass a reference without its beta
    row, without its alpha row and without its height row, and the curvature line passes a beta-row curvature 20 % off and an
    alpha-row curvature 40 % off; the row metric flags each.  (The multiplier line is printed, not claimed: on these states a row
    left out of the update moves lam by 0.15 .. 2.0 against the 0.069 the line allows.)"""
    X, lam0 = old_inputs()
    assert X.shape == (13, 13, 40)
    orc = er._oracle()
    lo = np.array([b[0] for b in OLD_BOUNDS]); hi = np.array([b[1] for b in OLD_BOUNDS])
    w = 3.0
    for lam in (None, lam0):
        t = io.envelope_al_terms(orc, X, lo, hi, w, lam)
        cw, gw, pw = t["terms"].sum(axis=(0, 1)), t["grad"].sum(axis=1), t["curv"].sum(axis=1)
        want = io.envelope_al_update(t["rows"], lo, hi, w, np.zeros_like(lam0) if lam is None else lam)
        if lam is None:      # the penalty test's states never cross the height bound: there that row is not exercised at all
            assert t["sabs"][:, 3].sum() == 0 and not t["grad"][:, 3].any()
        for r, off in ((1, 0.2), (2, 0.4), (3, 1.0))[:2 if lam is None else 3]:
            assert t["sabs"][:, r].sum() > 0 and np.abs(t["grad"][:, r]).max() > 0, (er.ROWS[r], "row not violated on the old inputs")
            keep = np.arange(4) != r
            cm, gm = t["terms"][:, keep].sum(axis=(0, 1)), t["grad"][:, keep].sum(axis=1)
            # the lines of tests/test_gpu_ilqr.py, with their own tolerances: all of them pass
            assert np.abs(cm - cw).max() <= 2e-5 * max(np.abs(cw).max(), 1.0)
            assert np.abs(gm - gw).max() <= 5e-5 * max(np.abs(gw).max(), 1.0)
            assert np.abs(off * t["curv"][:12, r]).max() <= 1e-4 * max(np.abs(pw).max(), 1.0)
            if lam is not None:
                print(er.ROWS[r], "left out of the update moves lam by", np.abs(want - lam)[:, [r, 4 + r]].max(), "the old line allows", 2e-5 * np.abs(want).max())
            # the row metric: the dropped row's own run has lost its whole cost, gradient and (where it has one) curvature
            assert er.term_err(0 * cw, t["terms"][:, r].sum(axis=0), t["sabs"][:, r].sum(axis=0)).max() > 0.1
            only = (np.arange(4) == r)
            e = er.grad_err(-t["grad"][:, r], t["grad"] * only[None, :, None, None])
            assert max(v.max() for v in e.values()) > 0.1
            if np.abs(t["curv"][:12, r]).max() > 0:
                e = er.curv_err(-off * t["curv"][:12, r], t["curv"][:12] * only[None, :, None, None, None])
                assert max(v.max() for v in e.values()) > 0.1
