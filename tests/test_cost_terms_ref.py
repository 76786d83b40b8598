"""CPU tests of the cost-term test infrastructure (tests/cost_terms_ref.py, oracle/track_oracle.py::mhtt_model and the
per-term losses): the float64 model agrees with finite differences of the loss it models, every case of the GPU matrix
meets the e32 condition and populates every branch it is meant to, and the metric flags each listed mistake where that
mistake reaches and nowhere else - while the whole-tensor assertions the suite had before miss two of them."""
import numpy as np
import pytest

import ilqr_oracle as io
import track_oracle as to
from tests import cost_terms_ref as cr
from tests.helpers import f32_exact

FLAG = 1e-5      # the largest bar the e32 condition allows: a mutant must be above it wherever it reaches


# ---- the restatements ---------------------------------------------------------------------------------------------------------------
def test_terms_add_up_to_the_losses():
    c = cr.track_case("arc", 1, 12)
    tro = to.TrackOracle(c["points"])
    n = 24
    terms = {k: v[:n] for k, v in c["terms"].items()}
    J = to.mhtt_loss(tro, c["L"], c["X"][:, :, :n], c["U"][:, :, :n], c["Sin"][:, :n])
    assert np.allclose(sum(terms.values()), J, rtol=1e-13, atol=0)
    g = cr.goal_cost_case(5, 3, 6)
    i = g["inp"]
    J = io.goal_cost(cr._oracle(), g["g"], i["goal"], i["X"], i["U"], i["lam"])
    assert np.allclose(sum(v[:15] for v in g["ref"].values()), J, rtol=1e-13, atol=0)


def test_float64_restatements_are_the_oracle():
    """cost_terms_ref's dtype-generic restatements, run in float64, are the oracle's numbers (this licenses their e32)"""
    for track in cr.TRACKS:
        for mode in (0, 1):
            c = cr.track_case(track, mode, 12)
            T = cr.TrackNP(c["points"], np.float64)
            S, sd, e2, nq, nx, ng = cr.progress_np(np.float64, T, c["X"], c["s0"], cr.DT, mode)
            assert np.abs(S - c["S"]).max() < 1e-13 and np.abs(sd - c["s_dot"]).max() < 1e-13
            assert np.abs(e2 - c["err2"]).max() < 1e-9
            for a, r in zip((nq, nx, ng), c["model"]):
                assert cr.zeros_kept(a, r) and max(v.max() for v in cr.group_err(a, r).values()) < 1e-12
            t64 = cr.mhtt_terms_np(np.float64, T, c["X"], c["U"], c["Sin"])
            for k in to.TERMS:
                assert cr.term_err(t64[k], c["terms"][k], c["sabs"][k]).max() < 1e-12, k
    g = cr.goal_cost_case(86, 7, 6)
    i = g["inp"]
    t64 = cr.goal_terms_np(np.float64, g["g"], i["goal"], i["X"], i["U"], i["lam"])
    for k in io.GOAL_TERMS:
        assert cr.term_err(t64[k], g["ref"][k][:258], g["sabs"][k][:258]).max() < 1e-12, k
    m = cr.goal_model_case(37, 7, 6)
    i = m["inp"]
    r64 = cr.goal_model_np(np.float64, m["g"], i["goal"], i["X"], i["U"], i["lam"])
    for a, r in zip(r64, m["ref"]):
        assert np.abs(a - r).max() <= 1e-9 * np.abs(r).max()
    # the attitude rows of the speed gradient: 2 epsilon sum_i d r_i / d q_j, left over when terms of ~6000 cancel
    assert np.abs(r64[2][:7, 6:10] - m["ref"][2][:7, 6:10]).max() < 1e-12 and np.abs(m["ref"][2][:7, 6:10]).max() < 1e-6


# ---- the model is the gradient of the loss --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track,mode,H", [("straight", 1, 2), ("arc", 1, 12), ("arc", 0, 2)])
def test_model_gradient_is_the_central_difference_of_the_loss_at_frozen_progress(track, mode, H):
    """w_progress = 0: nq (x - nx) + ng against central differences of mhtt_loss with S held, for p_k, v_k of every node,
    terminal node included, on the first 24 columns of a parent case (two of every kind of instance: backward fliers,
    slow and motionless ones at k = 0, k > 0 and at node H, terminal positions inside and outside the 1e-3 m clamp)."""
    c = cr.track_case(track, mode, H)
    n = 24
    tro = to.TrackOracle(c["points"])
    w = dict(to.DEFAULT_WEIGHTS, w_progress=0.0)
    X, U, s0 = np.array(c["X"][:, :, :n]), c["U"][:, :, :n], c["s0"][:n]
    nq, nx, ng, det = to.mhtt_model(tro, c["L"], X, s0, cr.DT, mode, w, detail=True)
    S = det["S"]
    br = cr.branches(dict(c, detail={k: v[..., :n] for k, v in det.items()}, s0=s0))
    for key in ("s_dot<0", "speed<0.1", "speed==0"):
        assert min(br[key]) >= 2, (key, br[key])
    assert br["speed<0.1@H"][0] >= 2 and br["dist<1e-3"][0] >= 2 and br["dist>1"][0] >= 2
    model = nq * (X - nx) + ng
    h = 1e-5
    loss = lambda Xq: to.mhtt_loss(tro, c["L"], Xq, U, S, w)  # noqa: E731
    clamp = det["dist"] < 1e-3
    worst = 0.0
    for k in range(H + 1):
        for r in range(6):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, r] += h; Xm[k, r] -= h
            fd = (loss(Xp) - loss(Xm)) / (2 * h)
            free = ~clamp if (k == H and r < 3) else np.ones(n, bool)
            err = np.abs(model[k, r] - fd)[free] / np.maximum(np.abs(fd[free]), 1.0)
            worst = max(worst, float(err.max()))
            assert (err < 2e-5).all(), (k, r, err.max())
    print(f"mhtt_model vs central differences [{track}, mode {mode}]: worst {worst:.2e}")
    # inside the clamp the model's curvature is w / 1e-3 (the gradient w d / |d| bounded as |d| -> 0)
    assert np.allclose(nq[H, :3][:, clamp], w["w_terminal_align"] / 1e-3, rtol=1e-15)
    assert not model[:, 6:].any()


def test_progress_gradient_counts_the_nodes_after_k():
    """only w_progress, mode 0, a straight track, no clip active: ng[k, 3:6] is the central difference of -w_p sum_j S_j through
    progress_initial with respect to v_k - tail = H - k, not H - k - 1 - and once the prediction reaches 1 the nodes from
    there on get zero"""
    P = cr.straight_points()
    tro = to.TrackOracle(P)
    L = tro.length()
    H, B = 5, 4
    rng = np.random.default_rng(3)
    X = np.zeros((H + 1, 13, B))
    X[:, :3] = rng.normal(0, 5, (H + 1, 3, B)); X[:, 3:6] = rng.uniform(20, 50, (H + 1, 1, B)) * np.array([1.0, 0.5, 0.25])[None, :, None] + rng.normal(0, 5, (H + 1, 3, B))
    s0 = np.array([0.2, 0.4, 0.6, 0.975])
    w = {k: 0.0 for k in to.DEFAULT_WEIGHTS}; w["w_progress"] = 5.0
    nq, nx, ng, det = to.mhtt_model(tro, L, X, s0, cr.DT, 0, w, detail=True)
    assert (det["pred"][:, :3] < 1).all() and (det["pred"][:, :3] > 0).all()      # no clip on instances 0..2
    hit = int(np.argmax(det["pred"][:, 3] >= 1))
    assert 0 < hit < H - 1 and (det["pred"][hit:, 3] >= 1).all()                   # instance 3 reaches the end at node `hit`
    h = 1e-4
    for k in range(H):
        for r in range(3, 6):
            Xp, Xm = X.copy(), X.copy()
            Xp[k, r] += h; Xm[k, r] -= h
            f = lambda Xq: -5.0 * to.progress_initial(tro, L, Xq, s0, cr.DT)[1:].sum(axis=0)  # noqa: E731
            fd = (f(Xp) - f(Xm)) / (2 * h)
            assert np.allclose(ng[k, r, :3], fd[:3], rtol=1e-6, atol=1e-12), (k, r)
        that = np.array([1.0, 0.5, 0.25]) / np.linalg.norm([1.0, 0.5, 0.25])
        assert np.allclose(ng[k, 3:6, 0], -5.0 * (H - k) * cr.DT * that / L, rtol=1e-12)
    assert not ng[hit:, :, 3].any() and ng[:hit, 3:6, 3].all()
    assert not ng[:, :3].any() and not nq[:H].any()      # mode 0: no position gradient; w_tracking = 0: no curvature


def test_structural_zeros_of_the_model():
    """mode 0 has no position gradient; rows 6..12 of all three arrays, and every velocity entry of nq and nx, are exactly 0"""
    for track in cr.TRACKS:
        for mode in (0, 1):
            for H in cr.TRACK_H:
                nq, nx, ng = cr.track_case(track, mode, H)["model"]
                assert not nq[:, 3:].any() and not nx[:, 3:].any() and not ng[:, 6:].any()
                if mode == 0:
                    assert not ng[:, :3].any()
                else:
                    assert ng[:H, :3].any()
                assert not ng[H, :3].any()


def test_mhtt_model_hand_computed():
    """A straight track of 140 m along x (t^ = e_x), dt = 0.01, H = 2, mode 1, default weights, s0 = 0.1:
    node 0 at (10, 3) flying forward at 50 m/s, node 1 flying backward at 20 m/s, node 2 half a millimetre from the end of the
    track at 0.06 m/s."""
    L, dt = 140.0, 0.01
    P = np.stack([np.linspace(0, L, 8), np.zeros(8), np.full(8, -200.0)], axis=1)
    tro = to.TrackOracle(P)
    X = np.zeros((3, 13, 1))
    X[0, :6, 0] = [10, 3, -200, 50, 0, 0]
    X[1, :6, 0] = [10.5, 3, -200, -20, 0, 0]
    X[2, :6, 0] = [140, 0.0005, -200, 0.06, 0, 0]
    nq, nx, ng, det = to.mhtt_model(tro, L, X, np.array([0.1]), dt, 1, detail=True)
    s1 = 0.1 + (50 / L) * dt + 0.05 * (10 - 14) / L
    assert np.isclose(det["S"][1, 0], s1, rtol=1e-14)
    assert np.allclose(nq[:2, :3, 0], 20.0) and np.allclose(nx[0, :3, 0], [14, 0, -200]) and np.allclose(nx[1, :3, 0], [L * s1, 0, -200])
    assert np.allclose(ng[0, :6, 0], [-5 * 2 * 0.05 / L, 0, 0, (-2 - 5 * 2 * dt) / L, 0, 0], rtol=1e-12, atol=1e-15)
    assert np.allclose(ng[1, :6, 0], [-5 * 1 * 0.05 / L, 0, 0, (-2 - 5 * 1 * dt + 2 * 50 * (-20 / L)) / L, 0, 0], rtol=1e-12, atol=1e-15)
    assert np.allclose(nq[2, :3, 0], 20 / 1e-3) and np.allclose(nx[2, :3, 0], [L, 0, -200])
    assert np.allclose(ng[2, :6, 0], [0, 0, 0, -2 * 10 * (0.1 - 0.06), 0, 0], rtol=1e-12)
    # the same trajectory in mode 0: no position correction, no position gradient
    _, _, ng0, d0 = to.mhtt_model(tro, L, X, np.array([0.1]), dt, 0, detail=True)
    assert np.isclose(d0["S"][1, 0], 0.1 + (50 / L) * dt, rtol=1e-14) and not ng0[:, :3].any() and np.allclose(ng0[:, 3:6], ng[:, 3:6])
    # per-term loss of the same trajectory
    U = np.zeros((2, 7, 1)); U[0, 0, 0] = 9.0; U[1, :2, 0] = [0.3, -0.4]
    S = det["S"]
    t, a = to.mhtt_loss_terms(tro, L, X, U, S)
    e0, e1 = 4.0 ** 2 + 9, (10.5 - L * s1) ** 2 + 9
    assert np.isclose(t["w_tracking"][0], 10 * (e0 + e1)) and np.isclose(t["w_progress"][0], -5 * (S[1, 0] + S[2, 0]))
    assert np.isclose(t["w_progress_rate"][0], -2 * (50 - 20) / L) and np.isclose(a["w_progress_rate"][0], 2 * (50 + 20) / L)
    assert np.isclose(t["w_backward"][0], 50 * (20 / L) ** 2) and np.isclose(t["w_low_velocity"][0], 10 * 0.04 ** 2)
    assert np.isclose(t["w_terminal_align"][0], 20 * 0.0005) and np.isclose(t["w_control"][0], 100 * 0.25)   # u_0 is not counted


# ---- every case of the GPU matrix: the e32 condition, the branches -----------------------------------------------------------------------
@pytest.mark.parametrize("track", list(cr.TRACKS))
def test_track_cases_meet_the_condition_and_populate_every_branch(track):
    for mode in (0, 1):
        for H in cr.TRACK_H:
            c = cr.track_case(track, mode, H)
            e = cr.progress_e32(c)
            e.update({k: float(cr.term_err(c["f32_terms"][k], c["terms"][k], c["sabs"][k]).max()) for k in to.TERMS})
            for i, n in enumerate(("nq", "nx", "ng")):
                e.update({f"{n}.{g}": float(v.max()) for g, v in cr.group_err(c["f32"][3 + i], c["model"][i]).items()})
            print(f"e32[{track}, mode {mode}, H {H}] " + "  ".join(f"{k} {v:.1e}" for k, v in e.items() if v > 0))
            assert max(e.values()) <= cr.E32_MAX, (mode, H, e)
            assert e["S"] > 0 and e["s_dot"] > 0 and e["ng.v"] > 0 and e["nx.p"] > 0
            br = cr.branches(c)
            print(f"branches[{track}, mode {mode}, H {H}] {br}")
            for key, (at0, later) in br.items():
                if key == "s0 outside" and mode == 0:
                    assert at0 == 0          # 0 / 0 in the reference's initial guess too: left to mode 1
                    continue
                assert at0 >= 2, (key, at0)
                if H > 1:
                    assert later >= 2, (key, later)
            # ... and among the first 65 columns too (the B = 65 calls); column 0 (B = 1) flies backwards
            sub = cr.branches(dict(c, detail={k: v[..., :65] for k, v in c["detail"].items()}, s0=c["s0"][:65]))
            assert all(v[0] >= 2 for k, v in sub.items() if not (k == "s0 outside" and mode == 0)), sub
            assert (c["detail"]["s_dot"][:, 0] < 0).all()
            # S sticks at 1 / at 0 exactly, and a knot value of s0 is an fp32 number
            assert ((c["S"] == 1).sum() > 2) and ((c["S"] == 0).sum() > 2)


def test_goal_cases_meet_the_condition():
    for B, H in cr.GOAL_MODEL_SHAPES:
        for tr in (0, 6):
            c = cr.goal_model_case(B, H, tr)
            e = {}
            for i, n in enumerate(("nq", "nx", "ng")):
                e.update({f"{n}.{g}": float(v.max()) for g, v in cr.group_err(c["f32"][i], c["ref"][i]).items()})
            e["uglin"] = float(cr.rows_err(c["f32"][3], c["ref"][3]).max()); e["uhess"] = float(cr.rows_err(c["f32"][4], c["ref"][4]).max())
            print(f"e32[goal_model, B {B}, H {H}, time_row {tr}] " + "  ".join(f"{k} {v:.1e}" for k, v in e.items() if v > 0))
            # the attitude rows of the speed gradient cannot meet the condition on any input (2 epsilon sum_i dr_i/dq_j ~ 4e-7
            # left over from terms of ~6000): recorded in DESIGN.md section 5, they keep the whole-tensor assertion
            assert e.pop("ng.q") > 0.1
            assert max(e.values()) <= cr.E32_MAX, (B, H, tr, e)
            act = c["inp"]["active"][:B]
            if B >= 7:
                assert act.any() and not act.all()
            U = c["inp"]["U"][:, :, :B]
            if H > 1 and B >= 7:
                d = np.abs(U[1:] - U[:-1])
                assert (d == 0).any() and ((d > 0.05) & (d < 0.15)).any() and (d > 1).any() and ((d > 0) & (d < 3e-4)).any()
    for Bn, H in cr.GOAL_COST_SHAPES:
        for tr in (0, 6):
            for lam_on in (True, False):
                c = cr.goal_cost_case(Bn, H, tr, lam_on)
                e = {k: float(cr.term_err(c["f32"][k], c["ref"][k], c["sabs"][k]).max()) for k in io.GOAL_TERMS}
                print(f"e32[goal_terms, Bn {Bn}, H {H}, time_row {tr}, lam {lam_on}] " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
                assert max(e.values()) <= cr.E32_MAX, (Bn, H, tr, e)
                # columns 1 and 2: two ulp either side of the inequality
                X, s = c["inp"]["X"], np.tile(c["inp"]["lam"] / (2 * cr.W_AL), cr.GOAL_REPS)
                if lam_on:
                    v = X[H, 3, 1:3] - cr.VX_MAX + s[1:3]
                    assert v[0] > 0 > v[1] and np.abs(v).max() < 1e-5


# ---- the metric can fail, and only where the mistake reaches -----------------------------------------------------------------------------
def _flagged(err, reach, name):
    """err (..., B) of the metric: above FLAG everywhere in `reach`, exactly zero elsewhere"""
    assert reach.any(), name
    assert not err[~reach].any(), (name, "moved something it cannot reach", np.argwhere((err > 0) & ~reach)[:4])
    assert (err[reach] > FLAG).all(), (name, "not flagged at", np.argwhere(reach & (err <= FLAG))[:4], float(err[reach].min()))
    print(f"mutant[{name}] reaches {int(reach.sum())} entries, smallest figure there {err[reach].min():.2e}")


@pytest.mark.parametrize("mode", [0, 1])
def test_metric_flags_the_track_mutants(mode):
    """tail = H - k - 1, `slow` without its k > 0 guard, `back` applied for s_dot > 0, the terminal distance clamp removed, the
    effort sum starting at k = 0 - each applied to the float64 reference of the arc parent at H = 12: above 1e-5 at every
    (node, instance) of the group, or instance of the term, that the change reaches; exactly zero at every other entry of
    every array and term."""
    c = cr.track_case("arc", mode, 12)
    nq, nx, ng = c["model"]
    d, H, B, L = c["detail"], 12, c["B"], c["L"]
    w = to.DEFAULT_WEIGHTS
    X = c["X"]
    none = np.zeros((H + 1, B), bool)

    def model_errs(mq, mx, mg):
        return {f"{n}.{g}": v for n, (a, r) in dict(nq=(mq, nq), nx=(mx, nx), ng=(mg, ng)).items() for g, v in cr.group_err(a, r).items()}

    def expect(name, errs, reach):   # reach: {key: (H+1, B) mask}; every other key must be exactly zero everywhere
        for k, e in errs.items():
            if k in reach:
                _flagged(e, reach[k], f"{name}:{k}")
            else:
                assert not e.any(), (name, k)

    # tail = H - k - 1
    live = np.concatenate([d["pred"] < 1, np.zeros((1, B), bool)]) & np.concatenate([np.abs(d["that"]).max(axis=1) > 0, np.zeros((1, B), bool)])
    mg = np.array(ng)
    mg[:H, 3:6] += np.where(d["pred"] < 1, w["w_progress"] * cr.DT, 0.0)[:, None] * d["that"] / L
    if mode:
        mg[:H, :3] += np.where(d["pred"] < 1, w["w_progress"] * 0.05, 0.0)[:, None] * d["that"] / L
    expect("tail_off_by_one", model_errs(nq, nx, mg), {"ng.v": live, **({"ng.p": live} if mode else {})})
    # slow without the k > 0 guard
    sp0 = d["speed"][0]
    mg = np.array(ng)
    mg[0, 3:6] += np.where(sp0 < 0.1, -2 * w["w_low_velocity"] * (0.1 - sp0) / np.maximum(sp0, 1e-6), 0.0) * X[0, 3:6]
    reach = none.copy(); reach[0] = (sp0 < 0.1) & (sp0 > 0)
    expect("slow_at_k0", model_errs(nq, nx, mg), {"ng.v": reach})
    # back applied for s_dot > 0
    mg = np.array(ng)
    mg[:H, 3:6] += np.where(d["s_dot"] > 0, 2 * w["w_backward"] * d["s_dot"], 0.0)[:, None] * d["that"] / L
    reach = none.copy(); reach[:H] = d["s_dot"] > 0
    expect("back_for_forward", model_errs(nq, nx, mg), {"ng.v": reach})
    # terminal dist clamp removed
    mq = np.array(nq)
    mq[H, :3] = np.where(d["dist"] < 1e-3, w["w_terminal_align"] / d["dist"], nq[H, :3])
    reach = none.copy(); reach[H] = d["dist"] < 1e-3
    expect("dist_clamp_removed", model_errs(mq, nx, ng), {"nq.p": reach})
    # effort sum from k = 0
    terms = dict(c["terms"])
    terms["w_control"] = terms["w_control"] + w["w_control"] * (c["U"][0] ** 2).sum(axis=0)
    for k in to.TERMS:
        e = cr.term_err(terms[k], c["terms"][k], c["sabs"][k])
        if k == "w_control":
            _flagged(e, np.ones(B, bool), "effort_from_k0")
        else:
            assert not e.any()
    # ... and on the sum under the default weights
    e = cr.term_err(sum(terms.values()), sum(c["terms"].values()), sum(c["sabs"].values()))
    assert (e > FLAG).all()


def test_metric_flags_the_goal_mutants():
    """the height term dropped, time_row not excluded, column o read as instance o / reps, the speed gradient x 1.25 - each
    applied to the float64 reference: flagged in the term or group it touches, exactly zero in every other"""
    orc = cr._oracle()
    c = cr.goal_cost_case(86, 7, 6)
    i, g, n = c["inp"], c["g"], 258
    ref = {k: v[:n] for k, v in c["ref"].items()}; sabs = {k: v[:n] for k, v in c["sabs"].items()}

    def only(name, terms, touched, reach=None):
        for k in io.GOAL_TERMS:
            e = cr.term_err(terms[k], ref[k], sabs[k])
            if k in touched:
                _flagged(e, np.ones(n, bool) if reach is None else reach, f"{name}:{k}")
            else:
                assert not e.any(), (name, k)

    only("height_dropped", dict(ref, height=np.zeros(n)), {"height"})
    t, _ = io.goal_cost_terms(orc, cr.goal_loss(0), i["goal"], i["X"], i["U"], i["lam"])
    only("time_row_not_excluded", t, {"rate"})
    # column o read as instance o / reps instead of o % Bn
    o = np.arange(n)
    perm = o // cr.GOAL_REPS
    t, _ = io.goal_cost_terms(orc, g, i["goal"][:, perm], i["X"], i["U"], i["lam"][perm])
    wrong = perm != o % 86
    eg, ea = cr.term_err(t["goal"], ref["goal"], sabs["goal"]), cr.term_err(t["al"], ref["al"], sabs["al"])
    _flagged(eg, wrong, "column_o_div_reps:goal")
    assert not ea[~wrong].any() and (ea[wrong] > FLAG).mean() > 0.5       # (two instances may share lam = 0)
    for k in ("rate", "height", "speed", "vx", "vyz"):
        assert not cr.term_err(t[k], ref[k], sabs[k]).any()
    # model: speed gradient x 1.25; time row not excluded
    m = cr.goal_model_case(37, 7, 6)
    nq, nx, ng, ug, uh = m["ref"]
    H, PB = 7, ng.shape[2]
    mg = np.array(ng); mg[:H, 3:10] *= 1.25
    errs = cr.group_err(mg, ng)
    reach = np.zeros((H + 1, PB), bool); reach[:H] = True
    _flagged(errs["v"], reach, "speed_gradient_x1.25:ng.v")
    _flagged(errs["q"], reach, "speed_gradient_x1.25:ng.q")
    assert not errs["p"].any() and not errs["w"].any()
    mi = m["inp"]
    r0 = io.goal_model(orc, cr.goal_loss(0), mi["goal"], mi["X"], mi["U"], mi["lam"])
    for a, b in zip(r0[:3], m["ref"][:3]):
        assert np.array_equal(a, b)
    for a, b, nm in ((r0[3], ug, "uglin"), (r0[4], uh, "uhess")):
        assert np.array_equal(a[:, :6], b[:, :6]) and not b[:, 6].any()
        # (every node of every instance is touched; where the row's difference is far beyond sqrt(eps) its l0' and l0'' are
        # e^-100 and below, so the figure is asserted where the row's own entry is visible at all)
        e = cr.rows_err(a, b)
        seen = np.abs(a[:, 6]) > 1e-3 * np.abs(a).max(axis=(1, 2))[:, None]
        print(f"mutant[time_row_not_excluded:{nm}] visible at {int(seen.sum())} of {seen.size}, smallest figure there {e[seen].min():.2e}")
        assert seen.mean() > 0.5 and (e[seen] > FLAG).all()


def _present_goal_problem(B=10, H=14):
    """the inputs of tests/test_gpu_ilqr.py::_goal_problem, rolled out by the oracle"""
    from tests.helpers import make_aircraft, make_oracle, near_trim_problem

    ac = make_aircraft("poly", normalise=True)
    X0, U = near_trim_problem(B, H, seed=6)
    rng = np.random.default_rng(12)
    U = f32_exact(U + rng.normal(0, 0.1, U.shape) * (np.arange(7) < 3)[None, :, None])
    goal = f32_exact(np.stack([rng.uniform(5, 9, B), rng.uniform(-1, 1, B)]))
    orc = make_oracle(ac)
    X = f32_exact(orc.rollout(f32_exact(X0), U, 0.01))
    lam = f32_exact(np.random.default_rng(1).uniform(0, 40, B) * (np.arange(B) % 2))
    return orc, io.GoalLoss(w_al=4.0, vx_max=58.0), goal, X, U, lam


def test_whole_tensor_assertions_miss_the_height_term_and_most_of_the_speed_gradient():
    """On the problem of test_goal_acquisition_kernels_match_numpy (B = 10, H = 14, ~55 m/s, terminal weights 1000), the
    assertions that test makes - max|delta| <= 2e-5 max|ref| over the whole tensor - pass a loss without its height term
    and a model whose speed gradient is 18 % too large (25 % too large is beyond the allowance on the faster instances
    only); the per-term and per-group figures are far above any bar on every instance."""
    orc, g, goal, X, U, lam = _present_goal_problem()
    H = U.shape[0]
    want = io.goal_cost(orc, g, goal, X, U, lam)
    t, a = io.goal_cost_terms(orc, g, goal, X, U, lam)
    got = want - t["height"]
    print(f"height term {np.abs(t['height']).max():.2e} of a loss of {np.abs(want).max():.2e}; allowance {2e-5 * np.abs(want).max():.2e}")
    assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max()                     # the present assertion passes
    assert (cr.term_err(np.zeros_like(want), t["height"], a["height"]) == 1.0).all()   # the per-term figure is 1
    nq, nx, ng, ug, uh = io.goal_model(orc, g, goal, X, U, lam)
    allow = 2e-5 * np.abs(ng).max()
    over = np.abs(0.25 * ng[:H, 3:10]) > allow
    print(f"speed gradient up to {np.abs(ng[:H]).max():.3f} beside max|ng| {np.abs(ng).max():.0f}; allowance {allow:.3f}: "
          f"x 1.25 is beyond it at {int(over.sum())} of {over.size} entries, on {int(over.any(axis=(0, 1)).sum())} of {ng.shape[2]} instances")
    # the faster instances fly at up to 75 m/s here, so x 1.25 (up to 0.027) exceeds the allowance (0.02) on them and passes on
    # the slower ones; anything up to 18 % too large passes the present assertion on every instance
    missed = ~over.any(axis=(0, 1))
    assert over.any() and missed.sum() >= 2      # whole instances (the slower ones) on which x 1.25 passes
    mg = np.array(ng); mg[:H, 3:10] *= 1.18
    assert np.abs(mg - ng).max() <= allow                                              # the present assertion passes
    assert cr.group_err(mg, ng)["v"][:H].min() > 0.05                                  # every (node, instance): far above any bar
    mg = np.array(ng); mg[:H, 3:10] *= 1.25
    assert cr.group_err(mg, ng)["v"][:H].min() > 0.05
