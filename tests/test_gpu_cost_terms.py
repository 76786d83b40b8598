"""The cost kernels the solvers minimise, term by term and node by node, against the float64 oracle (tests/cost_terms_ref.py
states the metric and the bar rule): k_goal_cost / k_goal_model / k_goal_multiplier (csrc/ac_goal.hpp), k_track_eval /
k_track_progress / k_mhtt_loss (csrc/ac_track.hpp), k_ilqr_cost<NODE> (csrc/ac_ilqr.hpp).

Inputs are synthetic and fp32-exact: these kernels only read arrays, no dynamics kernel runs.  Every output is a view into
a NaN-filled buffer whose padding must stay bit-unchanged and whose inside must be finite; every input must be
bit-unchanged; a repeat of every call must be bit-identical.  Scalar losses run with one weight non-zero at a time, then
with all of them."""
import ctypes as C

import numpy as np
import pytest

import ilqr_oracle as io
import track_oracle as to
from tests import cost_terms_ref as cr
from tests.helpers import f32_exact, parity_report
from tests.test_gpu_riccati import assert_guards, bits_equal, dev, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ac(gpu):
    return cr._aircraft()


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


class Inputs:
    """device copies of named host arrays; unchanged() asserts that no kernel wrote to them"""

    def __init__(self, gpu, **arrays):
        self.t = {k: dev(v, gpu) for k, v in arrays.items()}
        self.before = {k: v.clone() for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def unchanged(self):
        for k, v in self.before.items():
            assert bits_equal(self.t[k], v), (k, "input modified")


def host(t):
    return t.cpu().numpy().astype(np.float64)


# ---- goal-acquisition loss --------------------------------------------------------------------------------------------------------------
def goal_struct(g, only=None):
    """ac_goal_loss of the oracle's GoalLoss; only = the one term whose weight stays non-zero"""
    from aircraft_amd import _lib

    w = dict(goal=g.w_goal, rate=g.w_rate, height=g.w_height, speed=g.w_speed, vx=g.w_vx, vyz=g.w_vyz, al=g.w_al)
    if only is not None:
        w = {k: (v if k == only else 0.0) for k, v in w.items()}
    return _lib.GoalLoss(w["goal"], w["rate"], g.eps_rate, w["height"], w["speed"], w["vx"], w["vyz"], g.vx_max, w["al"], g.time_row)


def goal_cost_call(ac, gpu, loss, inp, lam, pre):
    """cost = pre, then ac_goal_cost_f32 adds to it -> the guarded view's host copy; twice, bit-identical"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    Bc, H, Bn = inp["X"].shape[2], inp["U"].shape[0], inp["goal"].shape[1]
    runs = []
    for _ in range(2):
        buf = {"cost": guarded((Bc,), gpu)}
        buf["cost"][1].copy_(dev(pre, gpu))
        _lib.check(lib.ac_goal_cost_f32(ac._handle, C.byref(loss), ptr(inp["goal"]), ptr(lam), Bn, ptr(inp["X"]), ptr(inp["U"]),
                                        Bc, H, ptr(buf["cost"][1]), ac._stream()), "ac_goal_cost_f32")
        torch.cuda.synchronize()
        assert ac.last_launch()[:3] == ("k_goal_cost", (Bc + 255) // 256, 256)
        assert_guards(buf, "goal_cost")
        runs.append(buf["cost"][1])
    assert bits_equal(*runs), "a repeat of the call differs"
    inp.unchanged()
    return host(runs[0])


@pytest.mark.parametrize("time_row", [0, 6])
@pytest.mark.parametrize("Bn,H", cr.GOAL_COST_SHAPES)
def test_goal_cost_term_by_term(gpu, ac, Bn, H, time_row):
    """ac_goal_cost_f32 on a candidate batch of 3 Bn columns (column o -> instance o % Bn; 258 columns cross a block), adding to a
    pre-filled cost: each term alone and all together, with multipliers given, all zero, and NULL (= zero, bit for bit)."""
    rng = np.random.default_rng(5)
    for lam_on in (True, False):
        c = cr.goal_cost_case(Bn, H, time_row, lam_on)
        i, g, Bc = c["inp"], c["g"], c["Bc"]
        inp = Inputs(gpu, goal=i["goal"], X=i["X"], U=i["U"], lam=i["lam"] if lam_on else np.zeros(Bn))
        wide = len(c["ref"]["goal"])
        terms = list(io.GOAL_TERMS) + ["all"] if lam_on else ["al", "all"]
        got, ref, sabs, f32 = {}, {}, {}, {}
        for t in terms:
            r = c["ref"][t] if t != "all" else sum(c["ref"].values())
            a = c["sabs"][t] if t != "all" else sum(c["sabs"].values())
            f = c["f32"][t] if t != "all" else sum(c["f32"].values())      # (summed in float64: the estimate of fp32's cost per term)
            pre = f32_exact(rng.uniform(-0.5, 0.5, wide) * a)               # the kernel adds to what is there
            key = f"{t}" if lam_on else f"{t}(lam=0)"
            ref[key], sabs[key] = pre + r, np.abs(pre) + a
            f32[key] = (np.float32(pre) + np.float32(f)).astype(np.float64)
            loss = goal_struct(g, None if t == "all" else t)
            got[key] = goal_cost_call(ac, gpu, loss, inp, inp["lam"], pre[:Bc])
            if not lam_on:
                null = goal_cost_call(ac, gpu, loss, inp, None, pre[:Bc])
                assert np.array_equal(null, got[key]), "lam = NULL differs from lam = 0"
        out = cr.check_terms(f"goal_terms[Bn{Bn}-H{H}-t{time_row}-lam{int(lam_on)}]", got, ref, sabs, f32, B=Bc)
        print(f"goal_terms[Bn{Bn} H{H} time_row {time_row} lam {lam_on}] " + "  ".join(f"{k} {w:.1e}/{e:.1e}" for k, (w, e) in out.items()))


def goal_model_call(ac, gpu, loss, inp, lam, B, H, hz_pre):
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    runs = []
    for _ in range(2):
        bufs = {"nq": guarded((H + 1, 13, B), gpu), "nx": guarded((H + 1, 13, B), gpu), "ng": guarded((H + 1, 13, B), gpu),
                "ug": guarded((H, 7, B), gpu), "Hz": guarded((H, 21, 21, B), gpu)}
        bufs["Hz"][1].copy_(dev(hz_pre, gpu))
        _lib.check(lib.ac_goal_model_f32(ac._handle, C.byref(loss), ptr(inp["goal"]), ptr(lam), ptr(inp["X"]), ptr(inp["U"]), B, H,
                                         *(ptr(bufs[k][1]) for k in ("nq", "nx", "ng", "ug", "Hz")), ac._stream()), "ac_goal_model_f32")
        torch.cuda.synchronize()
        assert ac.last_launch()[:3] == ("k_goal_model", ((H + 1) * B + 255) // 256, 256)
        assert_guards(bufs, "goal_model")
        runs.append({k: v[1] for k, v in bufs.items()})
    for k in runs[0]:
        assert bits_equal(runs[0][k], runs[1][k]), (k, "a repeat of the call differs")
    inp.unchanged()
    return runs[0]


def columns(c, sl, lam_on=True):
    i = c["inp"]
    return dict(goal=np.ascontiguousarray(i["goal"][:, sl]), X=np.ascontiguousarray(i["X"][:, :, sl]), U=np.ascontiguousarray(i["U"][:, :, sl]),
                lam=np.ascontiguousarray(i["lam"][sl]) if lam_on else np.zeros(len(i["lam"][sl])))


@pytest.mark.parametrize("time_row", [0, 6])
@pytest.mark.parametrize("B,H", cr.GOAL_MODEL_SHAPES)
def test_goal_model_node_by_node(gpu, ac, B, H, time_row):
    """ac_goal_model_f32, one lane per (node, instance): (H + 1) B crosses 256 with B not dividing it; H = 1 has no control
    difference, H = 2 one neighbour only.  Hz arrives filled with an arbitrary tensor: only its seven (u, u) diagonal entries
    may change, by the reference's increment."""
    c = cr.goal_model_case(B, H, time_row)
    g = c["g"]
    PB = c["ref"][0].shape[2]
    rng = np.random.default_rng(9)
    hz_wide = f32_exact(rng.normal(0, 30, (H, 21, 21, PB)))
    hz_pre = np.ascontiguousarray(hz_wide[..., :B])
    inp = Inputs(gpu, **columns(c, slice(0, B)))
    out = goal_model_call(ac, gpu, goal_struct(g), inp, inp["lam"], B, H, hz_pre)
    nq, nx, ng, ug, uh = c["ref"]
    # Hz: all but the diagonal of the (u, u) block bit-equal to what was there
    Hz = out["Hz"].cpu().numpy()
    idx = np.arange(13, 20)
    rest = Hz.copy(); rest[:, idx, idx] = hz_pre[:, idx, idx].astype(np.float32)
    assert np.array_equal(rest.view(np.int32), hz_pre.astype(np.float32).view(np.int32)), "Hz changed outside the (u, u) diagonal"
    pre_d = np.stack([hz_wide[:, 13 + r, 13 + r] for r in range(7)], axis=1)           # (H, 7, PB)
    got_d = np.stack([Hz[:, 13 + r, 13 + r] for r in range(7)], axis=1).astype(np.float64)
    f32_d = (np.float32(pre_d) + np.float32(c["f32"][4])).astype(np.float64)
    # (the sum is compared, on the scale of the increments: |pre| <= ~100 beside increments of ~2e4)
    arrays = {"nq": (host(out["nq"]), nq, c["f32"][0]), "nx": (host(out["nx"]), nx, c["f32"][1]), "ng": (host(out["ng"]), ng, c["f32"][2]),
              "uglin": (host(out["ug"]), ug, c["f32"][3])}
    res = cr.check_groups(f"goal_model[B{B}-H{H}-t{time_row}]", arrays, skip={("ng", "q")})
    if H > 1:
        e32 = float(cr.rows_err(f32_d - pre_d, uh).max())
        e = cr.rows_err(np.concatenate([got_d - pre_d[..., :B], uh[..., B:]], axis=-1), uh)[:, :B]
    else:
        e32, e = 0.0, np.zeros(1)
        assert np.array_equal(got_d, pre_d[..., :B]) and not uh.any()       # no control difference: Hz untouched
    bar = cr.bar_of(e32, "Hz diagonal")
    parity_report(f"goal_model[B{B}-H{H}-t{time_row}].Hz", worst=float(e.max()), e32=e32, ratio=float(e.max() / e32) if e32 else 0.0)
    assert (e <= bar).all(), ("Hz diagonal beyond", bar, float(e.max()))
    # the attitude rows of the speed gradient (fp32 restatement 0.5 .. 0.9 of their own 4e-7: DESIGN.md section 5) and everything
    # else once more on the whole tensor, as before
    assert np.abs(host(out["ng"]) - ng[..., :B]).max() <= 2e-5 * np.abs(ng).max()
    print(f"goal_model[B{B} H{H} time_row {time_row}] " + "  ".join(f"{k} {w:.1e}/{e:.1e}" for k, (w, e) in res.items()) + f"  Hz {e.max():.1e}/{e32:.1e}")
    # multipliers NULL = multipliers zero, bit for bit, and both the reference without multipliers
    c0 = cr.goal_model_case(B, H, time_row, False)
    inp0 = Inputs(gpu, **columns(c0, slice(0, B), lam_on=False))
    z = goal_model_call(ac, gpu, goal_struct(g), inp0, inp0["lam"], B, H, hz_pre)
    n = goal_model_call(ac, gpu, goal_struct(g), inp0, None, B, H, hz_pre)
    assert all(bits_equal(z[k], n[k]) for k in z), "lam = NULL differs from lam = 0"
    cr.check_groups(f"goal_model[B{B}-H{H}-t{time_row}-lam0]", {"nq": (host(z["nq"]), c0["ref"][0], c0["f32"][0]),
                                                                "nx": (host(z["nx"]), c0["ref"][1], c0["f32"][1])})
    if B == 37:   # one lane per (node, instance): a piece of the batch reproduces its columns
        sl = slice(16, 37)
        sub = goal_model_call(ac, gpu, goal_struct(g), Inputs(gpu, **columns(c, sl)), dev(c["inp"]["lam"][sl], gpu), 21, H,
                              np.ascontiguousarray(hz_pre[..., sl]))
        for k in sub:
            assert bits_equal(sub[k], out[k][..., sl]), (k, "columns 16:37 differ from the parent batch")


@pytest.mark.parametrize("B", [1, 37, 257])
def test_goal_multiplier(gpu, ac, B):
    """lam <- max(0, lam + 2 w_al (v_x(N) - vx_max)) from multipliers at zero, positive, and driven to the clamp at 0; the excess
    reported or not (NULL) without a bit of difference in lam"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    H = 2
    c = cr.goal_model_case(257, H, 0)
    g, X = c["g"], c["inp"]["X"]
    exc = X[H, 3] - g.vx_max
    lams = {"zero": np.zeros(257), "positive": c["inp"]["lam"] + 1.0,
            "clamped": f32_exact(np.where(exc < 0, -1.5 * g.w_al * exc, 1.0))}       # lam + 2 w exc < 0 wherever the excess is negative
    Xd = Inputs(gpu, X=np.ascontiguousarray(X[:, :, :B]))
    for name, lam in lams.items():
        want, vw = io.goal_multiplier(g, X, lam)
        l32 = np.maximum(np.float32(0), np.float32(lam) + np.float32(2 * g.w_al) * (np.float32(X[H, 3]) - np.float32(g.vx_max))).astype(np.float64)
        sabs = np.abs(lam) + np.abs(2 * g.w_al * exc)
        res = []
        for with_viol in (True, False):
            bufs = {"lam": guarded((B,), gpu)}
            if with_viol:
                bufs["viol"] = guarded((B,), gpu)
            bufs["lam"][1].copy_(dev(lam[:B], gpu))
            _lib.check(lib.ac_goal_multiplier_f32(ac._handle, C.byref(goal_struct(g)), ptr(Xd["X"]), B, H, ptr(bufs["lam"][1]),
                                                  ptr(bufs["viol"][1] if with_viol else None), ac._stream()), "ac_goal_multiplier_f32")
            torch.cuda.synchronize()
            assert_guards(bufs, "goal_multiplier")
            res.append(bufs)
        Xd.unchanged()
        assert bits_equal(res[0]["lam"][1], res[1]["lam"][1])
        got = host(res[0]["lam"][1])
        out = cr.check_terms(f"goal_multiplier[B{B}-{name}]", {"lam": got}, {"lam": want}, {"lam": sabs}, {"lam": l32}, B=B)
        assert cr.zeros_kept(got, want[:B])
        assert np.array_equal(host(res[0]["viol"][1]), np.maximum(0.0, exc[:B]))      # one exact subtraction of fp32 numbers
        if name == "clamped":
            assert (want[:B] == 0).sum() >= min(B, 2) or B == 1
        print(f"goal_multiplier[B{B} {name}] {out['lam'][0]:.1e}/{out['lam'][1]:.1e}")


# ---- track ---------------------------------------------------------------------------------------------------------------------------------
def install(ac, points):
    from aircraft_amd.control.track import Track

    tr = Track(points)
    tr.install(ac)
    return tr


def mhtt_struct(w):
    from aircraft_amd import _lib

    return _lib.MhttWeights(*(float(w[k]) for k in ("w_tracking", "w_progress", "w_progress_rate", "w_backward", "w_terminal_align",
                                                      "w_low_velocity", "w_control")))


@pytest.mark.parametrize("n", cr.TRACK_EVAL_N)
@pytest.mark.parametrize("track", list(cr.TRACKS))
def test_track_eval_point_by_point(gpu, ac, track, n):
    """ac_track_eval_f32 at n = 1 (an interior knot: counted twice), 255, 256, 257 points: every point's position within
    8 x e32 relative to max(|pos|, 1 m), every tangent within 8 x e32 of the track's largest"""
    import torch
    from aircraft_amd import _lib

    c = cr.track_eval_case(track)
    install(ac, c["points"])
    lib = ac._sync()
    e32p, e32t = (float(v.max()) for v in cr.track_point_err(*c["f32"], c))
    bp, bt = cr.bar_of(e32p, "pos"), cr.bar_of(e32t, "tan")
    s = Inputs(gpu, s=c["s"][:n])
    runs = []
    for _ in range(2):
        bufs = {"pos": guarded((3, n), gpu), "tan": guarded((3, n), gpu)}
        _lib.check(lib.ac_track_eval_f32(ac._handle, ptr(s["s"]), n, ptr(bufs["pos"][1]), ptr(bufs["tan"][1]), ac._stream()), "ac_track_eval_f32")
        torch.cuda.synchronize()
        assert_guards(bufs, "track_eval")
        runs.append(bufs)
    s.unchanged()
    assert bits_equal(runs[0]["pos"][1], runs[1]["pos"][1]) and bits_equal(runs[0]["tan"][1], runs[1]["tan"][1])
    pos, tan = host(runs[0]["pos"][1]), host(runs[0]["tan"][1])
    ep, et = cr.track_point_err(pos, tan, c, n)
    parity_report(f"track_eval[{track}-n{n}]", worst_pos=float(ep.max()), e32_pos=e32p, worst_tan=float(et.max()), e32_tan=e32t)
    print(f"track_eval[{track} n{n}] pos {ep.max():.1e}/{e32p:.1e} tan {et.max():.1e}/{e32t:.1e}")
    assert (ep <= bp).all(), ("position beyond", bp, np.flatnonzero(ep > bp)[:8], float(ep.max()))
    assert (et <= bt).all(), ("tangent beyond", bt, np.flatnonzero(et > bt)[:8], float(et.max()))
    assert cr.zeros_kept(tan, c["tan"][:, :n])                 # outside [0, 1]: zero tangent
    assert np.allclose(pos[:, 0], 2 * c["points"][16], rtol=1e-6)   # s = 0.5 = knot 16: both segments count it


TRACK_CASES = [(t, m, B, H) for t in cr.TRACKS for m in (0, 1) for H in cr.TRACK_H for B in cr.TRACK_B]


def progress_call(ac, gpu, inp, w, mode, B, H, model):
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    bufs = {"S": guarded((H + 1, B), gpu), "sd": guarded((H, B), gpu), "e2": guarded((H, B), gpu)}
    if model:
        bufs.update(nq=guarded((H + 1, 13, B), gpu), nx=guarded((H + 1, 13, B), gpu), ng=guarded((H + 1, 13, B), gpu))
    m = [ptr(bufs[k][1]) if model else ptr(None) for k in ("nq", "nx", "ng")] if model else [ptr(None)] * 3
    _lib.check(lib.ac_track_progress_f32(ac._handle, C.byref(mhtt_struct(w)), ptr(inp["X"]), ptr(inp["s0"]), C.c_float(cr.DT), B, H, mode,
                                         ptr(bufs["S"][1]), ptr(bufs["sd"][1]), ptr(bufs["e2"][1]), *m, ac._stream()), "ac_track_progress_f32")
    torch.cuda.synchronize()
    assert ac.last_launch()[:3] == ("k_track_progress", (B + 255) // 256, 256)
    assert_guards(bufs, "track_progress")
    inp.unchanged()
    return {k: v[1] for k, v in bufs.items()}


@pytest.mark.parametrize("track,mode,B,H", TRACK_CASES, ids=[f"{t}-m{m}-B{B}-H{H}" for t, m, B, H in TRACK_CASES])
def test_progress_and_node_model(gpu, ac, track, mode, B, H):
    """ac_track_progress_f32 on instances that enter every branch (tests/test_cost_terms_ref.py asserts the inventory): S, s_dot
    and err2 per instance, the node model per (node, instance, row group); with the model outputs NULL, S is the same bit for
    bit."""
    c = cr.track_case(track, mode, H)
    e32 = cr.progress_e32(c)
    bars = {k: cr.bar_of(v, k) for k, v in e32.items()}                       # conditions first
    install(ac, c["points"])
    inp = Inputs(gpu, X=np.ascontiguousarray(c["X"][:, :, :B]), s0=c["s0"][:B])
    w = to.DEFAULT_WEIGHTS
    out = progress_call(ac, gpu, inp, w, mode, B, H, True)
    again = progress_call(ac, gpu, inp, w, mode, B, H, True)
    bare = progress_call(ac, gpu, inp, w, mode, B, H, False)
    assert all(bits_equal(out[k], again[k]) for k in out), "a repeat of the call differs"
    assert all(bits_equal(out[k], bare[k]) for k in bare), "S / s_dot / err2 depend on whether the model is asked for"
    S, sd, e2 = host(out["S"]), host(out["sd"]), host(out["e2"])
    # the bars the suite had
    assert np.abs(S - c["S"][:, :B]).max() < 2e-6
    assert np.abs(sd - c["s_dot"][:, :B]).max() <= 1e-5 * np.abs(c["s_dot"]).max()
    assert np.abs(e2 - c["err2"][:, :B]).max() <= 1e-4 * np.abs(c["err2"]).max()
    # per instance
    errs = {"S": cr.inst_err(S, c["S"][:, :B], scale=1.0), "s_dot": cr.inst_err(sd, c["s_dot"][:, :B], scale=c["sd_scale"][:B]),
            "err2": cr.inst_err(e2, c["err2"][:, :B])}
    parity_report(f"progress[{track}-m{mode}-B{B}-H{H}]", **{k: dict(worst=float(v.max()), e32=e32[k], ratio=float(v.max() / e32[k])) for k, v in errs.items()})
    for k, v in errs.items():
        assert (v <= bars[k]).all(), (k, "beyond", bars[k], "at instances", np.flatnonzero(v > bars[k])[:8].tolist(), float(v.max()))
    assert cr.zeros_kept(S, c["S"][:, :B]) and ((S == 1) == (c["S"][:, :B] == 1)).all()     # the clip: exactly 0, exactly 1
    assert cr.zeros_kept(sd, c["s_dot"][:, :B])
    names = ("nq", "nx", "ng")
    res = cr.check_groups(f"mhtt_model[{track}-m{mode}-B{B}-H{H}]",
                          {n: (host(out[n]), c["model"][i], c["f32"][3 + i]) for i, n in enumerate(names)})
    print(f"progress[{track} m{mode} B{B} H{H}] " + "  ".join(f"{k} {float(v.max()):.1e}/{e32[k]:.1e}" for k, v in errs.items()) + "  "
          + "  ".join(f"{k} {w_:.1e}/{e:.1e}" for k, (w_, e) in res.items() if e > 0))


@pytest.mark.parametrize("track,mode,B,H", TRACK_CASES, ids=[f"{t}-m{m}-B{B}-H{H}" for t, m, B, H in TRACK_CASES])
def test_mhtt_loss_term_by_term(gpu, ac, track, mode, B, H):
    """ac_mhtt_loss_f32 on the same instances and their progress sequences (rounded to fp32; S_0 outside [0, 1], values stuck
    at 0 and at 1, on knots): each weight alone, then the defaults.  H = 1 has no effort term, H = 2 takes it from u_1 only."""
    import torch
    from aircraft_amd import _lib

    c = cr.track_case(track, mode, H)
    install(ac, c["points"])
    lib = ac._sync()
    inp = Inputs(gpu, X=np.ascontiguousarray(c["X"][:, :, :B]), U=np.ascontiguousarray(c["U"][:, :, :B]), S=np.ascontiguousarray(c["Sin"][:, :B]))
    got, ref, sabs, f32 = {}, {}, {}, {}
    for label, w in cr.weights_one_hot():
        runs = []
        for _ in range(2):
            buf = {"J": guarded((B,), gpu)}
            _lib.check(lib.ac_mhtt_loss_f32(ac._handle, C.byref(mhtt_struct(w)), ptr(inp["X"]), ptr(inp["U"]), ptr(inp["S"]), B, H,
                                            ptr(buf["J"][1]), ac._stream()), "ac_mhtt_loss_f32")
            torch.cuda.synchronize()
            assert_guards(buf, "mhtt_loss")
            runs.append(buf["J"][1])
        assert bits_equal(*runs), "a repeat of the call differs"
        got[label] = host(runs[0])
        if label == "all":
            ref[label], sabs[label], f32[label] = sum(c["terms"].values()), sum(c["sabs"].values()), sum(v.astype(np.float64) for v in c["f32_terms"].values())
        else:
            ref[label], sabs[label], f32[label] = c["terms"][label], c["sabs"][label], c["f32_terms"][label]
    inp.unchanged()
    if H == 1:
        assert not got["w_control"].any() and not ref["w_control"].any()
    out = cr.check_terms(f"mhtt_terms[{track}-m{mode}-B{B}-H{H}]", got, ref, sabs, f32, B=B)
    print(f"mhtt_terms[{track} m{mode} B{B} H{H}] " + "  ".join(f"{k} {w:.1e}/{e:.1e}" for k, (w, e) in out.items()))


# ---- quadratic cost kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("B", cr.QUAD_B)
def test_quadratic_cost_term_by_term(gpu, ac, B, wide):
    """ac_ilqr_cost_f32 and ac_ilqr_cost_node_f32 with q, qf, r, u_lin (node_q, node_glin, r, u_lin) each alone, on a plain batch and
    on a line-search-wide one (column a B + b reads node column b)."""
    import copy

    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    c = cr.quad_case(wide)
    H, na = cr.QUAD_H, c["na"]
    Xp, Up, nodep = cr.quad_columns(c, max(cr.QUAD_B))          # parent: e32 over 65 (195) instances
    X, U, node = cr.quad_columns(c, B)
    inp = Inputs(gpu, X=X, U=U, nq=node[0], nx=node[1], ng=node[2])
    zero13, zero7 = [0.0] * 13, [0.0] * 7
    for use_node in (False, True):
        ref, sabs = cr.quad_terms_np(np.float64, c["cost"], Xp, Up, nodep if use_node else None)
        f32, _ = cr.quad_terms_np(np.float32, c["cost"], Xp, Up, nodep if use_node else None)
        assert np.allclose(sum(ref.values()), io.cost(c["cost"], Xp, Up, node=nodep if use_node else None), rtol=1e-12)
        # parent columns a 65 + b -> the case's columns a B + b
        pick = (np.arange(na)[:, None] * max(cr.QUAD_B) + np.arange(B)[None, :]).reshape(-1)
        got, r_, a_, f_ = {}, {}, {}, {}
        for label in list(ref) + ["all"]:
            cost = copy.deepcopy(c["cost"])
            if label != "all":
                cost.q, cost.qf = (cost.q if label == "q" else zero13), (cost.qf if label == "qf" else zero13)
                cost.r, cost.u_lin = (cost.r if label == "r" else zero7), (cost.u_lin if label == "u_lin" else zero7)
            z = torch.zeros_like(inp["nq"])
            nq = inp["nq"] if label in ("node_q", "all") else z
            ng = inp["ng"] if label in ("node_glin", "all") else z
            runs = []
            for _ in range(2):
                buf = {"J": guarded((na * B,), gpu)}
                if use_node:
                    _lib.check(lib.ac_ilqr_cost_node_f32(ac._handle, C.byref(cost.struct()), ptr(nq), ptr(inp["nx"]), ptr(ng), B, ptr(inp["X"]),
                                                         ptr(inp["U"]), na * B, H, ptr(buf["J"][1]), ac._stream()), "ac_ilqr_cost_node_f32")
                else:
                    _lib.check(lib.ac_ilqr_cost_f32(ac._handle, C.byref(cost.struct()), ptr(inp["X"]), ptr(inp["U"]), na * B, H, ptr(buf["J"][1]),
                                                    ac._stream()), "ac_ilqr_cost_f32")
                torch.cuda.synchronize()
                assert_guards(buf, "ilqr_cost")
                runs.append(buf["J"][1])
            assert bits_equal(*runs), "a repeat of the call differs"
            got[label] = host(runs[0])
            src = (lambda d: sum(v.astype(np.float64) for v in d.values())) if label == "all" else (lambda d: d[label])  # noqa: E731
            rest = np.setdiff1d(np.arange(len(src(ref))), pick)
            order = np.concatenate([pick, rest])                   # the case's columns first, the rest of the parent after them
            r_[label], a_[label], f_[label] = src(ref)[order], src(sabs)[order], src(f32)[order]
        inp.unchanged()
        name = f"quad_terms[{'node' if use_node else 'plain'}-B{B}-{'wide' if wide else 'one'}]"
        out = cr.check_terms(name, got, r_, a_, f_, B=na * B)
        print(name + " " + "  ".join(f"{k} {w:.1e}/{e:.1e}" for k, (w, e) in out.items()))
