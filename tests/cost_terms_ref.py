"""Term-by-term checks of the cost kernels the solvers minimise (TEST INFRASTRUCTURE, NOT PRODUCT): the goal-acquisition
loss, its quadratic model and multiplier (csrc/ac_goal.hpp), the track tracker's progress recursion, node model and loss
(csrc/ac_track.hpp), the quadratic cost kernels (csrc/ac_ilqr.hpp).

References (float64): oracle/ilqr_oracle.py (goal_cost_terms, goal_model, goal_multiplier, cost) and oracle/track_oracle.py
(progress_initial, progress_tight, mhtt_loss_terms, mhtt_model).

Metric.  A scalar loss is compared term by term: the kernel runs with one weight non-zero at a time, and per instance the
error is |J - ref| / S_abs, S_abs = the sum of the absolute values of the term's summands.  A model array is compared per
(node, instance, row group p / v / q / omega): max|delta| over the group / max|ref| over that group and node across the
case; control arrays per (node, instance) over their seven rows.  What the reference has exactly zero must be exactly zero.

Bar.  8 x e32, where e32 is the worst such error of the np.float32 restatements below against the float64 reference on
the case's own inputs (never of the GPU), under the condition e32 <= 1.25e-6, asserted before a GPU result is looked at: no
bar exceeds 1e-5.  e32 is a maximum over at least 64 instances: a case narrower than that is the leading columns of a wider
parent batch (or, where columns map to instances, is joined by a 64-wide batch of the same generator), so that one
instance's lucky rounding does not set the bar.  A case that breaks the condition gets other inputs, never a wider bar.
"""
import functools

import numpy as np

import ilqr_oracle as io
import track_oracle as to
from tests.helpers import BLOCKS, f32_exact, parity_report

E32_MAX = 1.25e-6
FACTOR = 8.0
EPSILON = 1e-6          # the dynamics' epsilon (v_rel = q^-1 v q + epsilon); the tests assert it is the aircraft's
PARENT = 64


# ---- metric ------------------------------------------------------------------------------------------------------------------
def _ratio(d, den):
    """d / den; where den == 0 the reference is exactly zero there: 0 if d is, inf otherwise"""
    with np.errstate(all="ignore"):
        out = np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isnan(out), np.inf, out)


def term_err(J, ref, sabs):
    """(B,) per instance |J - ref| / S_abs"""
    return _ratio(np.abs(np.asarray(J, np.float64) - ref), np.asarray(sabs, np.float64))


def group_err(a, ref):
    """state array (N, 13, B) -> {group: (N, B)}: max|a - ref| over the group / max|ref| over that group and node across the case"""
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    out = {}
    for name, sl in BLOCKS.items():
        d = np.abs(a[:, sl] - ref[:, sl]).max(axis=1)
        out[name] = _ratio(d, np.abs(ref[:, sl]).max(axis=(1, 2))[:, None] * np.ones_like(d))
    return out


def rows_err(a, ref):
    """(N, r, B) (or (N, B)) -> (N, B): max|a - ref| over the rows / max|ref| over that node across the case"""
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    if a.ndim == 2:
        a, ref = a[:, None], ref[:, None]
    d = np.abs(a - ref).max(axis=1)
    return _ratio(d, np.abs(ref).max(axis=(1, 2))[:, None] * np.ones_like(d))


def inst_err(a, ref, scale=None):
    """(N, B) per-node values -> (B,): max over nodes |a - ref| / the instance's scale (default max over nodes |ref|)"""
    a = np.asarray(a, np.float64); ref = np.asarray(ref, np.float64)
    den = np.abs(ref).max(axis=0) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), ref.shape[1:])
    return _ratio(np.abs(a - ref).max(axis=0), den)


def zeros_kept(a, ref):
    """entries the reference has exactly zero are exactly zero"""
    return bool((np.asarray(a)[np.asarray(ref) == 0] == 0).all())


def bar_of(e32, name=""):
    assert e32 <= E32_MAX, (name, "fp32 restatement vs float64:", e32, ">", E32_MAX, "- choose other inputs, never a wider bar")
    return FACTOR * e32


def check_terms(name, got, ref, sabs, f32, B=None, report=True):
    """Every (term, instance): term_err <= 8 x e32 of that term.  got / ref / sabs / f32: {term: (B,)}; f32 and the parent part
    of ref / sabs may be wider than got (the case is their leading B columns).  -> {term: (worst, e32)}"""
    out = {}
    for t in got:
        e32 = float(term_err(f32[t], ref[t], sabs[t]).max())
        bar = bar_of(e32, f"{name}:{t}")
        n = len(got[t]) if B is None else B
        e = term_err(got[t], ref[t][:n], sabs[t][:n])
        out[t] = (float(e.max()), e32)
        assert (e <= bar).all(), (name, t, "beyond", bar, "at instances", np.flatnonzero(e > bar)[:8].tolist(), "worst", float(e.max()))
    if report:
        parity_report(name, **{t: dict(worst=w, e32=e, ratio=(w / e if e > 0 else 0.0)) for t, (w, e) in out.items()})
    return out


def check_groups(name, arrays, skip=(), report=True):
    """arrays: {array name: (got, ref, f32)} of state arrays (N, 13, B) or control arrays (N, 7, B) / (N, B).  Every
    (node, instance, group) within 8 x e32 of that array and group; exact zeros kept.  `skip`: (array, group) pairs whose
    restatement cannot meet the condition (recorded in DESIGN.md); they keep their whole-tensor assertion only."""
    out = {}
    for an, (got, ref, f32) in arrays.items():
        n = np.asarray(got).shape[-1]
        assert zeros_kept(got, ref[..., :n]), (name, an, "an entry the reference has exactly zero is not")
        if np.asarray(ref).ndim == 3 and ref.shape[1] == 13:
            e32s = {g: float(v.max()) for g, v in group_err(f32, ref).items()}
            errs = {g: v[:, :n] for g, v in group_err(np.concatenate([got, ref[..., n:]], axis=-1), ref).items()}
        else:
            e32s = {"u": float(rows_err(f32, ref).max())}
            errs = {"u": rows_err(np.concatenate([got, ref[..., n:]], axis=-1), ref)[:, :n]}
        for g, e in errs.items():
            if (an, g) in skip:
                continue
            bar = bar_of(e32s[g], f"{name}:{an}:{g}")
            out[f"{an}.{g}"] = (float(e.max()), e32s[g])
            assert (e <= bar).all(), (name, an, g, "beyond", bar, "at (node, instance)",
                                      [tuple(int(i) for i in w) for w in np.argwhere(e > bar)[:8]], "worst", float(e.max()))
    if report:
        parity_report(name, **{k: dict(worst=w, e32=e, ratio=(w / e if e > 0 else 0.0)) for k, (w, e) in out.items()})
    return out


# ---- the goal-acquisition loss in a chosen precision -----------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.stack([aw * bx + bw * ax + (ay * bz - az * by), aw * by + bw * ay + (az * bx - ax * bz),
                     aw * bz + bw * az + (ax * by - ay * bx), aw * bw - (ax * bx + ay * by + az * bz)])


def speed_np(dtype, x, grad=False):
    """x (13, n) -> v_rel . v_rel (n,), v_rel = (q^-1 (v, 0) q)_vec + epsilon, quaternion rows 6..9 = (x, y, z, w); with
    grad=True also its gradient with respect to rows 3..9 (7, n): 2 sum_i v_rel_i d v_rel_i, d r = M dv + 2 r x (q^-1 dq)_vec."""
    x = np.asarray(x, dtype)
    q = x[6:10]
    qi = np.stack([-q[0], -q[1], -q[2], q[3]]) / (q * q).sum(axis=0)
    zero = np.zeros_like(x[0])
    r = _qmul(_qmul(qi, np.stack([x[3], x[4], x[5], zero])), q)[:3]
    vr = r + dtype(EPSILON)
    vv = (vr * vr).sum(axis=0)
    assert vv.dtype == dtype
    if not grad:
        return vv
    g = np.zeros((7,) + vv.shape, dtype)
    for a in range(3):
        e = np.zeros_like(q); e[a] = 1
        g[a] = 2 * (vr * _qmul(_qmul(qi, e), q)[:3]).sum(axis=0)
    for j in range(4):
        e = np.zeros_like(q); e[j] = 1
        g[3 + j] = 2 * (vr * (2 * np.cross(r, _qmul(qi, e)[:3], axis=0))).sum(axis=0)
    assert g.dtype == dtype
    return vv, g


def _l0(dtype, d, eps):
    return -np.expm1(-(d * d) / dtype(eps))


def goal_terms_np(dtype, g, goal, X, U, lam=None):
    """io.goal_cost_terms' values in `dtype` throughout -> {term: (Bc,)}"""
    t = lambda a: np.asarray(a, dtype)  # noqa: E731
    X, U, goal = t(X), t(U), t(goal)
    H, _, Bc = U.shape
    Bn = goal.shape[1]
    gl = np.tile(goal, (1, Bc // Bn))
    out = {}
    dx, dy = X[H, 0] - gl[0], X[H, 1] - gl[1]
    out["goal"] = dtype(g.w_goal) * (dx * dx + dy * dy)
    rows = io._rate_rows(g)
    out["rate"] = dtype(g.w_rate) * _l0(dtype, (U[1:] - U[:-1])[:, rows], g.eps_rate).sum(axis=(0, 1), dtype=dtype) if H > 1 else np.zeros(Bc, dtype)
    dz = X[H, 2] - X[0, 2]
    out["height"] = dtype(g.w_height) * (dz * dz)
    speed = np.zeros(Bc, dtype)
    for k in range(H):
        speed = speed + speed_np(dtype, X[k])
    out["speed"] = -(dtype(g.w_speed) / dtype(H)) * speed
    out["vx"] = dtype(g.w_vx) * X[H, 3]
    out["vyz"] = dtype(g.w_vyz) * (X[H, 4] * X[H, 4] + X[H, 5] * X[H, 5])
    out["al"] = np.zeros(Bc, dtype)
    if g.w_al > 0:
        s = np.tile((np.zeros(Bn, dtype) if lam is None else t(lam)) * (dtype(0.5) / dtype(g.w_al)), Bc // Bn)
        v = np.maximum(dtype(0), X[H, 3] - dtype(g.vx_max) + s)
        out["al"] = dtype(g.w_al) * (v * v - s * s)
    assert all(v.dtype == dtype for v in out.values())
    return out


def goal_model_np(dtype, g, goal, X, U, lam=None):
    """io.goal_model in `dtype` throughout -> nq, nx, ng (H+1, 13, B), uglin, uhess (H, 7, B)"""
    t = lambda a: np.asarray(a, dtype)  # noqa: E731
    X, U, goal = t(X), t(U), t(goal)
    H, _, B = U.shape
    nq = np.zeros((H + 1, 13, B), dtype); nx = np.zeros_like(nq); ng = np.zeros_like(nq)
    for k in range(H):
        ng[k, 3:10] = -(dtype(g.w_speed) / dtype(H)) * speed_np(dtype, X[k], grad=True)[1]
    nq[H, 0] = nq[H, 1] = dtype(2) * dtype(g.w_goal); nx[H, 0], nx[H, 1] = goal[0], goal[1]
    nq[H, 2] = dtype(2) * dtype(g.w_height); nx[H, 2] = X[0, 2]
    nq[H, 4] = nq[H, 5] = dtype(2) * dtype(g.w_vyz)
    ng[H, 3] = dtype(g.w_vx)
    if g.w_al > 0:
        s = (np.zeros(B, dtype) if lam is None else t(lam)) * (dtype(0.5) / dtype(g.w_al))
        act = X[H, 3] - dtype(g.vx_max) + s > 0
        nq[H, 3] = np.where(act, dtype(2) * dtype(g.w_al), dtype(0)); nx[H, 3] = np.where(act, dtype(g.vx_max) - s, dtype(0))
    eps = dtype(g.eps_rate)
    d = U[1:] - U[:-1]
    e = np.exp(-(d * d) / eps)
    gp = (dtype(2) * d / eps) * e
    l0 = -np.expm1(-(d * d) / eps)
    with np.errstate(all="ignore"):
        hp = np.where(l0 > dtype(1e-12), (gp * gp) / (dtype(2) * np.maximum(l0, dtype(1e-30))), (dtype(2) / eps) * e)
    ug = np.zeros((H, 7, B), dtype); uh = np.zeros((H, 7, B), dtype)
    ug[1:] += gp; ug[:-1] -= gp
    uh[1:] += hp; uh[:-1] += hp
    mask = np.zeros(7, dtype); mask[io._rate_rows(g)] = 1
    out = nq, nx, ng, dtype(g.w_rate) * ug * mask[None, :, None], dtype(g.w_rate) * uh * mask[None, :, None]
    assert all(a.dtype == dtype for a in out)
    return out


VX_MAX, W_AL = 58.0, 4.0


def goal_loss(time_row=0, **kw):
    return io.GoalLoss(**dict(dict(w_al=W_AL, vx_max=VX_MAX, time_row=time_row), **kw))


def goal_inputs(Bn, reps, H, seed):
    """Synthetic, fp32-exact inputs of the goal kernels: goal (2, Bn), lam (Bn,), X (H+1, 13, Bc), U (H, 7, Bc), Bc = reps Bn.
    Control differences exactly 0, near sqrt(eps_rate) = 0.1, tiny, and far beyond (rows 0..5); the terminal inequality active on some
    columns, inactive on others, and on columns 1 and 2 (where there are that many) two ulp either side of zero, by
    construction exactly so in float32 and in float64."""
    from aircraft_amd.synthetic import quat_from_euler, quat_rotate

    rng = np.random.default_rng(seed)
    Bc = Bn * reps
    goal = f32_exact(np.stack([rng.uniform(5, 9, Bn), rng.uniform(-4, 4, Bn)]))
    lam = np.where(np.arange(Bn) % 3 == 0, 0.0, np.round(rng.uniform(1, 40, Bn) * 4) / 4)   # s = lam / 8: a multiple of 1/32
    X = np.zeros((H + 1, 13, Bc))
    X[:, 0] = rng.uniform(-20, 20, (H + 1, Bc)); X[:, 1] = rng.uniform(-20, 20, (H + 1, Bc))
    X[:, 2] = -200.0 + rng.uniform(-3, 3, (H + 1, Bc))
    X[H, :2] = np.tile(goal, (1, reps)) + rng.uniform(-5, 5, (2, Bc))
    V = rng.uniform(30, 60, (H + 1, Bc))
    q = quat_from_euler(rng.uniform(-0.3, 0.3, (H + 1) * Bc), rng.uniform(-0.3, 0.3, (H + 1) * Bc), rng.uniform(-0.5, 0.5, (H + 1) * Bc))
    al, be = rng.uniform(-0.15, 0.15, (H + 1) * Bc), rng.uniform(-0.1, 0.1, (H + 1) * Bc)
    vb = V.reshape(-1) * np.stack([np.cos(al) * np.cos(be), np.sin(be), np.sin(al) * np.cos(be)])
    X[:, 3:6] = quat_rotate(q, vb).reshape(3, H + 1, Bc).transpose(1, 0, 2)
    X[:, 6:10] = q.reshape(4, H + 1, Bc).transpose(1, 0, 2)
    X[:, 10:13] = rng.normal(0, 0.1, (H + 1, 3, Bc))
    X[H, 3] = VX_MAX + rng.uniform(-3, 3, Bc)
    X[H, 4:6] = rng.uniform(-4, 4, (2, Bc))
    X = f32_exact(X)
    s = np.tile(lam / (2 * W_AL), reps)
    for o, ulps in ((1, 2), (2, -2)):
        if o < Bc:
            v = np.float32(VX_MAX - s[o])
            for _ in range(abs(ulps)):
                v = np.nextafter(v, np.float32(np.inf if ulps > 0 else -np.inf))
            X[H, 3, o] = float(v)
    U = np.zeros((H, 7, Bc))
    U[0] = rng.normal(0, 0.3, (7, Bc))
    for k in range(1, H):
        kind = rng.integers(0, 5, (7, Bc))
        kind[6] = rng.choice([1, 2, 4], Bc)     # row 6 may carry dt_k: it moves at every node, so that counting it is visible
        d = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                      [0.0, 0.1 * rng.uniform(0.5, 1.5, (7, Bc)), rng.uniform(1, 3, (7, Bc)), 1e-4 * rng.uniform(0.5, 2, (7, Bc))],
                      rng.normal(0, 0.05, (7, Bc))) * rng.choice([-1.0, 1.0], (7, Bc))
        U[k] = f32_exact(f32_exact(U[k - 1]) + d)
        U[k][kind == 0] = f32_exact(U[k - 1])[kind == 0]
    U = f32_exact(U)
    # the side of the inequality is the same in float32 and float64 on every column (else: another seed)
    s32 = np.tile(np.float32(lam) * (np.float32(0.5) / np.float32(W_AL)), reps)
    a32 = np.float32(X[H, 3]) - np.float32(VX_MAX) + s32 > 0
    a64 = X[H, 3] - VX_MAX + s > 0
    assert (a32 == a64).all(), "float32 and float64 disagree on the side of the terminal inequality: re-draw"
    return dict(goal=goal, lam=lam, X=X, U=U, Bn=Bn, reps=reps, H=H, active=a64)


GOAL_MODEL_SHAPES = [(1, 1), (1, 2), (7, 3), (37, 7), (257, 2)]
GOAL_COST_SHAPES = [(1, 1), (5, 3), (86, 7)]      # (Bn, H); candidate batches of 3 Bn columns
GOAL_REPS = 3


@functools.lru_cache(maxsize=None)
def goal_model_case(B, H, time_row, lam_on=True):
    """(B, H) of the model matrix: the leading B columns of a parent batch at least 64 wide, reference and fp32 restatement of
    the parent (read-only)."""
    PB = max(B, PARENT)
    inp = goal_inputs(PB, 1, H, 100 * H + 7 * (time_row > 0) + PB)
    g = goal_loss(time_row)
    lam = inp["lam"] if lam_on else None
    orc = _oracle()
    ref = io.goal_model(orc, g, inp["goal"], inp["X"], inp["U"], lam)
    f32 = goal_model_np(np.float32, g, inp["goal"], inp["X"], inp["U"], lam)
    return dict(inp=inp, g=g, ref=ref, f32=f32, B=B, H=H)


@functools.lru_cache(maxsize=None)
def goal_cost_case(Bn, H, time_row, lam_on=True):
    """(Bn, H) of the cost matrix (3 Bn candidate columns) and a 64-instance batch of the same generator that joins its e32"""
    g = goal_loss(time_row)
    orc = _oracle()
    out = {}
    for key, (bn, reps) in (("case", (Bn, GOAL_REPS)), ("aux", (PARENT, 1))):
        inp = goal_inputs(bn, reps, H, 300 * H + 11 * (time_row > 0) + bn)
        lam = inp["lam"] if lam_on else None
        ref, sabs = io.goal_cost_terms(orc, g, inp["goal"], inp["X"], inp["U"], lam)
        out[key] = dict(inp=inp, ref=ref, sabs=sabs, f32=goal_terms_np(np.float32, g, inp["goal"], inp["X"], inp["U"], lam))
    c, a = out["case"], out["aux"]
    join = lambda k: {t: np.concatenate([c[k][t], a[k][t]]) for t in c[k]}  # noqa: E731
    return dict(inp=c["inp"], g=g, ref=join("ref"), sabs=join("sabs"), f32=join("f32"), Bc=Bn * GOAL_REPS, H=H)


@functools.lru_cache(maxsize=None)
def _aircraft():
    from tests.helpers import make_aircraft

    ac = make_aircraft("poly")
    assert ac.epsilon == EPSILON
    return ac


@functools.lru_cache(maxsize=None)
def _oracle():
    from tests.helpers import make_oracle

    return make_oracle(_aircraft())


# ---- the track, the progress recursion, the node model and the loss in a chosen precision ---------------------------------------
class TrackNP:
    """The device's evaluation of the track (one cubic per segment and axis, Horner; the double count on knots an fp32 progress
    value can hit) in `dtype`.  float32 takes the fp32-rounded cubics the device gets, float64 the unrounded ones."""

    def __init__(self, points, dtype):
        from aircraft_amd.control.track import Track

        tr = Track(points)
        y0, y1 = tr.points[:-1], tr.points[1:]
        m0, m1 = tr.h[:, None] * tr.d[:-1], tr.h[:, None] * tr.d[1:]
        c = np.stack([y0, m0, -3 * y0 - 2 * m0 + 3 * y1 - m1, 2 * y0 + m0 - 2 * y1 + m1], axis=-1)   # (nseg, 3, 4)
        if dtype == np.float32:
            assert np.array_equal(c.astype(np.float32), tr.segment_cubics())
        self.dtype, self.nseg, self.c = dtype, tr.n_segments, c.astype(dtype)
        self.knot = np.array([float(np.float32(s)) == s for s in tr.s_vals])
        self.L = tr.length()
        last = self.c[-1]
        self.end = (last[:, 0] + last[:, 1] + last[:, 2] + last[:, 3]).astype(dtype)

    def eval(self, s):
        dt_ = self.dtype
        s = np.asarray(s, dt_)
        below, above = s < 0, s > 1
        sc = np.clip(s, dt_(0), dt_(1)) * dt_(self.nseg)
        seg = np.minimum(sc.astype(np.int64), self.nseg - 1)
        t = sc - seg.astype(dt_)
        c = self.c[seg]                                       # (n, 3, 4)
        c0, c1, c2, c3 = (c[:, :, i].T for i in range(4))     # (3, n)
        pos = ((c3 * t + c2) * t + c1) * t + c0
        tan = np.where(below | above, dt_(0), ((dt_(3) * c3 * t + dt_(2) * c2) * t + c1) * dt_(self.nseg))
        twice = (t == 0) & (seg > 0) & ~below & self.knot[seg] & (s == seg.astype(dt_) / dt_(self.nseg))
        cl = self.c[np.maximum(seg - 1, 0)]
        l0, l1, l2, l3 = (cl[:, :, i].T for i in range(4))
        pos = pos + np.where(twice, ((l3 + l2) + l1) + l0, dt_(0))
        tan = tan + np.where(twice, ((dt_(3) * l3 + dt_(2) * l2) + l1) * dt_(self.nseg), dt_(0))
        assert pos.dtype == dt_ and tan.dtype == dt_
        return pos, tan

    def terms(self, s, p, v, safe):
        ref, tan = self.eval(s)
        dt_ = self.dtype
        nrm = np.sqrt((tan * tan).sum(axis=0))
        div = np.where(nrm > dt_(1e-3), nrm, dt_(1)) if safe else nrm
        with np.errstate(all="ignore"):
            that = tan / div
        e = p - ref
        il = dt_(1) / dt_(self.L)
        return dict(ref=ref, that=that, s_dot=(v * that).sum(axis=0) * il, delta_s=(e * that).sum(axis=0) * il, err2=(e * e).sum(axis=0))


def progress_np(dtype, T, X, s0, dt, mode, w=None):
    """k_track_progress' outputs in `dtype` throughout: S (H+1, B), s_dot, err2 (H, B), nq, nx, ng (H+1, 13, B)"""
    w = {k: dtype(v) for k, v in dict(to.DEFAULT_WEIGHTS, **(w or {})).items()}
    X = np.asarray(X, dtype); dt = dtype(dt)
    H, B = X.shape[0] - 1, X.shape[2]
    il = dtype(1) / dtype(T.L)
    S = np.zeros((H + 1, B), dtype); sd = np.zeros((H, B), dtype); e2 = np.zeros((H, B), dtype)
    nq = np.zeros((H + 1, 13, B), dtype); nx = np.zeros_like(nq); ng = np.zeros_like(nq)
    S[0] = np.asarray(s0, dtype)

    def slow_of(v):
        speed = np.sqrt((v * v).sum(axis=0))
        return np.where(speed < dtype(0.1), dtype(-2) * w["w_low_velocity"] * (dtype(0.1) - speed) / np.maximum(speed, dtype(1e-6)), dtype(0))

    for k in range(H):
        p, v = X[k, :3], X[k, 3:6]
        t = T.terms(S[k], p, v, mode != 0)
        sd[k], e2[k] = t["s_dot"], t["err2"]
        pred = S[k] + t["s_dot"] * dt + (dtype(0.05) * t["delta_s"] if mode else dtype(0))
        S[k + 1] = np.minimum(np.maximum(pred, dtype(0)), dtype(1))
        tail = np.where(pred < 1, dtype(H - k), dtype(0))
        back = np.where(t["s_dot"] < 0, dtype(2) * w["w_backward"] * t["s_dot"], dtype(0))
        slow = slow_of(v) if k > 0 else np.zeros(B, dtype)
        nq[k, :3] = dtype(2) * w["w_tracking"]
        nx[k, :3] = t["ref"]
        if mode:
            ng[k, :3] = -w["w_progress"] * tail * dtype(0.05) * t["that"] * il
        ng[k, 3:6] = (-w["w_progress_rate"] - w["w_progress"] * tail * dt + back) * t["that"] * il + slow * v
    d = X[H, :3] - T.end[:, None]
    dist = np.maximum(np.sqrt((d * d).sum(axis=0)), dtype(1e-3))
    nq[H, :3] = w["w_terminal_align"] / dist
    nx[H, :3] = T.end[:, None]
    ng[H, 3:6] = slow_of(X[H, 3:6]) * X[H, 3:6]
    assert all(a.dtype == dtype for a in (S, sd, e2, nq, nx, ng))
    return S, sd, e2, nq, nx, ng


def mhtt_terms_np(dtype, T, X, U, S, w=None):
    """to.mhtt_loss_terms' values in `dtype` throughout -> {weight name: (B,)}"""
    w = {k: dtype(v) for k, v in dict(to.DEFAULT_WEIGHTS, **(w or {})).items()}
    X, U, S = (np.asarray(a, dtype) for a in (X, U, S))
    H, B = U.shape[0], U.shape[2]
    z = lambda: np.zeros(B, dtype)  # noqa: E731
    tr, pg, rt, bk, sl, ef = z(), z(), z(), z(), z(), z()
    for k in range(H):
        t = T.terms(S[k], X[k, :3], X[k, 3:6], True)
        tr = tr + t["err2"]; rt = rt + t["s_dot"]
        neg = np.maximum(dtype(0), -t["s_dot"]); bk = bk + neg * neg
        pg = pg + S[k + 1]
        vn = X[k + 1, 3:6]
        lv = np.maximum(dtype(0.1) - np.sqrt((vn * vn).sum(axis=0)), dtype(0)); sl = sl + lv * lv
        if k >= 1:
            ef = ef + (U[k] * U[k]).sum(axis=0, dtype=dtype)
    d = X[H, :3] - T.end[:, None]
    out = {"w_tracking": w["w_tracking"] * tr, "w_progress": -w["w_progress"] * pg, "w_progress_rate": -w["w_progress_rate"] * rt,
           "w_backward": w["w_backward"] * bk, "w_low_velocity": w["w_low_velocity"] * sl,
           "w_terminal_align": w["w_terminal_align"] * np.sqrt((d * d).sum(axis=0)), "w_control": w["w_control"] * ef}
    assert all(v.dtype == dtype for v in out.values())
    return out


# ---- tracks and instances of the progress / model / loss matrix --------------------------------------------------------------------
NSEG = 32     # every knot k / 32 is an fp32 number: a progress value can sit on any of them


def straight_points():
    """33 points 1.1456 m apart on a line, dyadic coordinates: the cubics, track(1) and the knots are exact in fp32"""
    return np.array([-8.0, 4.0, -24.0]) + np.arange(NSEG + 1)[:, None] * np.array([1.0, 0.5, 0.25])


def arc_points(R=64.0, sweep=0.5):
    """an arc of 64 m radius climbing 2 m, coordinates rounded to 1/64 m, with a straight run-out of two segments (the last
    three points collinear and evenly spaced), so that the last segment is a straight line and track(1) is the last point
    exactly in fp32 as in float64 - the terminal distance of an instance a fraction of a millimetre from it is then a
    property of the inputs, not of the track's rounding"""
    th = np.linspace(0, sweep, NSEG + 1)
    P = np.stack([R * np.sin(th), R * (1 - np.cos(th)), -24.0 + 2.0 * th / sweep], axis=1)
    P = np.round(P * 64) / 64
    P[-1] = 2 * P[-2] - P[-3]
    return P


TRACKS = {"straight": straight_points, "arc": arc_points}
TRACK_B = (1, 65, 257)
TRACK_H = (1, 2, 12)
DT = 0.01
KINDS = ("forward", "backward", "slow", "still", "finishing", "clip0", "knot", "outside", "at_end", "turning", "finished", "mixed")
# the order puts one of each kind into the first 12 columns; B = 1 is a backward flier (column 0 is rotated to `backward`)


def _kind_of(B):
    k = (np.arange(B) + 1) % len(KINDS)
    return np.array(KINDS)[k]


@functools.lru_cache(maxsize=None)
def track_case(track, mode, H):
    """One parent batch (B = 257) per track, recursion mode and horizon: inputs, float64 references (unit structure: the
    default weights; every output is linear in them), fp32 restatements, the branch inventory.  Smaller batches are its
    leading columns.  Read-only."""
    B = max(TRACK_B)
    P = TRACKS[track]()
    tro = to.TrackOracle(P)
    T64, T32 = TrackNP(P, np.float64), TrackNP(P, np.float32)
    L = T64.L
    rng = np.random.default_rng(1000 * list(TRACKS).index(track) + 100 * mode + H)
    kind = _kind_of(B)
    s0 = rng.uniform(0.1, 0.6, B)
    sign = np.ones((H + 1, B)); speed = rng.uniform(20, 60, (H + 1, B))
    is_ = lambda *names: np.isin(kind, names)  # noqa: E731
    sign[:, is_("backward", "clip0")] = -1.0
    sign[1:, is_("turning")] = -1.0
    mixed = is_("mixed")
    sign[:, mixed] = rng.choice([-1.0, 1.0], (H + 1, int(mixed.sum())))
    speed[:, is_("slow")] = rng.uniform(0.005, 0.06, (H + 1, int(is_("slow").sum())))
    speed[:, is_("still")] = 0.0
    slow_nodes = mixed[None, :] & (rng.uniform(0, 1, (H + 1, B)) < 0.4)
    speed[slow_nodes] = np.where(rng.uniform(0, 1, int(slow_nodes.sum())) < 0.3, 0.0, rng.uniform(0.005, 0.06, int(slow_nodes.sum())))
    s0[is_("finishing")] = np.where(np.arange(int(is_("finishing").sum())) % 2 == 0, 0.97, 0.996)
    speed[:, is_("finishing", "finished")] = rng.uniform(50, 60, (H + 1, int(is_("finishing", "finished").sum())))
    s0[is_("finished")] = 1.0
    s0[is_("clip0")] = rng.uniform(0.001, 0.01, int(is_("clip0").sum()))
    s0[is_("knot")] = rng.integers(1, NSEG, int(is_("knot").sum())) / NSEG
    out = is_("outside")
    if mode:      # the initial guess divides by the plain norm: outside [0, 1] it is 0 / 0 in the reference too
        s0[out] = np.where(np.arange(int(out.sum())) % 2 == 0, -0.2, 1.3)
    s0 = f32_exact(s0)
    # velocities within 0.35 rad of the chord (the tangent turns by at most 0.5 rad): |cos| >= 0.7 with any tangent, so that
    # s_dot carries no cancellation; positions 15 .. 40 m off the track, so that the tracking error carries none
    chord = P[-1] - P[0]; chord = chord / np.linalg.norm(chord)
    a = np.cross(chord, [0, 0, 1.0]); a = a / np.linalg.norm(a)
    b = np.cross(chord, a)
    ang, phi = rng.uniform(0, 0.35, (H + 1, B)), rng.uniform(0, 2 * np.pi, (H + 1, B))
    dirv = (np.cos(ang)[:, None] * chord[None, :, None] + np.sin(ang)[:, None] * (np.cos(phi)[:, None] * a[None, :, None] + np.sin(phi)[:, None] * b[None, :, None]))
    X = np.zeros((H + 1, 13, B))
    X[:, 3:6] = (sign * speed)[:, None] * dirv
    sg = np.clip(s0[None, :] + np.arange(H + 1)[:, None] * 0.02 * sign, 0, 1)
    off = rng.normal(0, 1, (H + 1, 3, B)); off = off / np.linalg.norm(off, axis=1, keepdims=True) * rng.uniform(15, 40, (H + 1, 1, B))
    X[:, :3] = T64.eval(0.0003 + 0.999 * sg.reshape(-1))[0].reshape(3, H + 1, B).transpose(1, 0, 2) + off   # (no guess on a knot)
    end = tro.eval(1.0)
    ae = is_("at_end")
    near = rng.normal(0, 1, (3, int(ae.sum()))); near = near / np.linalg.norm(near, axis=0) * rng.uniform(2e-4, 8e-4, int(ae.sum()))
    X[H][:3, ae] = end[:, None] + near
    X[:, 9] = 1.0
    X[:, 6:10] += rng.normal(0, 0.1, (H + 1, 4, B)); X[:, 10:13] = rng.normal(0, 0.1, (H + 1, 3, B))   # rows the kernels must ignore
    X = f32_exact(X)
    U = f32_exact(rng.normal(0, 0.3, (H, 7, B)))
    # float64 references
    nq, nx, ng, det = to.mhtt_model(tro, L, X, s0, DT, mode, detail=True)
    if mode == 0:
        S = to.progress_initial(tro, L, X, s0, DT); sd, e2 = det["s_dot"], det["err2"]
    else:
        S, sd, e2 = to.progress_tight(tro, L, X, s0, DT)
    assert np.array_equal(S, det["S"])
    Sin = f32_exact(S)                                   # the loss kernels read a given progress sequence
    terms, sabs = to.mhtt_loss_terms(tro, L, X, U, Sin)
    f32 = progress_np(np.float32, T32, X, s0, DT, mode)
    f32_terms = mhtt_terms_np(np.float32, T32, X, U, Sin)
    # scale of s_dot per instance: sum_a |v_a t^_a| / L, the summands of the projection
    sd_scale = (np.abs(X[:H, 3:6] * det["that"]).sum(axis=1) / L).max(axis=0)
    case = dict(track=track, mode=mode, H=H, B=B, points=P, L=L, kind=kind, X=X, U=U, s0=s0, Sin=Sin, S=S, s_dot=sd, err2=e2,
                model=(nq, nx, ng), detail=det, terms=terms, sabs=sabs, f32=f32, f32_terms=f32_terms, sd_scale=sd_scale)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def progress_e32(case):
    """{S, s_dot, err2}: worst per-instance error of the fp32 restatement (S in absolute terms: progress lives on [0, 1])"""
    S, sd, e2 = case["f32"][:3]
    out = {"S": float(inst_err(S, case["S"], scale=1.0).max()), "s_dot": float(inst_err(sd, case["s_dot"], scale=case["sd_scale"]).max())}
    out["err2"] = float(inst_err(e2, case["err2"]).max())
    return out


def branches(case):
    """{branch: (instances at k = 0, instances at some k > 0)} on the float64 reference of a parent case"""
    d, H = case["detail"], case["H"]
    sp = d["speed"]
    s0 = case["s0"]
    knots = np.arange(1, NSEG) / NSEG

    def split(m):   # m (H, B) over nodes 0 .. H-1
        return int(m[0].sum()), int(m[1:].any(axis=0).sum())

    return {
        "s_dot<0": split(d["s_dot"] < 0),
        "speed<0.1": split(sp[:H] < 0.1),
        "speed==0": split(sp[:H] == 0),
        "speed<0.1@H": (int((sp[H] < 0.1).sum()),) * 2,
        "pred>=1": split(d["pred"] >= 1),
        "pred<0": split(d["pred"] < 0),
        "S==1 held": split((d["S"][:H] == 1) & (d["S"][1:] == 1)),
        "s0 on knot": (int(np.isin(s0, knots).sum()),) * 2,
        "s0 outside": (int(((s0 < 0) | (s0 > 1)).sum()),) * 2,
        "dist<1e-3": (int((d["dist"] < 1e-3).sum()),) * 2,
        "dist>1": (int((d["dist"] > 1).sum()),) * 2,
    }


def weights_one_hot():
    """[(label, weights dict)]: each MHTT weight alone at its default, then all of them"""
    out = [(n, {k: (v if k == n else 0.0) for k, v in to.DEFAULT_WEIGHTS.items()}) for n in to.TERMS]
    return out + [("all", dict(to.DEFAULT_WEIGHTS))]


# ---- the track itself: per-point evaluation ---------------------------------------------------------------------------------------------
TRACK_EVAL_N = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def track_eval_case(track):
    """257 progress values (the cases are its leading n): interior knots, both ends, outside [0, 1], random interior values;
    point 0 is an interior knot.  Position error per point relative to max(|pos|, 1 m), tangent relative to the largest
    tangent of the case (tangents of one track have one scale)."""
    P = TRACKS[track]()
    tro = to.TrackOracle(P)
    rng = np.random.default_rng(77)
    s = f32_exact(np.concatenate([[0.5, 0.0, 1.0, -0.3, 1.5, 0.25, 31 / 32, 1 / 32], rng.uniform(0, 1, 249)]))
    pos = np.stack([tro.eval(float(v)) for v in s], axis=1); tan = np.stack([tro.eval_tangent(float(v)) for v in s], axis=1)
    p32, t32 = TrackNP(P, np.float32).eval(s)
    return dict(points=P, s=s, pos=pos, tan=tan, f32=(p32, t32))


def track_point_err(pos, tan, case, n=None):
    """-> (per-point position error, per-point tangent error) of the leading n points"""
    n = pos.shape[1] if n is None else n
    rp, rt = case["pos"][:, :n], case["tan"][:, :n]
    ep = np.abs(np.asarray(pos, np.float64)[:, :n] - rp).max(axis=0) / np.maximum(np.abs(rp).max(axis=0), 1.0)
    et = np.abs(np.asarray(tan, np.float64)[:, :n] - rt).max(axis=0) / np.abs(case["tan"]).max()
    return ep, et


# ---- the quadratic cost kernels, term by term ----------------------------------------------------------------------------------------------
def quad_terms_np(dtype, c, X, U, node=None):
    """io.cost term by term in `dtype`: ({term: (B,)}, {term: S_abs}); terms q, qf, r, u_lin, or with node = (nq, nx, ng)
    (columns b % Bn) node_q, node_glin, r, u_lin"""
    t = lambda a: np.asarray(a, dtype)  # noqa: E731
    X, U = t(X), t(U)
    half = dtype(0.5)
    s = lambda a: a.sum(axis=(0, 1), dtype=dtype)  # noqa: E731
    out = {}
    if node is None:
        dx = X[:-1] - t(c.x_ref)[None, :, None]; dg = X[-1:] - t(c.x_goal)[None, :, None]
        out["q"] = half * t(c.q)[None, :, None] * dx * dx
        out["qf"] = half * t(c.qf)[None, :, None] * dg * dg
    else:
        nq, nx, ng = (np.tile(t(a), (1, 1, X.shape[2] // a.shape[2])) for a in node)
        d = X - nx
        out["node_q"] = half * nq * d * d
        out["node_glin"] = ng * X
    out["r"] = half * t(c.r)[None, :, None] * U * U
    out["u_lin"] = t(io._u_lin(c))[None, :, None] * U
    return {k: s(v) for k, v in out.items()}, {k: s(np.abs(v)) for k, v in out.items()}


QUAD_B = (1, 65)
QUAD_H = 5
QUAD_NA = 3


@functools.lru_cache(maxsize=None)
def quad_case(wide):
    """Inputs of the quadratic cost kernels at the parent width 65 (B = 1 is column 0; a line-search-wide batch has
    3 x B columns, column a B + b reading node column b)"""
    from aircraft_amd.control import QuadraticCost

    B, H = max(QUAD_B), QUAD_H
    rng = np.random.default_rng(41 + int(wide))
    n = lambda *s: rng.normal(size=s)  # noqa: E731
    f = lambda a: [float(v) for v in f32_exact(a)]  # noqa: E731
    cost = QuadraticCost(q=f(rng.uniform(0.2, 2, 13)), qf=f(rng.uniform(0.5, 3, 13)), r=f(rng.uniform(0.3, 1, 7)),
                         x_ref=f(n(13)), x_goal=f(n(13)), reg=0.25, u_lin=f(0.3 * n(7)))
    node = (f32_exact(rng.uniform(0.2, 2, (H + 1, 13, B))), f32_exact(n(H + 1, 13, B)), f32_exact(0.5 * n(H + 1, 13, B)))
    na = QUAD_NA if wide else 1
    return dict(cost=cost, node=node, X=f32_exact(n(H + 1, 13, na, B)), U=f32_exact(n(H, 7, na, B)), na=na)


def quad_columns(case, B):
    """the B leading instances of a quad_case: X (H+1, 13, na B), U, node arrays (.., B)"""
    H, na = QUAD_H, case["na"]
    X = np.ascontiguousarray(case["X"][..., :B]).reshape(H + 1, 13, na * B)
    U = np.ascontiguousarray(case["U"][..., :B]).reshape(H, 7, na * B)
    return X, U, tuple(np.ascontiguousarray(a[..., :B]) for a in case["node"])
