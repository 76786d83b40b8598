"""CPU side of the step-by-step trim tests (tests/test_gpu_trim_steps.py): the layout that tests/trim_ref.py restates against
aircraft_amd/csrc/ac_trim.hpp and ac_trim_f32, `chain` / `step` / `lm` against the versions they were split out of, the e32
condition of every case the device is held to (the g++ build of ac_trim.hpp, tests/host_trim/trim_host.cpp, against float64 on
identical inputs), the decisiveness of every status decision, the transitions the chain goes through, and the same
evaluation / step / chain checks the device gets, run on the host build for the analytic models."""
import os
import re

import numpy as np
import pytest

from tests import riccati_ref as rr
from tests import trim_ref as T
from tests.helpers import ROOT, parity_report

CSRC = os.path.join(ROOT, "aircraft_amd", "csrc")

# (model, lateral mode) of each part of tests/test_gpu_trim_steps.py
EVAL_CASES = [(m, 0) for m in ("default", "linear", "net_3x64_valu", "net_4x128", "poly", "real_net")] + \
             [(m, 1) for m in ("poly", "linear", "real_net")]
STEP_CASES = [("poly", 0), ("poly", 1), ("default", 0), ("linear", 0), ("linear", 1), ("real_net", 0), ("real_net", 1)]
STEP_CASES_POINT0 = [("net_4x128", 0), ("net_3x64_valu", 0)]   # the synthetic nets: the first step only
CHAIN_CASES = [("poly", 0), ("poly", 1), ("default", 0), ("linear", 0), ("linear", 1), ("real_net", 0)]
HOST_CASES = [c for c in CHAIN_CASES if c[0] != "real_net"]    # the host build has the analytic models


def step_points(name):
    return (0,) if (name, 0) in STEP_CASES_POINT0 else T.POINTS


def ids(cases):
    return [f"{m}-{lat}" for m, lat in cases]


# ---- 1. the restated layout ------------------------------------------------------------------------------------------------------
def test_layout_matches_the_header():
    h = open(os.path.join(CSRC, "ac_trim.hpp")).read()

    def const(name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", h)
        assert m, name
        return m.group(1).strip()

    assert int(const("kTrimStateWords")) == T.STATE_WORDS == dict(T.WS_ROWS)["St"]
    assert const("kTrimWsFloats").replace(" ", "") == "13+7+13+169+91+kTrimStateWords"
    assert [r for _, r in T.WS_ROWS] == [13, 7, 13, 169, 91, 57] and sum(r for _, r in T.WS_ROWS) == T.WS_FLOATS
    got = {k: int(const(c)) for k, c in dict(zc="kTzc", zb="kTzb", rb="kTrb", Jb="kTJb", lam="kTlam", cost="kTcost", flag="kTflag").items()}
    assert got == T.WORDS
    assert const("kTrimActive") == "-1.0f" and T.ACTIVE == -1.0
    assert int(const("kTrimBlock")) == T.BLOCK and T.BLOCK < max(T.SIZES)
    m = re.search(r"kTrimLambda0\s*=\s*([\w.+-]+)f,\s*kTrimLambdaMin\s*=\s*([\w.+-]+)f,\s*kTrimLambdaMax\s*=\s*([\w.+-]+)f", h)
    assert m and tuple(float(v) for v in m.groups()) == (T.LAM0, T.LAM_MIN, T.LAM_MAX)
    assert [int(const(c)) for c in ("AC_TRIM_CONVERGED", "AC_TRIM_MAXITER", "AC_TRIM_BOUND", "AC_TRIM_NONFINITE")] == [0, 1, 2, 3]
    assert "lam * (1.0f / 3.0f)" in h and "lam * 4.0f" in h
    # the carving in ac_trim_f32
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("ac_abi.hpp", "abi_flight.hip"))  # (align256: ac_abi.hpp)
    assert re.search(r"kTrimWsPad\s*=\s*6\s*\*\s*64;", src) and T.WS_PAD == 6 * 64
    assert "(((uintptr_t)p + 255) & ~(uintptr_t)255)" in src
    carve = re.findall(r"float\* (\w+) = align256\(([^;]*)\);", src)
    assert carve == [("Xw", "ws"), ("Uw", "Xw + 13 * N"), ("Xd", "Uw + 7 * N"), ("Fx", "Xd + 13 * N"), ("Fu", "Fx + 169 * N"),
                     ("St", "Fu + 91 * N")]


@pytest.mark.parametrize("n", T.SIZES + (128,))
def test_layout_fits_the_workspace_at_every_alignment(n):
    for mis in range(0, 256, 4):
        off, end = T.ws_layout(4096 + mis, n)
        assert end <= n * T.WS_FLOATS + T.WS_PAD
        assert all((4096 + mis + 4 * o) % 256 == 0 for o in off.values())
        names = [k for k, _ in T.WS_ROWS]
        for a, b in zip(names, names[1:]):
            assert 0 <= off[b] - (off[a] + dict(T.WS_ROWS)[a] * n) < 64   # no overlap, less than one boundary of padding
    off, _ = T.ws_layout(4096 + 12, n)
    assert off["X"] == 61   # 3 floats past a boundary: 61 floats of padding in front


# ---- 2. chain, step and lm against the versions they were split out of --------------------------------------------------------------
def _jacobian_before(orc, z, target, uhold, lateral, h=1e-6):
    """trim_ref.jacobian as it was before `chain` was split out of it, kept verbatim"""
    n = z.shape[1]
    x, u = T.assemble(z, target, uhold, lateral)
    f, Fx, Fu = orc.state_derivative_sens(x, u)
    q = T.kinematics(z, target, lateral)[0]
    r = T.transform(z, target, lateral, f[3:6], f[10:13])
    J = np.zeros((6, 6, n))
    for j in range(6):
        e = np.zeros((6, 1))
        e[j] = h
        xp, up = T.assemble(z + e, target, uhold, lateral)
        xm, um = T.assemble(z - e, target, uhold, lateral)
        dx, du = (xp - xm) / (2 * h), (up - um) / (2 * h)
        df = np.einsum("icn,cn->in", Fx, dx) + np.einsum("icn,cn->in", Fu, du)
        rp = T.transform(z + e, target, lateral, f[3:6], f[10:13])
        rm = T.transform(z - e, target, lateral, f[3:6], f[10:13])
        dT = (rp - rm) / (2 * h)
        lin = np.concatenate([T.rot(T.qconj(q), df[3:6]), df[10:13]])
        J[:, j] = dT + lin
    return r, J


def _lm_before(orc, z0, target, uhold, lateral, lo, hi, tol=(1e-4, 1e-4), iters=200):
    """trim_ref.lm as it was before `step` was split out of it, kept verbatim (on `_jacobian_before`)"""
    lo, hi = np.asarray(lo)[:, None], np.asarray(hi)[:, None]
    w = np.array([1 / tol[0]] * 3 + [1 / tol[1]] * 3)[:, None]
    n = z0.shape[1]
    zc = np.clip(z0, lo, hi)
    zb, rb, Jb = zc.copy(), np.full((6, n), np.nan), np.zeros((6, 6, n))
    cost_b = np.full(n, np.inf)
    lam = np.full(n, T.LAM0)
    active = np.ones(n, bool)
    conv = np.zeros(n, bool)
    for _ in range(iters):
        idx = np.where(active)[0]
        if not len(idx):
            break
        r, J = _jacobian_before(orc, zc[:, idx], target[:, idx], uhold[:, idx], lateral)
        cost = ((w * r) ** 2).sum(0)
        better = cost < cost_b[idx]
        a, b = idx[better], idx[~better]
        zb[:, a], rb[:, a], Jb[:, :, a], cost_b[a] = zc[:, a], r[:, better], J[:, :, better], cost[better]
        lam[a] = np.maximum(lam[a] / 3, T.LAM_MIN)
        lam[b] = np.minimum(lam[b] * 4, T.LAM_MAX)
        ok = (np.abs(rb[:3]) <= tol[0]).all(0) & (np.abs(rb[3:]) <= tol[1]).all(0)
        conv |= ok & active
        active &= ~ok & np.isfinite(cost_b)
        for i in np.where(active)[0]:
            Jw = w * Jb[:, :, i]
            H = Jw.T @ Jw
            g = Jw.T @ (w[:, 0] * rb[:, i])
            M = H + lam[i] * np.diag(np.diag(H)) + (1e-7 * np.diag(H).max() + 1e-30) * np.eye(6)
            zc[:, i] = np.clip(zb[:, i] + np.linalg.solve(M, -g), lo[:, 0], hi[:, 0])
    return zb, rb, conv


@pytest.mark.parametrize("lateral", [0, 1])
@pytest.mark.parametrize("model", ["default", "linear", "poly", "real_net"])
def test_chain_fed_with_the_oracle_is_the_old_jacobian(model, lateral):
    from tests.test_host_trim import synthetic_problem

    c = T.case(model, 0)
    tg, uh, z = synthetic_problem(96, lateral, seed=2)
    r0, J0 = _jacobian_before(c.orc, z, tg, uh, lateral)
    r1, J1 = T.jacobian(c.orc, z, tg, uh, lateral)
    assert np.array_equal(r0, r1) and np.array_equal(J0, J1)
    x, u = T.assemble(z, tg, uh, lateral)
    r2, J2 = T.chain(z, tg, lateral, *c.orc.state_derivative_sens(x, u))
    assert np.array_equal(r0, r2) and np.array_equal(J0, J2)


@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_lm_results_unchanged_on_the_host_trim_grid(model):
    c = T.case(model, 0)
    g = T.grid(seed=3)
    for lateral in (0, 1):
        cases = [k for k in g if (k[1] == 0.0 or (model == "linear") == (lateral == 1))] if lateral == 0 else \
            [k for k in g if model == "linear" and k[1] != 0.0]
        if not cases:
            continue
        n = len(cases)
        tg, uh = np.zeros((7, n)), np.zeros((7, n))
        for i, (V, psid, beta, fl, psi) in enumerate(cases):
            tg[:, i] = [0.0, 0.0, -200.0, V, psi, psid, 0.0 if lateral else beta]
            uh[6, i] = fl
        tg, uh = T.f32x(tg), T.f32x(uh)
        z0 = T.default_guess(tg[3], tg[5], c.ac.opts.aircraft_config.glide_ratio)
        lo, hi = c.ac.trim_bounds(lateral)
        for iters in (7, 40):
            a = _lm_before(c.orc, z0, tg, uh, lateral, lo, hi, iters=iters)
            b = T.lm(c.orc, z0, tg, uh, lateral, lo, hi, iters=iters)
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def test_step_leaves_z_on_a_non_finite_step_and_clips():
    lo, hi = -np.ones(6), np.ones(6)
    z = np.full((6, 3), 0.5)
    J = np.stack([np.eye(6)] * 3, axis=2)
    r = np.full((6, 3), 1.0)
    r[2, 1] = np.nan
    r[:, 2] = -3.0
    zn, free = T.step(z, r, J, np.full(3, 1e-3), lo, hi, tol=(1.0, 1.0), raw=True)
    assert np.allclose(zn[:, 0], 0.5 - 1 / (1 + 1e-3 + 1e-7)) and np.array_equal(zn[:, 1], z[:, 1])
    assert np.array_equal(zn[:, 2], hi) and (free[:, 2] > 3).all()
    got = T.host_step(z, r, J, np.full(3, 1e-3), 0, lo, hi, (1.0, 1.0))
    assert np.abs(got[:, 0] - zn[:, 0]).max() < 1e-6 and np.array_equal(got[:, 1:], zn[:, 1:])


def test_transition_rules():
    f = np.float32
    prev = dict(lam=np.array([1e-3, 1e-3, 2e-8, 5e7, 1e-3, 1e-3], f), cost=np.array([2, 2, 2, 2, np.inf, 2], f),
                flag=np.array([-1, -1, -1, -1, -1, 0], f))
    kind, lam, nonfinite = T.transition(prev, np.array([1, 2, 1, 3, np.nan, 1], f))
    assert list(kind) == ["accept", "reject", "accept", "reject", "reject", "frozen"]
    third = f(1) / f(3)
    assert T.same_bits(lam, np.array([f(1e-3) * third, f(1e-3) * f(4), f(1e-8), f(1e8), f(1e-3) * f(4), f(1e-3)], f))
    assert list(nonfinite) == [False, False, False, False, True, False]


# ---- 3. the e32 condition of every case the device is held to ------------------------------------------------------------------------
@pytest.mark.parametrize("model,lateral", EVAL_CASES, ids=ids(EVAL_CASES))
def test_e32_of_the_chain(model, lateral):
    er, eJ = T.case(model, lateral).e32_chain()
    parity_report("trim_steps_e32_chain", model=model, lateral=lateral, e32_r=er, e32_J=eJ)
    print(f"[trim steps] e32 chain {model} {lateral}: r {er:.2e} J {eJ:.2e}")
    assert 0 < er <= rr.E32_MAX and 0 < eJ <= rr.E32_MAX


@pytest.mark.parametrize("model,lateral", STEP_CASES + STEP_CASES_POINT0, ids=ids(STEP_CASES + STEP_CASES_POINT0))
def test_e32_of_the_step_from_every_point(model, lateral):
    c = T.case(model, lateral)
    e = {k: c.e32_step_point(k) for k in step_points(model)}
    parity_report("trim_steps_e32_step", model=model, lateral=lateral, **{f"point{k}": v for k, v in e.items()})
    print(f"[trim steps] e32 step {model} {lateral}: " + " ".join(f"{k}: {v:.2e}" for k, v in e.items()))
    assert all(0 < v <= rr.E32_MAX for v in e.values()), e


@pytest.mark.parametrize("model,lateral", CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_e32_of_the_steps_along_the_chain(model, lateral):
    e = T.case(model, lateral).e32_step_chain()
    parity_report("trim_steps_e32_step_chain", model=model, lateral=lateral, e32=e)
    print(f"[trim steps] e32 steps along the chain {model} {lateral}: {e:.2e}")
    assert 0 < e <= rr.E32_MAX


# ---- 4. status decisions are decisive, and the chain goes through every transition -----------------------------------------------
@pytest.mark.parametrize("model,lateral", EVAL_CASES, ids=ids(EVAL_CASES))
def test_status_decisions_are_decisive(model, lateral):
    """min |g_j| / sum_i |J_ij w_i^2 r_i| over the on-bound components of every instance whose status the device decides:
    after one evaluation at every starting point, and after K evaluations of the chain"""
    c = T.case(model, lateral)
    worst = np.inf
    for k in T.POINTS:
        r, J = T.jacobian(c.orc, c.points[k], c.tg, c.uh, lateral)
        fs, dec = T.final_status(c.points[k], r, J, c.lo, c.hi, c.tol)
        worst = min(worst, dec[~T.converged(r, c.tol)].min(initial=np.inf))
        assert np.array_equal(T.host_final_status(c.points[k], r, J, lateral, c.lo, c.hi, c.tol), fs)
    if (model, lateral) in CHAIN_CASES:
        s = c.traj[T.K - 1]
        a = s["active"]
        fs, dec = T.final_status(s["zb"][:, a], s["rb"][:, a], s["Jb"][:, :, a], c.lo, c.hi, c.tol)
        worst = min(worst, dec.min(initial=np.inf))
        assert np.array_equal(T.host_final_status(s["zb"][:, a], s["rb"][:, a], s["Jb"][:, :, a], lateral, c.lo, c.hi, c.tol), fs)
    print(f"[trim steps] decisiveness {model} {lateral}: {worst:.2e}")
    assert worst >= 1e-4


@pytest.mark.parametrize("model,lateral", CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_chain_shows_every_transition(model, lateral):
    c = T.case(model, lateral)
    traj = c.traj[:T.K]
    acc = sum(int((s["kind"] == "accept").sum()) for s in traj)
    rej = sum(int((s["kind"] == "reject").sum()) for s in traj)
    last = traj[-1]
    a = last["active"]
    fs, _ = T.final_status(last["zb"][:, a], last["rb"][:, a], last["Jb"][:, :, a], c.lo, c.hi, c.tol)
    freeze = int(last["conv"].sum())
    print(f"[trim steps] {model} {lateral}: {acc} accepts, {rej} rejects, {freeze} freezes, status 1 x {(fs == 1).sum()}, 2 x {(fs == 2).sum()}")
    assert acc >= 1 and rej >= 1 and freeze >= 1
    assert any(not s["active"].all() and s["active"].any() for s in traj[:-1]), "a frozen instance next to active ones"
    if model == "poly" and lateral == 0:
        assert (freeze, int((fs == 1).sum()), int((fs == 2).sum())) == (42, 4, 2)
    if model != "linear":   # the linear model leaves no instance out of iterations within K: it converges or stops on a bound
        assert (fs == 1).any()
    assert (fs == 2).any()


def test_every_status_is_seen_along_the_chains():
    seen = set()
    for model, lateral in CHAIN_CASES:
        c = T.case(model, lateral)
        last = c.traj[T.K - 1]
        a = last["active"]
        seen |= set(T.final_status(last["zb"][:, a], last["rb"][:, a], last["Jb"][:, :, a], c.lo, c.hi, c.tol)[0].tolist())
        seen |= {0} if last["conv"].any() else set()
    assert seen == {0, 1, 2}


# ---- 5. the device's checks on the host build (analytic models) ------------------------------------------------------------------------
def initial_snapshot(z0, lo, hi):
    """the state trim_init_unit leaves (usable inputs)"""
    n = z0.shape[1]
    st = np.full((T.STATE_WORDS, n), np.nan, np.float32)
    z = np.clip(T.c32(z0), T.c32(lo)[:, None], T.c32(hi)[:, None])
    st[0:6], st[6:12] = z, z
    st[T.WORDS["lam"]], st[T.WORDS["cost"]], st[T.WORDS["flag"]] = T.LAM0, np.inf, T.ACTIVE
    return dict(st=st, S=np.full(n, 1, np.int32), Z=z, R=st[12:18])


@pytest.mark.parametrize("model,lateral", HOST_CASES, ids=ids(HOST_CASES))
def test_host_build_one_evaluation_and_one_step(model, lateral):
    c = T.case(model, lateral)
    er, eJ = c.e32_chain()
    tg, uh, z0, pt = c.pool()
    bar = rr.FACTOR * np.array([c.e32_step_point(k) for k in pt])
    one = T.host_trace(c.ac, tg, uh, z0, lateral, 1, c.lo, c.hi, c.tol)
    fig = T.check_evaluation(one, tg, uh, z0, lateral, c.lo, c.hi, c.tol, rr.FACTOR * er, rr.FACTOR * eJ)
    two = T.host_trace(c.ac, tg, uh, z0, lateral, 2, c.lo, c.hi, c.tol)
    worst, clipped = T.check_step(one, two, c.lo, c.hi, c.tol, bar)
    print(f"[trim steps] host {model} {lateral}: r {fig['r']:.2e} / {fig['bar_r']:.2e}, J {fig['J']:.2e} / {fig['bar_J']:.2e}, "
          f"cost {fig['cost_ulp']:.2f} ulp, step {worst:.2e} / {bar.max():.2e}, {clipped} clipped components")
    assert clipped > 0 and fig["status2"] > 0


@pytest.mark.parametrize("model,lateral", HOST_CASES, ids=ids(HOST_CASES))
def test_host_build_chain(model, lateral):
    c = T.case(model, lateral)
    bar_r, bar_z = rr.FACTOR * c.e32_chain()[0], rr.FACTOR * c.e32_step_chain()
    snaps = [initial_snapshot(c.z0, c.lo, c.hi)] + [T.host_trace(c.ac, c.tg, c.uh, c.z0, lateral, k, c.lo, c.hi, c.tol)
                                                    for k in range(1, T.K + 1)]
    total = dict(accept=0, reject=0, freeze=0, undecided=0)
    worst = 0.0
    for k in range(T.K):
        cnt = T.check_transition(snaps[k], snaps[k + 1], c.tg, lateral, c.tol, bar_r)
        total = {key: total[key] + cnt[key] for key in total}
        if k:
            worst = max(worst, T.check_step(snaps[k], snaps[k + 1], c.lo, c.hi, c.tol, bar_z)[0])
    s1, s2, dec = T.check_last_status(snaps[-1], c.lo, c.hi, c.tol)
    print(f"[trim steps] host chain {model} {lateral}: {total}, step {worst:.2e} / {bar_z:.2e}, status 1 x {s1}, 2 x {s2}")
    assert total["accept"] and total["reject"] and total["freeze"] and total["undecided"] == 0
    assert len({float(v) for s in snaps[1:] for v in T.unpack(s["st"])["lam"]}) >= 4, "several values of lambda"
