"""The float64 restatement of the loop closed through the estimator (tests/lqg_ref.py) against first principles, on the CPU:
the counter layout against Philox's known answers, the independence of a draw from the batch, the moments of the noise, the
schedule, the float32 fmaf emulation against exact rational arithmetic, the score against a direct inverse, and the consistency
of the closed loop (NEES and NIS of a Monte-Carlo run against their chi-square means)."""
from fractions import Fraction

import numpy as np

from tests import ekf_ref as E
from tests import lqg_ref as R
from tests import lqr_ref as L
from tests import mppi_ref as M


def test_counter_layout_matches_the_known_answers():
    """key = (seed low, seed high), counter = (g low, g high, step, purpose): the third known answer of mppi_ref through words()"""
    ctr, key, out = M.KNOWN_ANSWERS[2]
    s = R.Sensors(seed=(key[1] << 32) | key[0], instance_offset=((ctr[1] << 32) | ctr[0]) - 3)
    w = R.words(s, 5, ctr[2], ctr[3])
    assert tuple(int(v[3]) for v in w) == out
    for ctr, key, out in M.KNOWN_ANSWERS[:2]:
        s = R.Sensors(seed=(key[1] << 32) | key[0], instance_offset=(ctr[1] << 32) | ctr[0])
        assert tuple(int(v[0]) for v in R.words(s, 1, ctr[2], ctr[3])) == out


def test_a_draw_depends_on_seed_step_instance_and_row_only():
    x = E.cycle(E.inputs("poly")["x"], 17)
    s = R.Sensors(seed=99, period=(5, 5, 1, 1, 1), phase=(2, 2, 0, 0, 0), dropout=(0, 0, 0, 0.3, 0))
    Z, mask, _, _ = R.sense(x, E.SIG_R, s, 12)
    for i in (0, 6, 16):  # the instance alone, at its own offset
        si = R.Sensors(seed=99, instance_offset=i, period=s.period, phase=s.phase, dropout=s.dropout)
        Zi, mi, _, _ = R.sense(x[:, i:i + 1], E.SIG_R, si, 12)
        assert np.array_equal(Zi[:, 0], Z[:, i], equal_nan=True) and mi[0] == mask[i]
        assert np.array_equal(R.disturb(x[:, i:i + 1], E.SIG_Q, si, 3)[0][:, 0], R.disturb(x, E.SIG_Q, s, 3)[0][:, i])
    # another step, another seed, the process noise: other draws
    assert not np.array_equal(R.sense(x, E.SIG_R, s, 17)[0], Z, equal_nan=True)
    assert not np.array_equal(R.sense(x, E.SIG_R, R.Sensors(seed=98, period=s.period, phase=s.phase, dropout=s.dropout), 12)[0], Z, equal_nan=True)
    assert not np.array_equal(R.normals(s, 17, 12, R.MEAS, 3)[0], R.normals(s, 17, 12, R.PROC, 3)[0])


def test_noise_moments_and_dropout_rate():
    n = 20000
    s = R.Sensors(seed=5, dropout=(0.0, 0.1, 0.3, 0.5, 0.9))
    nrm = np.concatenate([R.normals(s, n, 4, R.MEAS, 4)[0][:15], R.normals(s, n, 4, R.PROC, 3)[0]])
    # 27 rows of n standard normals: mean within 5 / sqrt(n), variance within 5 sqrt(2 / n), rows uncorrelated within 5 / sqrt(n)
    assert np.abs(nrm.mean(axis=1)).max() <= 5 / np.sqrt(n) and np.abs(nrm.var(axis=1) - 1).max() <= 5 * np.sqrt(2 / n)
    c = np.corrcoef(nrm) - np.eye(27)
    assert np.abs(c).max() <= 5 / np.sqrt(n)
    mask = R.report_mask(s, n, 4)
    for j, p in enumerate(s.dropout):
        rate = 1 - (((mask >> (3 * j)) & 7) == 7).mean()
        assert abs(rate - p) <= 5 * np.sqrt(max(p * (1 - p), 1e-12) / n), (j, rate)
        assert set(np.unique((mask >> (3 * j)) & 7)) <= {0, 7}


def test_fmaf_emulation_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a, b = (rng.standard_normal(2000).astype(np.float32) for _ in range(2))
    c = (-(a.astype(np.float64) * b) * (1 + rng.choice([0.0, 2.0 ** -24, 2.0 ** -30, 1.0], 2000))).astype(np.float32)  # cancellation
    got = R.fmaf(a, b, c)
    for i in range(2000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # (Fraction -> float64 is correctly rounded; check the float32 neighbours exactly)
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
        assert abs(Fraction(float(got[i])) - exact) == abs(Fraction(float(best)) - exact), i


def test_score_is_the_mahalanobis_distance():
    d = E.inputs("poly")
    e, nees, st = R.score(d["truth"], d["x"], d["P"])
    assert not st.any() and np.abs(E.boxplus(d["x"], e) - d["truth"]).max() <= 1e-12
    direct = np.array([e[:, k] @ np.linalg.inv(d["P"][:, :, k]) @ e[:, k] for k in range(e.shape[1])])
    assert np.abs(nees - direct).max() <= 1e-9 * direct.max()


def loop_inputs(name="poly", repeat=2, shrink=2.0, T_=60, seed=7):
    """test_ekf_ref's consistency settings (P0 and the sigma of Qd shrunk by 2), the LQR about every trim of the grid"""
    d = E.inputs(name, scale=1.0 / shrink)
    orc = d["orc"]
    x, u, P = (np.tile(d[k], repeat) for k in ("x", "u", "P"))
    N = x.shape[1]
    Qd, Rd = np.tile(d["Qd"], repeat) / shrink ** 2, np.tile(d["Rd"], repeat)
    rng = np.random.default_rng(seed)
    truth0 = E.boxplus(x, np.stack([np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12) for k in range(N)], axis=1))
    A, B = L.oracle_projection(orc, x, u)
    K = L.solve(A, B)[1]
    Xnom = orc.rollout(x, np.repeat(u[None], T_, axis=0), E.DT)
    return dict(orc=orc, eps=d["eps"], x=x, u=u, P=P, Qd=Qd, Rd=Rd, truth0=truth0, Xnom=Xnom, Unom=np.repeat(u[None], T_, axis=0),
                Kx=L.expand(Xnom, K), T=T_, N=N)


def test_zero_noise_loop_is_the_state_feedback_loop():
    """sigma = 0, every sensor at every step, feedback from the truth: the truth is lqr_ref.closed_loop's, and Z is h of it"""
    c = loop_inputs(repeat=1, T_=8)
    lo, hi = np.full(7, -np.inf), np.full(7, np.inf)
    out = R.rollout(c["orc"], c["truth0"], c["x"], c["P"], c["Xnom"], c["Unom"], c["Kx"], c["Qd"], c["Rd"], None, np.zeros(15), R.Sensors(),
                    E.DT, lo, hi, c["eps"], feedback="truth")
    X, U, _ = L.closed_loop(c["orc"], c["truth0"], c["x"], c["u"], c["Kx"], E.DT, Xnom=c["Xnom"])
    assert np.abs(out["X"] - X).max() <= 1e-9 and np.abs(out["U"] - U).max() <= 1e-9 and (out["mask"] == E.ALL).all()
    assert np.abs(out["Z"] - np.stack([E.h(x, E.MAG, c["eps"]) for x in X[1:]])).max() <= 1e-9


def test_the_closed_loop_is_consistent():
    """T = 60 steps of the loop closed through the EKF (feedback from the estimate, GPS every 10th step, the other sensors at
    every step, process noise sqrt(Qd) on the truth) on the cubic-fit trims times two.  Per instance, the mean over the run of
    NEES / 12 and of NIS per used row; the sampling standard deviation of their means from the spread across the instances.
    A consistent filter gives 1 for both: each mean stays within 5 of its standard deviations of 1."""
    c = loop_inputs()
    s = R.Sensors(seed=2024, period=(10, 10, 1, 1, 1))
    lo, hi = np.full(7, -np.inf), np.full(7, np.inf)
    out = R.rollout(c["orc"], c["truth0"], c["x"], c["P"], c["Xnom"], c["Unom"], c["Kx"], c["Qd"], c["Rd"], np.sqrt(c["Qd"]), np.sqrt(c["Rd"]),
                    s, E.DT, lo, hi, c["eps"])
    assert (out["status"] == 0).all() and np.isfinite(out["X"]).all()
    rows = np.array([[bin(int(v)).count("1") for v in r] for r in out["used"]])
    assert (rows[9::10] == 15).all() and (np.delete(rows, np.s_[9::10], axis=0) == 9).all()
    nees = out["nees"].mean(axis=0) / 12
    nis = out["nis"].sum(axis=0) / rows.sum(axis=0)
    for name, v in (("nees / 12", nees), ("nis / row", nis)):
        mean, sd = v.mean(), v.std(ddof=1) / np.sqrt(c["N"])
        print(f"[lqg ref] consistency over {c['N']} instances x {c['T']} steps: mean {name} {mean:.4f}, sampling sd {sd:.4f}")
        assert abs(mean - 1) <= 5 * sd, (name, mean, sd)
    # the loop holds the flight: the estimate's error stays where P says, the truth stays near the nominal
    assert np.abs(out["X"][-1, 3:6] - c["Xnom"][-1, 3:6]).max() <= 5.0
