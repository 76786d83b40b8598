"""The float64 restatement of the EM statistics for the EKF's noise variances (tests/em_ref.py) against what is not the kernel's
formula, on the CPU: the textbook form of E[w w' | all data] from the smoother gains, Abar and node k-1; a numpy float32
imitation of both forms (the evidence for the kernel's choice); the pooled EM loop in the Monte-Carlo set-up of
tests/test_ekf_ref.py; and the planted failure paths."""
import numpy as np
import pytest

from tests import ekf_ref as E
from tests import em_ref as M
from tests import rts_ref as R


def q_measure(a, ref):
    return float((np.abs(a - ref["Qsum"]) / ref["Qabs"]).max())


@pytest.mark.parametrize("name", E.MODELS)
def test_the_two_forms_agree_on_the_chain_records(name):
    """The innovations form (em_ref.noise_stats) against the textbook form on rts_ref.chain_records, within rts_ref's bar for
    "against what is not the recursion": 1e-8 of the Q measure.

    chain_records rounds P, P- and Abar to float32 AFTER the filter ran, so the process noise these records are consistent with
    is Q~_k = P-_k - Abar_k P_{k-1} Abar_k' and no longer diag(Qd): it differs by 6e-8 |P-_k| ~ 2e-7 where the position variances of
    Q are 1e-4.  The textbook form never reads Q; it is the innovations form with Q~_k (I - Abar_k C_k = Q~_k (P-_k)^-1).  So the
    innovations form is given the records' own Q~_k here, as rts_ref.joint_marginals takes the links' Q from the records for the
    same bar.  With diag(Qd) on these rounded records the two differ by 4.0e-4 .. 4.6e-4 (printed; parts in 1e3 of Q, the size
    of the rounding); with diag(Qd) on the chains' records before the rounding they agree to 1e-8 as well
    (test_the_two_forms_agree_on_consistent_records)."""
    c = M.chain_case(name)
    s = c["s64"]
    Qk = c["Ppred"] - np.stack([M.mm(M.mm(c["Abar"][k], c["P_prev"][k]), M.tr(c["Abar"][k])) for k in range(c["Abar"].shape[0])])
    a = (c["Xpred"], c["Ppred"], s["X"], s["P"], c["Z"], c["used"], c["Qd"], c["Rd"])
    ref, diag = M.noise_stats(*a, eps=c["eps"], Qk=Qk), M.noise_stats(*a, eps=c["eps"])
    tb, _ = M.noise_stats_textbook(c["Xpred"], s["X"], s["P"], c["Abar"], c["C"], c["Ps_prev"])
    e = q_measure(tb, ref)
    print(f"[em ref] {name}: textbook against innovations form on the float32-rounded chain records: {e:.2e} with the records' own "
          f"Q_k, {q_measure(tb, diag):.2e} with diag(Qd)")
    assert e <= 1e-8


@pytest.mark.parametrize("name", E.MODELS)
def test_the_two_forms_agree_on_consistent_records(name):
    """The same chains, the float64 filter's records as it computed them (P-_k = Abar_k P_{k-1} Abar_k' + Q to float64 rounding):
    the two forms agree within 1e-8 of the Q measure (measured 3.7e-12 .. 6.3e-12)."""
    c = E.chain_inputs(name)
    r = M.filter_run(c["orc"].step_sens, c["x"], c["P"], c["u"], c["Z"], c["masks"], c["Qd"], c["Rd"], E.MAG, c["eps"])
    s = R.smooth(r["X"], r["P"], r["Xpred"], r["Ppred"], r["Abar"], c["x"], c["P"])
    ref = M.noise_stats(r["Xpred"], r["Ppred"], s["X"], s["P"], c["Z"], r["used"], c["Qd"], c["Rd"], eps=c["eps"])
    tb, _ = M.noise_stats_textbook(r["Xpred"], s["X"], s["P"], r["Abar"], s["C"], np.concatenate([s["P0"][None], s["P"][:-1]]))
    e = q_measure(tb, ref)
    print(f"[em ref] {name}: textbook against innovations form on the float64 records: {e:.2e}")
    assert e <= 1e-8


@pytest.mark.parametrize("name", E.MODELS)
def test_float32_imitation_of_both_forms(name):
    """Both forms with every product and sum rounded to float32 (numpy), against the float64 statistic on the same inputs: the
    innovations form is the more accurate one (measured 2.1e-7 .. 2.9e-7 against 2.0e-3 .. 3.1e-3 of the Q measure: the textbook
    form subtracts P-sized terms to get Q-sized ones).  Recorded, and asserted only as innovations <= textbook."""
    c = M.chain_case(name)
    s = c["s64"]
    ref = M.noise_stats(c["Xpred"], c["Ppred"], s["X"], s["P"], c["Z"], c["used"], c["Qd"], c["Rd"], eps=c["eps"])
    ei = q_measure(M.q_terms_innovations(c["Xpred"], c["Ppred"], s["X"], s["P"], c["Qd"], np.float32).sum(0), ref)
    et = q_measure(M.q_terms_textbook(c["Xpred"], s["X"], s["P"], c["Abar"], c["C"], c["Ps_prev"], np.float32).sum(0), ref)
    print(f"[em ref] {name}: float32 imitation, innovations form {ei:.2e}, textbook form {et:.2e}")
    assert ei <= et


def test_pooled_em_raises_the_likelihood():
    """The set-up of tests/test_ekf_ref.py's consistency test (84 filters x 50 steps on the cubic-fit trims, GPS every 10th step,
    P0 and the sigma of Qd shrunk by 2), one airframe with 84 logs: the pooled float64 loop from sigma wrong by 4 x (even
    components of q and odd rows of r 4 x too large, the others 4 x too small).  The pooled log-likelihood rises at every one
    of the ten iterations (measured -40652 -> 78368 -> ... -> 84669) and ends above where it began.  Where the sigma end
    relative to truth is recorded in DESIGN.md §4.17: every r within 13 % but the third GPS row; the q of position and
    velocity, seen by GPS five times in a log, do not move."""
    SHRINK, T_, REPEAT, ITERS = 2.0, 50, 2, 10
    d = E.inputs("poly", scale=1.0 / SHRINK)
    orc, eps = d["orc"], d["eps"]
    x, u, P = (np.tile(d[k], REPEAT) for k in ("x", "u", "P"))
    N = x.shape[1]
    assert N == 84
    Qd, Rd = np.tile(d["Qd"], REPEAT) / SHRINK ** 2, np.tile(d["Rd"], REPEAT)
    rng = np.random.default_rng(7)
    truth0 = E.boxplus(x, np.stack([np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12) for k in range(N)], axis=1))
    _, Z = E.simulate(orc, truth0, u, T_, Qd, Rd, rng, E.MAG, eps)
    masks = np.full((T_, N), E.ALL & ~E.GPS, np.int32)
    masks[9::10] = E.ALL
    q = Qd * np.where(np.arange(12) % 2 == 0, 16.0, 1 / 16.0)[:, None]
    r = Rd * np.where(np.arange(15) % 2 == 0, 1 / 16.0, 16.0)[:, None]
    ll = []
    for it in range(ITERS):
        st, l, _ = M.em_iteration(orc.step_sens, x, P, u, Z, masks, q, r, E.MAG, eps)
        assert (st["status"] == 0).all()
        ll.append(float(l.sum()))
        q, r = M.pooled(st, q, r)
        assert (q == q[:, :1]).all() and (r == r[:, :1]).all()
    ll.append(float(M.filter_run(orc.step_sens, x, P, u, Z, masks, q, r, E.MAG, eps)["ll"].sum()))
    print("[em ref] pooled ll per iteration: " + " ".join(f"{v:.0f}" for v in ll))
    print("[em ref] sigma_q / truth: " + " ".join(f"{v:.2f}" for v in np.sqrt(q[:, 0] / Qd[:, 0])))
    print("[em ref] sigma_r / truth: " + " ".join(f"{v:.2f}" for v in np.sqrt(r[:, 0] / Rd[:, 0])))
    assert ll[-1] > ll[0]
    assert all(b > a for a, b in zip(ll, ll[1:])), ll


def test_planted_cases():
    """A non-PD P- (the node is out of Q, its R terms stay), a NaN record (the node adds nothing), a row never used (nr = 0, Rn
    the input), T = 0 (zero sums and counts, Qn, Rn the inputs); the untouched instance is what it is without the planted ones."""
    from tests.test_host_em import planted

    c = M.chain_case("poly")
    T_ = c["Xpred"].shape[0]
    a, want = planted(c)
    s = M.noise_stats(*[a[k] for k in M.ARGS], eps=c["eps"])
    clean = M.noise_stats(*[c[k][..., :4] for k in M.ARGS], eps=c["eps"])
    assert np.array_equal(s["status"], want)
    assert list(s["nq"]) == [T_, T_ - 2, T_ - 1, T_ - 1]
    assert (s["nr"][6:, 1] == T_).all() and np.array_equal(s["Rsum"][:, 1], clean["Rsum"][:, 1])   # the R terms of a non-PD node stay
    assert (s["nr"][6:, 2] == T_ - 1).all() and (s["Rsum"][6:, 2] < clean["Rsum"][6:, 2]).all()  # the NaN node adds nothing
    assert s["nr"][0, 3] == 0 and s["Rsum"][0, 3] == 0 and s["Rn"][0, 3] == c["Rd"][0, 3]
    assert np.isfinite(s["Qsum"]).all() and np.isfinite(s["Rsum"]).all()
    for k in ("Qsum", "Rsum", "Qn", "Rn", "nq", "nr"):
        assert np.array_equal(s[k][..., 0], clean[k][..., 0]), k
    z = M.noise_stats(*[c[k][:0] if k not in ("Qd", "Rd") else c[k] for k in M.ARGS], eps=c["eps"])
    assert (z["Qsum"] == 0).all() and (z["Rsum"] == 0).all() and (z["nq"] == 0).all() and (z["nr"] == 0).all()
    assert np.array_equal(z["Qn"], c["Qd"]) and np.array_equal(z["Rn"], c["Rd"])
