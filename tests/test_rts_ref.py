"""The float64 restatement of the RTS smoother (tests/rts_ref.py) against what is not the recursion, on the CPU: the diagonal
blocks of the inverse of the block-tridiagonal joint information matrix built from the records alone; the consistency of the
smoothed estimate in a Monte-Carlo run (normalised estimation error squared against its chi-square mean, smoothed against
filtered RMS error); and the failure paths (a non-PD predicted covariance, a NaN record)."""
import numpy as np
import pytest

from tests import ekf_ref as E
from tests import rts_ref as R


@pytest.mark.parametrize("name", ("poly", "default"))
@pytest.mark.parametrize("initial", (False, True))
def test_recursion_gives_the_marginals_of_the_joint_information_matrix(name, initial):
    """Every fifth instance of the chain: the recursion's P^s at every node against the inverse of the joint information matrix
    (prior, per link Q_k = P-_k - Abar_k P_{k-1} Abar_k', per node P_k^-1 - (P-_k)^-1), to 1e-8 in err_P."""
    rec = R.chain_records(name)
    args = [rec[k] for k in ("X", "P", "Xpred", "Ppred", "Abar")] + ([rec["X0"], rec["P0"]] if initial else [])
    s = R.smooth(*args)
    assert (s["status"] == 0).all()
    worst = 0.0
    for i in range(0, rec["X"].shape[2], 5):
        M = R.joint_marginals(rec["P"][..., i], rec["Ppred"][..., i], rec["Abar"][..., i], rec["P0"][..., i] if initial else None)
        got = np.concatenate([s["P0"][None, :, :, i], s["P"][..., i]]) if initial else s["P"][..., i]
        for k in range(M.shape[0]):
            worst = max(worst, float(E.err_P(got[k][:, :, None], M[k][:, :, None])[0]))
    print(f"[rts ref] {name}, initial node {initial}: P^s against the joint information matrix, worst err_P {worst:.2e}")
    assert worst <= 1e-8
    # the smoothed covariance is no larger than the filtered one, and at the first node far smaller (GPS every fifth step)
    ratio = np.trace(s["P"][0]) / np.trace(rec["P"][0])
    print(f"[rts ref] {name}: trace P^s_0 / trace P_0 = {ratio.mean():.3f}")
    assert (ratio < 1).all()


def test_the_smoother_is_consistent():
    """The set-up of tests/test_ekf_ref.py's consistency test: 84 filters x 50 steps on the cubic-fit trims, truth driven by
    process noise through [+], GPS every 10th step, P0 and the sigma of Qd shrunk by its SHRINK = 2.  At the middle node the
    mean over the instances of e' (P^s)^-1 e / 12 with e = truth [-] x^s is chi-square(12) / 12 for a consistent smoother: within
    4 sampling standard deviations sqrt(2 / (12 * 84)) = 0.045 of 1.  The smoothed RMS error is no larger than the filtered one
    in each of the four blocks (p, v, attitude, w), over all nodes and instances."""
    SHRINK, T_, REPEAT = 2.0, 50, 2
    d = E.inputs("poly", scale=1.0 / SHRINK)
    orc, eps = d["orc"], d["eps"]
    x, u, P = (np.tile(d[k], REPEAT) for k in ("x", "u", "P"))
    N = x.shape[1]
    assert N == 84
    Qd, Rd = np.tile(d["Qd"], REPEAT) / SHRINK ** 2, np.tile(d["Rd"], REPEAT)
    rng = np.random.default_rng(7)
    truth0 = E.boxplus(x, np.stack([np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12) for k in range(N)], axis=1))
    Xt, Z = E.simulate(orc, truth0, u, T_, Qd, Rd, rng, E.MAG, eps)
    masks = np.full((T_, N), E.ALL & ~E.GPS, np.int32)
    masks[9::10] = E.ALL
    rec = R.filter_records(orc.step_sens, x, P, u, Z, masks, Qd, Rd, E.MAG, eps)
    assert (rec["status"] == 0).all()
    s = R.smooth(rec["X"], rec["P"], rec["Xpred"], rec["Ppred"], rec["Abar"], rec["X0"], rec["P0"])
    assert (s["status"] == 0).all()
    k = T_ // 2
    e = E.boxminus(Xt[k + 1], s["X"][k])
    nees = np.array([e[:, i] @ np.linalg.solve(s["P"][k][:, :, i], e[:, i]) for i in range(N)]) / 12
    sd = np.sqrt(2.0 / (12 * N))
    print(f"[rts ref] consistency at node {k}: mean NEES / 12 = {nees.mean():.4f}, sampling sd {sd:.4f}")
    assert abs(nees.mean() - 1) <= 4 * sd, (nees.mean(), sd)
    ef = np.stack([E.boxminus(Xt[t + 1], rec["X"][t]) for t in range(T_)])
    es = np.stack([E.boxminus(Xt[t + 1], s["X"][t]) for t in range(T_)])
    for name, sl in (("p", slice(0, 3)), ("v", slice(3, 6)), ("attitude", slice(6, 9)), ("w", slice(9, 12))):
        rf, rs = np.sqrt((ef[:, sl] ** 2).mean()), np.sqrt((es[:, sl] ** 2).mean())
        print(f"[rts ref] RMS error {name}: filtered {rf:.4e}, smoothed {rs:.4e}")
        assert rs <= rf, name
    # the initial node too
    e0f, e0s = E.boxminus(Xt[0], rec["X0"]), E.boxminus(Xt[0], s["X0"])
    assert np.sqrt((e0s ** 2).mean()) <= np.sqrt((e0f ** 2).mean())


def test_failure_paths():
    """A non-PD P- at one link, a NaN record at one link: the bits are set, the node before is the filtered one, the nodes
    further back are smoothed again from it, and the other instances are what they are without the crafted ones."""
    clean = {k: v[..., :3] for k, v in R.chain_records("poly").items()}
    rec = {k: v.copy() for k, v in clean.items()}
    T_ = rec["X"].shape[0]
    rec["Ppred"][11][:, :, 1] -= 2 * np.diag(np.diag(rec["Ppred"][11][:, :, 1]))  # negative diagonal
    rec["X"][6][4, 2] = np.nan                                                  # x^_6: an operand of link 7 (and node 6 itself)
    keys = ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")
    s, c = R.smooth(*[rec[k] for k in keys]), R.smooth(*[clean[k] for k in keys])
    want = np.zeros((T_, 3), np.int32)
    want[11, 1], want[7, 2] = R.NOT_PD, R.NONFINITE
    # link 6 reads the carried x^s_6 = the filtered (NaN) x^_6 as well
    want[6, 2] = R.NONFINITE
    assert np.array_equal(s["status"], want)
    assert np.array_equal(s["X"][10][:, 1], rec["X"][10][:, 1]) and np.array_equal(s["P"][10][:, :, 1], rec["P"][10][:, :, 1])
    assert (s["C"][11][:, :, 1] == 0).all()
    assert not np.array_equal(s["P"][9][:, :, 1], rec["P"][9][:, :, 1]) and (np.trace(s["P"][9][:, :, 1]) < np.trace(rec["P"][9][:, :, 1]))
    assert np.array_equal(s["X"][6][:, 2], rec["X"][6][:, 2], equal_nan=True) and np.array_equal(s["X"][5][:, 2], rec["X"][5][:, 2])
    assert not np.array_equal(s["P"][4][:, :, 2], rec["P"][4][:, :, 2]) and np.isfinite(s["X"][:6][:, :, 2]).all()
    for k in ("X", "P", "C", "X0", "P0"):
        assert np.array_equal(s[k][..., 0], c[k][..., 0]), k
    # after the broken link the recursion restarts from the filtered node: instance 1 before node 10 is a smoother of the
    # first eleven nodes alone
    short = R.smooth(*[rec[k][:11] for k in keys[:5]], rec["X0"], rec["P0"])
    assert np.array_equal(short["P"][:, :, :, 1], s["P"][:11][:, :, :, 1]) and np.array_equal(short["X"][:, :, 1], s["X"][:11][:, :, 1])
