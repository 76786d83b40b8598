"""The float64 restatement of the unscented Kalman filter (tests/ukf_ref.py) against first principles, on the CPU: on
linear-Gaussian stand-ins it is the Kalman filter; its Cholesky-ordered innovations are the batch figures; in the small-P limit
it is the EKF, second order in the spread; rts_ref's recursion on its records is the unscented RTS smoother; and where the EKF is
inconsistent (the first step with the full P0) it is closer to consistent."""
import numpy as np
import pytest

from tests import ekf_ref as E
from tests import rts_ref as R
from tests import ukf_ref as U

rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
ROWS = [list(range(15)), [0, 1, 2, 3, 4, 5], list(range(6, 15)), [9], [4, 10, 13]]
# the UKF's mean nis per row over the first step of the §4.14 Monte-Carlo run with the full P0 and Qd, as this file measures it
# (DESIGN.md §4.18 quotes it; the EKF's on the same draws is 1.31)
UKF_FIRST_STEP = 1.09


def linear_case(kappa, m=6):
    """x, P of the cubic-fit grid; the images of the sigma points under F(x [+] d) = xb [+] A d; the linear measurement
    h(xm [+] d) = h(xm) + H d with the EKF's H at xm"""
    d = E.inputs("poly")
    x, P, Qd = d["x"][:, :m], d["P"][:, :, :m], d["Qd"][:, :m]
    rng = np.random.default_rng(5)
    A = np.repeat((np.eye(12) + 0.2 * rng.standard_normal((12, 12)))[:, :, None], m, axis=2)
    xb = E.boxplus(x, 0.1 * rng.standard_normal((12, m)))
    s = U.sigma(x, P, kappa)
    pts = s["pts"].copy()
    pts[0:3] += x[0:3, None]
    F = np.stack([E.boxplus(xb, E.mv(A, E.boxminus(pts[:, j], x))) for j in range(U.PTS)], axis=1)
    F[0:3] -= x[0:3, None]
    return d, x, P, Qd, A, xb, s, F


@pytest.mark.parametrize("kappa", (0.0, 3.0))
@pytest.mark.parametrize("rows", ROWS)
def test_linear_gaussian_step_is_the_kalman_step(kappa, rows):
    d, x, P, Qd, A, xb, s, F = linear_case(kappa)
    m = x.shape[1]
    xm, Pm, Ab = U.time_update(x, P, s["L"], s["ok"], F, Qd, kappa)
    Pk = E.mm(E.mm(A, P), E.tr(A))
    Pk[np.arange(12), np.arange(12)] += Qd
    assert rel(xm, xb) <= 1e-10 and rel(Pm, Pk) <= 1e-10 and rel(Ab, A) <= 1e-10
    H, h0 = E.H_of(xm, E.MAG, d["eps"]), E.h(xm, E.MAG, d["eps"])
    z, Rd = d["z"][:, :m], d["Rd"][:, :m]
    mask = np.full(m, sum(1 << i for i in rows))

    def hfun(xs):
        return h0 + E.mv(H, E.boxminus(xs, xm))

    out = U.measurement_update(xm, Pm, z, mask, Rd, kappa, hfun=hfun)
    Pj, dj, nis, ll = E.joseph(xm, Pm, z, rows, Rd, E.MAG, d["eps"])
    assert rel(out["P"], Pj) <= 1e-10 and rel(out["d"], dj) <= 1e-10 and rel(out["nis"], nis) <= 1e-10 and rel(out["ll"], ll) <= 1e-10
    # the Cholesky-ordered nu, S are the sequential filter's: row i given the rows before it
    seq = E.update(xm, Pm, z, mask, Rd, E.MAG, d["eps"])
    assert rel(out["nu"], seq["nu"]) <= 1e-10 and rel(out["S"], seq["S"]) <= 1e-10
    assert (out["used"] == mask).all() and (out["status"] == 0).all()
    assert (out["S"][[i for i in range(15) if i not in rows]] == 0).all() and out["S"][rows].min() > 0


def test_small_P_limit_is_the_ekf():
    """Abar against E(x-) A G(x) and P- against Abar P Abar' + Q as P0 shrinks: the difference is second order in the spread,
    about 100 x per 10 x in sigma (measured: Abar 1.14, 1.05e-2, 1.05e-4 at sigma x 1, 0.1, 0.01; P- 3e-7 in ekf_ref.err_P at 0.01)"""
    dA, dP = [], []
    for scale in (1.0, 0.1, 0.01):
        d = E.inputs("poly", scale=scale)
        x, u, P, orc = d["x"], d["u"], d["P"], d["orc"]
        xp, A, _, _ = orc.step_sens(x, u, E.DT)
        Ab, Pm = E.predict(x, P, xp, A, d["Qd"])
        s = U.sigma(x, P)
        F = U.propagate(orc.state_update, s["pts"], u)
        _, Pu, Au = U.time_update(x, P, s["L"], s["ok"], F, d["Qd"])
        dA.append(np.abs(Au - Ab).max())
        dP.append(float(E.err_P(Pu, Pm).max()))
    print("[ukf ref] small-P limit: |Abar - Abar_ekf| " + ", ".join(f"{v:.3g}" for v in dA) + "; P- " + ", ".join(f"{v:.3g}" for v in dP))
    for a, b in zip(dA[:-1], dA[1:]):
        assert 30 <= a / b <= 300, dA
    assert dA[-1] <= 1e-3 and dP[-1] <= 1e-6


def test_rts_recursion_on_ukf_records_is_the_unscented_smoother():
    T_, m = 8, 6
    c = E.chain_inputs("poly", T_=T_)
    orc, eps = c["orc"], c["eps"]
    x, P, u, Z, masks, Qd, Rd = (c[k][..., :m] for k in ("x", "P", "u", "Z", "masks", "Qd", "Rd"))

    def one(x_, P_, u_, z_, mask_, ll_):
        return U.step(orc.state_update, x_, P_, u_, z_, mask_, Qd, Rd, 0.0, E.MAG, eps)

    rec = U.chain(one, x, P, u, Z, masks)
    assert (rec["status"] == 0).all()
    sm = R.smooth(rec["X"], rec["P"], rec["Xpred"], rec["Ppred"], rec["Abar"], x, P)
    assert (sm["status"] == 0).all()
    xs, ps = rec["X"][-1], rec["P"][-1]
    for k in range(T_ - 1, -1, -1):
        xh, ph = (rec["X"][k - 1], rec["P"][k - 1]) if k > 0 else (x, P)
        s = U.sigma(xh, ph)
        C = U.cross_cov(s["L"], U.propagate(orc.state_update, s["pts"], u))
        G = np.stack([np.linalg.solve(rec["Ppred"][k][:, :, i], C[:, :, i].T).T for i in range(m)], axis=2)
        xs = E.boxplus(xh, E.mv(G, E.boxminus(xs, rec["Xpred"][k])))
        ps = ph + E.mm(E.mm(G, ps - rec["Ppred"][k]), E.tr(G))
        want_x, want_p = (sm["X"][k - 1], sm["P"][k - 1]) if k > 0 else (sm["X0"], sm["P0"])
        assert rel(want_x, xs) <= 1e-10 and rel(want_p, ps) <= 1e-10 and rel(sm["C"][k], G) <= 1e-9, k


def _redraws(name, repeat, seed):
    """ekf_ref.inputs(name) with `repeat` redraws of truth and measurement noise (full SIG_P0, no process noise: inputs()'s rule)"""
    d = E.inputs(name)
    x, u, P, Qd, Rd = (np.tile(d[k], repeat) for k in ("x", "u", "P", "Qd", "Rd"))
    n = x.shape[1]
    rng = np.random.default_rng(seed)
    dd = np.stack([np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12) for k in range(n)], axis=1)
    z = E.h(d["orc"].state_update(E.boxplus(x, dd), u, E.DT), E.MAG, d["eps"]) + np.sqrt(Rd) * rng.standard_normal((15, n))
    return d, x, u, P, Qd, Rd, z


@pytest.mark.parametrize("name", ("poly", "real_net"))
def test_first_step_is_closer_to_consistent_than_the_ekf(name):
    """One step from the full SIG_P0 with all 15 rows, 42 grid instances x 12 redraws = 7560 rows (sampling sd 0.016): the UKF's
    mean nis per row is closer to 1 than the EKF's on the same draws by at least 5 sd (measured: 10 sd on the cubic fits, 30 on
    the shipped net)."""
    d, x, u, P, Qd, Rd, z = _redraws(name, 12, 11)
    orc, eps = d["orc"], d["eps"]
    xp, A, _, _ = orc.step_sens(x, u, E.DT)
    ekf = E.step(x, P, xp, A, z, None, Qd, Rd, E.MAG, eps)
    ukf = U.step(orc.state_update, x, P, u, z, None, Qd, Rd, 0.0, E.MAG, eps)
    assert (ekf["status"] == 0).all() and (ukf["status"] == 0).all()
    rows = 15 * x.shape[1]
    sd = np.sqrt(2.0 / rows)
    me, mu = ekf["nis"].sum() / rows, ukf["nis"].sum() / rows
    print(f"[ukf ref] consistency {name}: mean nis / row EKF {me:.4f}, UKF {mu:.4f} over {rows} rows, sampling sd {sd:.4f}: "
          f"closer by {(abs(me - 1) - abs(mu - 1)) / sd:.1f} sd")
    assert rows >= 7000 and abs(mu - 1) <= abs(me - 1) - 5 * sd, (me, mu, sd)


def test_monte_carlo_first_step_without_shrinking():
    """The §4.14 Monte-Carlo run (84 filters x 50 steps, GPS every 10th step) WITHOUT the halving of P0 and sigma(Qd): the UKF's
    first-step mean nis per row is within 5 sampling sd of the figure DESIGN.md §4.18 records (UKF_FIRST_STEP)."""
    T_, REPEAT = 50, 2
    d = E.inputs("poly")
    orc, eps = d["orc"], d["eps"]
    x, u, P, Qd, Rd = (np.tile(d[k], REPEAT) for k in ("x", "u", "P", "Qd", "Rd"))
    N = x.shape[1]
    rng = np.random.default_rng(7)
    truth0 = E.boxplus(x, np.stack([np.linalg.cholesky(P[:, :, k]) @ rng.standard_normal(12) for k in range(N)], axis=1))
    _, Z = E.simulate(orc, truth0, u, T_, Qd, Rd, rng, E.MAG, eps)
    masks = np.full((T_, N), E.ALL & ~E.GPS, np.int32)
    masks[9::10] = E.ALL

    def one(x_, P_, u_, z_, mask_, ll_):
        return U.step(orc.state_update, x_, P_, u_, z_, mask_, Qd, Rd, 0.0, E.MAG, eps)

    ukf = U.chain(one, x, P, u, Z, masks)
    ekf = E.chain(E.step, orc.step_sens, x, P, u, Z, masks, Qd, Rd, E.MAG, eps)
    assert (ukf["status"] == 0).all()
    fig = {}
    for name, sl in (("whole run", slice(None)), ("first step", slice(0, 1))):
        rows = sum(bin(int(v)).count("1") for v in ukf["used"][sl].ravel())
        sd = np.sqrt(2.0 / rows)
        fig[name] = (ukf["nis"][sl].sum() / rows, ekf["nis"][sl].sum() / rows, sd)
        print(f"[ukf ref] Monte Carlo, {name}: mean nis / row UKF {fig[name][0]:.4f}, EKF {fig[name][1]:.4f} over {rows} rows, sampling sd {sd:.4f}")
    mu, _, sd = fig["first step"]
    assert abs(mu - UKF_FIRST_STEP) <= 5 * sd, (mu, UKF_FIRST_STEP, sd)
