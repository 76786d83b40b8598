"""The float64 restatement of the LQR about a trim (tests/lqr_ref.py) against independent references, on the CPU: the Riccati
solve against scipy, the analytic T and E against central differences of the chart, the invariance of A_xi along a trim
helix, the ignorable coordinates, and closed-loop stability on every instance of the grid that trims."""
import numpy as np
import pytest

from tests import lqr_ref as L

MODELS = ("poly", "default")


@pytest.fixture(scope="module", params=MODELS)
def case(request):
    ac, orc, x, u = L.grid(request.param)
    A, B = L.oracle_projection(orc, x, u)
    return request.param, orc, x, u, A, B


def test_grid_trims(case):
    name, orc, x, u, A, B = case
    assert x.shape[1] >= 40  # 42 of the 48 grid points trim in float64


@pytest.mark.parametrize("sel", sorted(L.SELECTIONS))
def test_doubling_matches_scipy(case, sel):
    import scipy.linalg as sl

    name, orc, x, u, A, B = case
    q = L.SELECTIONS[sel]
    P, K, res, st, it = L.solve(A, B, q)
    assert (st == 0).all() and it.max() <= 16 and res.max() <= 1e-12
    keep = [i for i in range(12) if i not in L.dropped(q)]
    ctl = [0, 1, 2, 6]  # the thrust columns of B are exactly zero
    worst = 0.0
    for i in range(A.shape[2]):
        a, b = L.reduce(A[:, :, i], B[:, :, i], q)
        Ps = sl.solve_discrete_are(a[np.ix_(keep, keep)], b[keep][:, ctl], np.diag(q[keep]), np.eye(len(ctl)))
        worst = max(worst, np.abs(P[:, :, i][np.ix_(keep, keep)] - Ps).max() / np.abs(Ps).max())
    print(f"[lqr ref] {name} selection {sel}: worst |P - scipy| / |P| {worst:.1e}, doubling steps {it.min()}..{it.max()}")
    assert worst <= 1e-10
    d = L.dropped(q)
    assert (P[d] == 0).all() and (P[:, d] == 0).all() and (K[:, d] == 0).all() and (K[3:6] == 0).all()


def test_T_and_E_match_central_differences(case):
    name, orc, x, u, A, B = case
    n, h = x.shape[1], 1e-6
    Tm, Em = L.T_of(x), L.E_of(x)
    for j in range(12):
        e = np.zeros((12, n))
        e[j] = h
        assert np.abs(Tm[:, j] - (L.unchart(e, x) - L.unchart(-e, x)) / (2 * h)).max() <= 1e-7
    for j in range(13):
        e = np.zeros((13, n))
        e[j] = h
        assert np.abs(Em[:, j] - (L.chart(x + e, x) - L.chart(x - e, x)) / (2 * h)).max() <= 1e-7
    # E T = I up to the rounding of the float32-exact attitude's norm (|v| <= 70 m/s times 1e-7)
    assert np.abs(L.mm(Em, Tm) - np.eye(12)[:, :, None]).max() <= 1e-5
    assert np.abs(L.chart(x, x)).max() == 0.0
    xi = np.random.default_rng(0).uniform(-0.1, 0.1, (12, n))
    assert np.abs(L.chart(L.unchart(xi, x), x) - xi).max() <= 1e-12


def steady(orc, x, u, H=50):
    """instances whose oracle rollout stays on the helix for H steps (an open-loop unstable trim leaves it: the trim's
    own residual of up to 1e-4 grows with rho(A)^H), and the rollout's last state"""
    X = orc.rollout(x, np.repeat(u[None], H, axis=0), L.DT)
    vb0 = L.mtv(L.rotmat(L.unit(x[6:10])), x[3:6])
    with np.errstate(all="ignore"):
        vb = L.mtv(L.rotmat(L.unit(X[-1][6:10])), X[-1][3:6])
        ok = (np.abs(vb - vb0).max(0) <= 1e-3) & (np.abs(X[-1][10:13] - x[10:13]).max(0) <= 1e-4)
    return ok, X[-1]


def test_projection_is_invariant_along_the_helix(case):
    """A_xi, B_xi at the trim state and at its 50-step rollout agree.  The bar: the rollout leaves the exact helix by what the
    trim's residual (<= 1e-4 m/s^2, rad/s^2) integrates to in 0.5 s, <= 1e-4 in the state, and A_xi moves by dt x the
    second derivatives (of order 10) x that: 1e-5."""
    name, orc, x, u, A, B = case
    ok, x50 = steady(orc, x, u)
    assert ok.sum() >= (40 if name == "poly" else 10), ok.sum()
    A2, B2 = L.oracle_projection(orc, x50[:, ok], u[:, ok])
    dA, dB = np.abs(A[:, :, ok] - A2).max(), np.abs(B[:, :, ok] - B2).max()
    print(f"[lqr ref] {name}: {ok.sum()} instances stay on the helix; max |dA_xi| {dA:.1e}, |dB_xi| {dB:.1e}")
    assert dA <= 1e-5 and dB <= 1e-5
    # the raw 13-state Jacobians do differ along a turning helix
    turning = ok & (np.abs(x[12]) > 0.01)
    _, Ar, _, _ = orc.step_sens(x[:, turning], u[:, turning], L.DT)
    _, Ar2, _, _ = orc.step_sens(x50[:, turning], u[:, turning], L.DT)
    assert np.abs(Ar - Ar2).max() >= 1e-3


def test_ignorable_coordinates(case):
    """Coordinates 0, 1, 2, 8 feed none of the other eight; among themselves the columns are kinematics: along- and
    cross-track rotate with the heading frame (the identity columns in straight flight), down is the identity column,
    and a heading error moves the position error by the step's displacement turned a quarter."""
    name, orc, x, u, A, B = case
    others = [i for i in range(12) if i not in L.IGNORABLE]
    assert np.abs(A[others][:, list(L.IGNORABLE)]).max() <= 2e-8
    n = x.shape[1]
    xp = orc.state_update(x, u, L.DT)
    dpsi = L.yaw(L.unit(xp[6:10])) - L.yaw(L.unit(x[6:10]))
    c, s = np.cos(dpsi), np.sin(dpsi)
    want = np.zeros((12, 4, n))
    want[0, 0], want[1, 0], want[0, 1], want[1, 1] = c, -s, s, c
    want[2, 2] = 1.0
    want[8, 3] = 1.0
    dp = L.mtv(L.heading(L.unit(xp[6:10])), xp[0:3] - x[0:3])
    want[0, 3], want[1, 3] = -dp[1], dp[0]
    assert np.abs(A[:, list(L.IGNORABLE)] - want).max() <= 2e-8
    straight = np.abs(x[12]) < 1e-6
    assert straight.any()
    eye = np.eye(12)[:, [0, 1, 2]]
    assert np.abs(A[:, [0, 1, 2]][:, :, straight] - eye[:, :, None]).max() <= 2e-8


@pytest.mark.parametrize("sel", sorted(L.SELECTIONS))
def test_closed_loop_is_stable(case, sel):
    name, orc, x, u, A, B = case
    q = L.SELECTIONS[sel]
    P, K, res, st, it = L.solve(A, B, q)
    r = L.rho(A, B, K, q)
    print(f"[lqr ref] {name} selection {sel}: rho(A - BK) {r.min():.4f} .. {r.max():.4f}")
    assert (r < 1).all()


def test_closed_loop_oracle_decays():
    """The float64 loop alone: from a start of |xi_0| = 0.5 m, 0.5 m/s, 0.02 rad, 0.02 rad/s per coordinate (random signs)
    the cost-to-go xi' P xi falls from the first node to the last over H = 200 steps of 0.01 s, on every instance (this is
    the start the GPU closed-loop test uses)."""
    ac, orc, x, u = L.grid("poly")
    A, B = L.oracle_projection(orc, x, u)
    P, K, *_ = L.solve(A, B, L.Q11)
    xi0 = L.closed_loop_start(x.shape[1])
    x0 = L.unchart(xi0, x)
    Kx = L.expand(orc.rollout(x, np.repeat(u[None], 200, axis=0), L.DT), K)
    X, U, Xnom = L.closed_loop(orc, x0, x, u, Kx)
    v0, vH = L.cost_to_go(X[0], Xnom[0], P), L.cost_to_go(X[-1], Xnom[-1], P)
    print(f"[lqr ref] closed loop: xi'P xi falls by {np.min(v0 / vH):.1f} .. {np.max(v0 / vH):.1f} x")
    assert (vH < v0).all()
