"""CPU checks of tests/riccati_rate_ref.py: the float64 restatement of the exact control-rate Riccati pass against a dense
solve of the stacked problem, its reductions to oracle/ilqr_oracle.py, the conditions of every case of the GPU matrix, and the
float64 rate models against central differences of the float64 losses."""
import numpy as np
import pytest

import ilqr_oracle as io
from tests import cost_terms_ref as ct
from tests import riccati_rate_ref as rr
from tests.riccati_ref import synthetic_riccati

INPUT_SETS = {"gn": dict(), "node": dict(node=True), "node_newton": dict(node=True, newton=True)}


@pytest.mark.parametrize("H", [1, 2, 4, 5, 9, 23])
@pytest.mark.parametrize("name", list(INPUT_SETS))
def test_recursion_matches_the_dense_stacked_solve(name, H):
    """The policy (k, Kx, Kp) rolled out on the linear model IS the minimiser of the stacked quadratic, and dV0 + dV1 its
    optimum value.  Both sides are float64 on the same O(1) inputs; 1e-11 leaves three digits over the condition of the
    stacked matrix (about 1e3) times the unit round-off."""
    B = 3
    inp = synthetic_riccati(B, H, 400 + H, **INPUT_SETS[name])
    g, h = rr.synthetic_rate(B, H, 900 + H)
    K, Kp, kff, dV, lo = rr.reference(inp, (g, h))
    assert lo >= rr.QUU_MIN
    for b in range(B):
        du, _, J, eig = rr.dense_solution(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], g, h, b, node=inp["node"], Hz=inp["Hz"])
        assert eig > 0
        got = rr.policy_on_linear_model(K, Kp, kff, inp["A"], inp["Bm"], b)
        assert np.abs(got - du).max() <= 1e-11 * max(1.0, np.abs(du).max()), (name, H, b, np.abs(got - du).max())
        assert abs(dV[0, b] + dV[1, b] - J) <= 1e-11 * abs(J), (name, H, b, dV[:, b], J)


@pytest.mark.parametrize("name,kw", [("gn", dict()), ("node", dict(node=True)), ("newton", dict(newton=True)),
                                     ("node_newton", dict(node=True, newton=True))])
def test_zero_rate_model_is_the_plain_pass(name, kw):
    B, H = 4, 9
    inp = synthetic_riccati(B, H, 77, **kw)
    z = np.zeros((H, 7, B))
    K, Kp, kff, dV, _ = rr.reference(inp, (z, z))
    Kr, kr, dVr = io.backward(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"])
    assert (Kp == 0).all()
    assert np.abs(K - Kr).max() <= 1e-12 * np.abs(Kr).max() and np.abs(kff - kr).max() <= 1e-12 * np.abs(kr).max()
    assert np.abs(dV - dVr).max() <= 1e-12 * np.abs(dVr).max()


def test_zero_row_zero_gives_no_gain_on_the_control_before_the_window():
    B, H = 4, 6
    inp = synthetic_riccati(B, H, 78, node=True)
    g, h = (a.copy() for a in rr.synthetic_rate(B, H, 79))
    g[0] = 0.0; h[0] = 0.0
    K, Kp, kff, dV, _ = rr.reference(inp, (g, h))
    assert (Kp[0] == 0).all() and (np.abs(Kp[1:]).max(axis=(1, 2)) > 0).all()


CASES = rr.matrix()


@pytest.mark.parametrize("variant,B,H", CASES, ids=[f"{v}-B{B}-H{H}" for v, B, H in CASES])
def test_every_gpu_case_meets_its_conditions(variant, B, H):
    c = rr.rate_case(variant, B, H)
    assert c["e32"] <= rr.E32_MAX, (variant, B, H, c["e32"])
    assert c["quu_min"] >= rr.QUU_MIN, (variant, B, H, c["quu_min"])
    assert rr.bar_of(c["e32"]) <= 1e-4


def test_horizons_follow_the_ring_depths():
    assert rr.horizons(False) == [1, 2, 7, 8, 9, 15, 16, 17, 23] and rr.horizons(True) == [1, 2, 4, 5, 6, 9, 10, 11, 23]


# ---- rate models against central differences of the float64 losses ---------------------------------------------------------------
def _central(f, U, k, i, step):
    up, um = U.copy(), U.copy()
    up[k, i] += step; um[k, i] -= step
    return (f(up) - f(um)) / (2 * step)


def test_quadratic_rate_model_is_the_derivative_of_the_quadratic_rate_cost():
    rng = np.random.default_rng(5)
    H, B = 5, 6
    U = rng.normal(size=(H, 7, B)); up = rng.normal(size=(7, B))
    w = rng.uniform(0.5, 3.0, 7); w[3] = 0.0
    for prev in (None, up):
        g, h = rr.quad_rate_model(np.float64, w, U, prev)
        f = lambda V: rr.quad_rate_cost(np.float64, w, V, prev)  # noqa: E731
        for k in range(H):
            for i in range(7):
                # dJ/du_k = g_k - g_{k+1};  d2J/du_k^2 = h_k + h_{k+1}   (the cost is quadratic: central differences are exact)
                want = g[k, i] - (g[k + 1, i] if k + 1 < H else 0.0)
                assert np.abs(_central(f, U, k, i, 1e-3) - want).max() <= 1e-9
                curv = (f(_shift(U, k, i, 1e-2)) - 2 * f(U) + f(_shift(U, k, i, -1e-2))) / 1e-4
                assert np.abs(curv - (h[k, i] + (h[k + 1, i] if k + 1 < H else 0.0))).max() <= 1e-7
        if prev is None:
            assert (g[0] == 0).all() and (h[0] == 0).all()


def _shift(U, k, i, s):
    V = U.copy(); V[k, i] += s
    return V


@pytest.mark.parametrize("time_row", [0, 6])
def test_l0_rate_model_is_the_derivative_of_the_goal_loss(time_row):
    """io.goal_cost depends on U through the rate term only: dJ/du_k = g_k - g_{k+1} with g = w_rate l0'(d).  Step 1e-5 on
    differences of the scale sqrt(eps) = 0.1: the truncation error of the central difference is about l0''' h^2 / 6 <= 1e-6
    of the gradient's scale 2 w / sqrt(eps)."""
    H = 5
    inp = ct.goal_inputs(8, 1, H, 4242)
    gl = ct.goal_loss(time_row)
    orc = ct._oracle()
    U = inp["U"]
    g, h = rr.l0_rate_model(np.float64, gl, U)
    assert (g[0] == 0).all() and (h[0] == 0).all() and (h >= 0).all()
    if time_row:
        assert (g[:, time_row] == 0).all() and (h[:, time_row] == 0).all()
    d = U[1:] - U[:-1]
    zero = (d == 0)
    assert zero.any()       # equal consecutive controls: the limit branch, curvature 2 w / eps exactly
    rows = io._rate_rows(gl)
    zr = zero[:, rows]
    assert np.allclose(h[1:][:, rows][zr], 2 * gl.w_rate / gl.eps_rate, rtol=1e-15) and (g[1:][:, rows][zr] == 0).all()
    f = lambda V: io.goal_cost(orc, gl, inp["goal"], inp["X"], V, inp["lam"])  # noqa: E731
    scale = 2 * gl.w_rate / np.sqrt(gl.eps_rate)
    for k in range(H):
        for i in range(7):
            want = g[k, i] - (g[k + 1, i] if k + 1 < H else 0.0)
            assert np.abs(_central(f, U, k, i, 1e-5) - want).max() <= 1e-5 * scale, (k, i)
    # Gauss-Newton curvature: l0 = 1/2 r^2 with r = sqrt(2 l0), r'^2 = l0'^2 / (2 l0), checked on r by central differences
    dd = d[~zero]
    r = lambda x: np.sign(x) * np.sqrt(2 * gl.w_rate * io.l0_smooth(x, gl.eps_rate))  # noqa: E731
    rp = (r(dd + 1e-6) - r(dd - 1e-6)) / 2e-6
    mask = np.zeros(7); mask[rows] = 1
    want_h = (h[1:] / np.maximum(mask[None, :, None], 1e-300))[~zero]
    sel = np.broadcast_to(mask[None, :, None] > 0, d.shape)[~zero]
    assert np.abs(rp[sel] ** 2 - want_h[sel]).max() <= 1e-5 * 2 * gl.w_rate / gl.eps_rate
