"""GPU tests of the MPPI sampler, update and controller (ac_mppi_sample_f32, ac_mppi_update_f32, aircraft_amd.control.MPPI)
against the NumPy restatement (tests/mppi_ref.py) and the float64 oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import mppi_ref as R
from tests.helpers import f32_exact, make_aircraft, make_oracle, parity_report
from tests.test_host_mppi import make_opts, sample_tolerance

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 4), (1, 300, 3), (3, 300, 3), (130, 5, 2), (64, 8, 2), (257, 70, 1)]  # (B, K, H)
U_MIN, U_MAX = [-5, -5, -5, 0, -1, -1, 0], [5, 5, 5, 1, 1, 1, 1]
WIDTH = np.array(U_MAX, dtype=np.float64) - np.array(U_MIN, dtype=np.float64)
SIGMA = [0.7, 1.3, 0.4, 0.2, 0.05, 0.3, 0.1]
SEED = (1 << 40) + 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


class Low:
    """The two entry points called directly on torch buffers."""

    def __init__(self, gpu):
        import torch

        self.torch, self.gpu = torch, gpu
        self.ac = make_aircraft("poly")
        self.lib = self.ac._sync()
        self.it = torch.zeros((1,), device=gpu, dtype=torch.int32)

    def sample_rc(self, o, Unom, X0, K, Uc, X0c, it="own", B=None, H=None):
        H0, _, B0 = Unom.shape
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return self.lib.ac_mppi_sample_f32(self.ac._handle, C.byref(o) if o is not None else None,
                                           ptr(self.it) if it == "own" else it, ptr(Unom), ptr(X0), K, B0 if B is None else B,
                                           H0 if H is None else H, ptr(Uc), ptr(X0c), self.ac._stream())

    def sample(self, o, Unom, X0, K, it="own"):
        H, _, B = Unom.shape
        Uc = self.torch.full((H, 7, K * B), float("nan"), device=self.gpu)
        X0c = self.torch.full((13, K * B), float("nan"), device=self.gpu) if X0 is not None else None
        _lib.check(self.sample_rc(o, Unom, X0, K, Uc, X0c, it=it), "ac_mppi_sample_f32")
        return Uc, X0c

    def update_rc(self, o, J, Uc, Unom, K, Unew, stats, ws, ws_floats=None, it="own", B=None, H=None):
        H0, _, B0 = Unom.shape
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        return self.lib.ac_mppi_update_f32(self.ac._handle, C.byref(o) if o is not None else None,
                                           ptr(self.it) if it == "own" else it, ptr(J), ptr(Uc), ptr(Unom), K,
                                           B0 if B is None else B, H0 if H is None else H, ptr(Unew), ptr(stats), ptr(ws),
                                           (ws.numel() if ws is not None else 0) if ws_floats is None else ws_floats, self.ac._stream())

    def update(self, o, J, Uc, Unom, K, Unew=None, it="own"):
        H, _, B = Unom.shape
        Unew = self.torch.full((H, 7, B), float("nan"), device=self.gpu) if Unew is None else Unew
        stats = self.torch.full((4, B), float("nan"), device=self.gpu)
        n = C.c_size_t(0)
        _lib.check(self.lib.ac_mppi_workspace_floats(self.ac._handle, K, B, H, C.byref(n)), "ac_mppi_workspace_floats")
        ws = self.torch.full((n.value,), float("nan"), device=self.gpu)
        _lib.check(self.update_rc(o, J, Uc, Unom, K, Unew, stats, ws, it=it), "ac_mppi_update_f32")
        return Unew, stats


@pytest.fixture(scope="module")
def low(gpu):
    return Low(gpu)


def nominal(B, H, seed):
    return f32_exact(np.random.default_rng(seed).uniform(-6, 6, (H, 7, B)))  # some entries outside the box


def random_costs(B, K, seed):
    """costs spanning four decades; NaN and +inf on some samples; every cost of the last instance non-finite when B > 1"""
    rng = np.random.default_rng(seed)
    J = (10.0 ** rng.uniform(-1, 3, (K, B))).astype(np.float32)
    if K > 2:
        J[rng.integers(0, K, max(1, K // 7)), rng.integers(0, B, max(1, K // 7))] = np.nan
        J[rng.integers(0, K, max(1, K // 9)), rng.integers(0, B, max(1, K // 9))] = np.inf
    if B > 1:
        J[:, B - 1] = np.where(np.arange(K) % 2 == 0, np.nan, np.inf)
    return J.reshape(-1)


# ---- 1. sample against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,H", SHAPES)
def test_sample_matches_reference(gpu, low, B, K, H):
    Unom = nominal(B, H, seed=B + K)
    X0 = f32_exact(np.random.default_rng(1).normal(0, 10, (13, B)))
    lo, hi = np.float32(U_MIN)[None, :, None], np.float32(U_MAX)[None, :, None]
    clipped = np.minimum(np.maximum(Unom.astype(np.float32), lo), hi)
    worst = 0.0
    for sigma, it in ((SIGMA, 0), ([1.0, 0.5, 2.0, 0, 0, 0, 0], 0), (SIGMA, 5)):
        o = make_opts(sigma, U_MIN, U_MAX, seed=SEED)
        low.it.fill_(it)
        Uc, X0c = low.sample(o, dev(Unom, gpu), dev(X0, gpu), K)
        Uc, X0c = Uc.cpu().numpy(), X0c.cpu().numpy()
        ref, rad = R.sample(Unom, sigma, U_MIN, U_MAX, SEED, it, K, want_radius=True)
        tol = sample_tolerance(ref, rad, sigma)
        err = np.abs(Uc - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all()
        assert (Uc >= lo).all() and (Uc <= hi).all()  # (false for a NaN left unwritten)
        dead = [r for r in range(7) if sigma[r] == 0]
        assert np.array_equal(Uc.reshape(H, 7, K, B)[:, dead], np.repeat(clipped[:, dead, None, :], K, axis=2))
        assert np.array_equal(Uc[:, :, :B], clipped)  # keep_nominal: column k = 0
        assert np.array_equal(X0c.reshape(13, K, B), np.repeat(X0.astype(np.float32)[:, None, :], K, axis=1))
    low.it.fill_(0)
    print(f"sample ({B}, {K}, {H}): worst error {worst:.3f} of the tolerance")
    if K > 1:  # without keep_nominal column 0 is sampled too, and X0c may be left out
        o = make_opts(SIGMA, U_MIN, U_MAX, seed=SEED, keep_nominal=False)
        Uc, none = low.sample(o, dev(Unom, gpu), None, K)
        ref, rad = R.sample(Unom, SIGMA, U_MIN, U_MAX, SEED, 0, K, keep_nominal=False, want_radius=True)
        assert none is None and (np.abs(Uc.cpu().numpy() - ref) <= sample_tolerance(ref, rad, SIGMA)).all()
        # it_dev = NULL means it = 0
        Uc0, _ = low.sample(o, dev(Unom, gpu), None, K, it=None)
        assert low.torch.equal(Uc, Uc0)


# ---- 2. shard invariance -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,H,lo,hi", [(130, 5, 2, 3, 70), (3, 300, 3, 1, 2), (257, 70, 1, 64, 257)])
def test_sample_shard_invariance(gpu, low, B, K, H, lo, hi):
    Unom = nominal(B, H, seed=7)
    whole, _ = low.sample(make_opts(SIGMA, U_MIN, U_MAX, seed=SEED), dev(Unom, gpu), None, K)
    part, _ = low.sample(make_opts(SIGMA, U_MIN, U_MAX, seed=SEED, instance_offset=lo), dev(Unom[:, :, lo:hi], gpu), None, K)
    assert low.torch.equal(whole.view(H, 7, K, B)[..., lo:hi], part.view(H, 7, K, hi - lo))


# ---- 3. the device counter -----------------------------------------------------------------------------------------------------------
def test_iteration_counter(gpu, low):
    B, K, H = 3, 5, 4
    Unom = nominal(B, H, seed=8)
    o = make_opts(SIGMA, U_MIN, U_MAX, seed=SEED)
    low.it.fill_(2)
    a, _ = low.sample(o, dev(Unom, gpu), None, K)
    b, _ = low.sample(o, dev(Unom, gpu), None, K)
    assert low.torch.equal(a, b) and int(low.it) == 2  # sampling alone does not advance the counter
    low.update(o, dev(random_costs(B, K, 1), gpu), a, dev(Unom, gpu), K)
    assert int(low.it) == 3
    c, _ = low.sample(o, dev(Unom, gpu), None, K)
    ref, rad = R.sample(Unom, SIGMA, U_MIN, U_MAX, SEED, 3, K, want_radius=True)
    assert (np.abs(c.cpu().numpy() - ref) <= sample_tolerance(ref, rad, SIGMA)).all() and not low.torch.equal(a, c)
    low.update(o, dev(random_costs(B, K, 1), gpu), a, dev(Unom, gpu), K, it=None)  # NULL: nothing to advance
    assert int(low.it) == 3
    low.it.fill_(0)


# ---- 4. update against float64 on the same fp32 J and Uc -------------------------------------------------------------------------------
def check_update(low, gpu, J, Uc, Unom, K, lam, Unew=None):
    o = make_opts(SIGMA, U_MIN, U_MAX, lam=lam, seed=SEED)
    got, stats = low.update(o, dev(J, gpu), Uc, dev(Unom, gpu) if Unew is None else Unew, K, Unew=Unew)
    got, stats = f64(got), f64(stats)
    lam32 = float(np.float32(lam))
    ref, rstats = R.update(J.astype(np.float64), f64(Uc), Unom, K, lam32, U_MIN, U_MAX)
    err = np.abs(got - ref) / np.where(WIDTH > 0, WIDTH, 1.0)[None, :, None]
    assert err.max() <= 1e-5, err.max()
    assert np.array_equal(stats[0], rstats[0]) and np.array_equal(stats[2], rstats[2]) and np.array_equal(stats[3], rstats[3])
    assert (np.abs(stats[1] - rstats[1]) <= 1e-5 * rstats[1]).all()
    empty = rstats[2] == 0
    if empty.any():  # no finite cost: the nominal bit for bit, stats (+inf, 0, 0, -1)
        assert np.array_equal(got[:, :, empty], Unom[:, :, empty])
        assert np.isposinf(stats[0, empty]).all() and (stats[1, empty] == 0).all() and (stats[3, empty] == -1).all()
    return got, stats, float(err.max())


@pytest.mark.parametrize("B,K,H", SHAPES)
def test_update_matches_float64(gpu, low, B, K, H):
    Unom = nominal(B, H, seed=B * K)
    Uc, _ = low.sample(make_opts(SIGMA, U_MIN, U_MAX, seed=SEED), dev(Unom, gpu), None, K)
    worst = 0.0
    for lam in (0.1, 1.0, 100.0):
        J = random_costs(B, K, seed=K + H)
        got, stats, e = check_update(low, gpu, J, Uc, Unom, K, lam)
        worst = max(worst, e)
    print(f"update ({B}, {K}, {H}): worst |Unew - ref| / width {worst:.2e} (bar 1e-5)")
    if K == 1 and B == 1:  # one sample: the blend is that sample
        J1 = np.float32([3.0])
        got, stats, _ = check_update(low, gpu, J1, Uc, Unom, K, 1.0)
        assert (np.abs(got - f64(Uc)) <= 1e-5 * WIDTH[None, :, None]).all() and stats[3, 0] == 0 and stats[1, 0] == 1.0


@pytest.mark.parametrize("B,K,H", [(3, 300, 3), (130, 5, 2), (64, 8, 2)])
def test_update_special_costs(gpu, low, B, K, H):
    Unom = nominal(B, H, seed=3)
    Uc, _ = low.sample(make_opts(SIGMA, U_MIN, U_MAX, seed=SEED), dev(Unom, gpu), None, K)
    # equal costs: the plain mean, ESS = K, best index 0
    got, stats, _ = check_update(low, gpu, np.full(K * B, 7.5, np.float32), Uc, Unom, K, 1.0)
    mean = np.minimum(np.maximum(f64(Uc).reshape(H, 7, K, B).mean(axis=2), np.float64(U_MIN)[None, :, None]), np.float64(U_MAX)[None, :, None])
    assert (np.abs(got - mean) <= 1e-5 * WIDTH[None, :, None]).all()
    assert (np.abs(stats[1] - K) <= 1e-5 * K).all() and (stats[3] == 0).all()
    # a temperature so small that every weight but the best underflows: the best sample itself
    rng = np.random.default_rng(4)
    J = rng.uniform(1.0, 2.0, (K, B)).astype(np.float32)
    got, stats, _ = check_update(low, gpu, J.reshape(-1), Uc, Unom, K, 1e-9)
    best = J.argmin(axis=0)
    pick = np.take_along_axis(f64(Uc).reshape(H, 7, K, B), best[None, None, None, :], axis=2)[:, :, 0, :]
    assert np.array_equal(stats[3], best) and (stats[1] == 1.0).all()
    assert (np.abs(got - pick) <= 1e-5 * WIDTH[None, :, None]).all()
    # ties: the lowest index wins
    J[:] = 5.0
    J[K // 2] = 1.0
    J[K - 1] = 1.0
    _, stats, _ = check_update(low, gpu, J.reshape(-1), Uc, Unom, K, 1.0)
    assert (stats[3] == K // 2).all()
    # Unew aliased to Unom (instance B - 1 has no finite cost and keeps its nominal)
    Jr = random_costs(B, K, seed=5)
    Ua = dev(Unom, gpu)
    separate, _, _ = check_update(low, gpu, Jr, Uc, Unom, K, 1.0)
    aliased, _, _ = check_update(low, gpu, Jr, Uc, Unom, K, 1.0, Unew=Ua)
    assert np.array_equal(separate, aliased) and np.array_equal(f64(Ua), aliased)


def test_update_and_sample_argument_errors(gpu, low):
    torch = low.torch
    B, K, H = 3, 5, 4
    Unom = dev(nominal(B, H, seed=9), gpu)
    o = make_opts(SIGMA, U_MIN, U_MAX, seed=SEED)
    Uc, X0c = low.sample(o, Unom, dev(np.zeros((13, B)), gpu), K)
    X0 = dev(np.zeros((13, B)), gpu)
    J = dev(random_costs(B, K, 1), gpu)
    Unew, stats, ws = torch.full((H, 7, B), 42.0, device=gpu), torch.full((4, B), 42.0, device=gpu), torch.zeros(K * B, device=gpu)
    Ucx = torch.full_like(Uc, 42.0)
    low.it.fill_(11)
    BAD, WSP = -1, -6

    def bad_opts(**kw):
        oo = make_opts(SIGMA, U_MIN, U_MAX, seed=SEED)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(oo, k)[v[0]] = v[1]
            else:
                setattr(oo, k, v)
        return oo

    opts_cases = [bad_opts(lambda_=0.0), bad_opts(lambda_=-1.0), bad_opts(lambda_=float("nan")), bad_opts(lambda_=float("inf")),
                  bad_opts(sigma=(2, -0.1)), bad_opts(sigma=(6, float("nan"))), bad_opts(sigma=(0, float("inf"))),
                  bad_opts(u_min=(1, 6.0)), bad_opts(u_max=(4, float("nan")))]
    for oo in opts_cases:
        assert low.sample_rc(oo, Unom, None, K, Ucx, None) == BAD
        assert low.update_rc(oo, J, Uc, Unom, K, Unew, stats, ws) == BAD
    for kw in (dict(B=0), dict(H=0), dict(B=-3), dict(H=-1)):
        assert low.sample_rc(o, Unom, None, K, Ucx, None, **kw) == BAD
        assert low.update_rc(o, J, Uc, Unom, K, Unew, stats, ws, **kw) == BAD
    for k in (0, -2):
        assert low.sample_rc(o, Unom, None, k, Ucx, None) == BAD
        assert low.update_rc(o, J, Uc, Unom, k, Unew, stats, ws) == BAD
    # K B above 2^31 - 1 (checked before anything is touched: the buffers are far smaller)
    assert low.sample_rc(o, Unom, None, 1 << 20, Ucx, None, B=1 << 11) == BAD
    assert low.update_rc(o, J, Uc, Unom, 1 << 20, Unew, stats, ws, B=1 << 11) == BAD
    n = C.c_size_t(0)
    assert low.lib.ac_mppi_workspace_floats(low.ac._handle, 1 << 20, 1 << 11, 1, C.byref(n)) == BAD
    # NULL required pointers, X0 / X0c one without the other
    assert low.sample_rc(None, Unom, None, K, Ucx, None) == BAD
    assert low.sample_rc(o, Unom, None, K, None, None) == BAD
    assert low.sample_rc(o, Unom, X0, K, Ucx, None) == BAD
    assert low.sample_rc(o, Unom, None, K, Ucx, X0c) == BAD
    assert low.update_rc(None, J, Uc, Unom, K, Unew, stats, ws) == BAD
    assert low.update_rc(o, None, Uc, Unom, K, Unew, stats, ws) == BAD
    assert low.update_rc(o, J, None, Unom, K, Unew, stats, ws) == BAD
    assert low.update_rc(o, J, Uc, Unom, K, None, stats, ws) == BAD
    assert low.update_rc(o, J, Uc, Unom, K, Unew, None, ws) == BAD
    # a short or missing workspace
    assert low.update_rc(o, J, Uc, Unom, K, Unew, stats, ws, ws_floats=K * B - 1) == WSP
    assert low.update_rc(o, J, Uc, Unom, K, Unew, stats, None) == WSP
    assert low.lib.ac_mppi_workspace_floats(low.ac._handle, K, B, H, C.byref(n)) == 0 and n.value >= K * B
    torch.cuda.synchronize()
    # nothing was launched: outputs untouched, the counter where it was
    assert bool((Unew == 42.0).all()) and bool((stats == 42.0).all()) and bool((Ucx == 42.0).all()) and int(low.it) == 11
    low.it.fill_(0)


# ---- 5. the same bits ----------------------------------------------------------------------------------------------------------------
def test_update_is_reproducible_and_graph_replay_equals_eager(gpu, low):
    torch = low.torch
    from aircraft_amd.control.moving_horizon import quiet_capture

    B, K, H = 3, 300, 3
    Unom = nominal(B, H, seed=10)
    o = make_opts(SIGMA, U_MIN, U_MAX, lam=2.0, seed=SEED)
    Uc, _ = low.sample(o, dev(Unom, gpu), None, K)
    J = dev(random_costs(B, K, 6), gpu)
    a, sa = low.update(o, J, Uc, dev(Unom, gpu), K)
    b, sb = low.update(o, J, Uc, dev(Unom, gpu), K)
    assert torch.equal(a, b) and torch.equal(sa.nan_to_num(), sb.nan_to_num())

    U = dev(Unom, gpu)
    Ucb, Jb = torch.empty((H, 7, K * B), device=gpu), torch.empty((K * B,), device=gpu)
    stats, ws = torch.empty((4, B), device=gpu), torch.empty((K * B,), device=gpu)

    def iteration():  # sample -> a cost computed on the device -> update in place on U
        _lib.check(low.sample_rc(o, U, None, K, Ucb, None))
        torch.sum(Ucb * Ucb, dim=(0, 1), out=Jb)
        _lib.check(low.update_rc(o, Jb, Ucb, U, K, U, stats, ws))

    low.it.fill_(0)
    iteration(); e1 = U.clone()
    iteration(); e2 = U.clone()
    assert int(low.it) == 2
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        iteration()  # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with quiet_capture(g, side):
            iteration()
    torch.cuda.current_stream().wait_stream(side)
    U.copy_(dev(Unom, gpu)); low.it.fill_(0)
    g.replay(); r1 = U.clone()
    g.replay(); r2 = U.clone()
    torch.cuda.synchronize()
    assert torch.equal(r1, e1) and torch.equal(r2, e2) and int(low.it) == 2
    assert not torch.equal(r1, r2)  # the device counter: fresh noise at every replay
    low.it.fill_(0)


# ---- 6. one whole iteration against the oracle -------------------------------------------------------------------------------------------
def goal_setup(model, B, H, seed=3, r=1e-2, trimmed=False):
    """B gliders released near trim from the same point, flying roughly along +x (tests/test_gpu_ilqr.py::setup); the goal is
    2 m to the side of where they would coast to.  trimmed: the glider's trim state at 50 m/s with small velocity and rate
    offsets instead (the default model's explicit step diverges within 20 nodes from the faster release states, in the oracle
    as on the device)."""
    from aircraft_amd.control import ILQR, QuadraticCost

    ac = make_aircraft(model)
    speed = 50.0 if trimmed else 60.0
    cost = QuadraticCost.goal((speed * H * 0.01, 2.0), w_goal=1.0, height=-200.0, w_height=1.0, w_lateral_speed=0.5, r=r, reg=1.0)
    il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost)
    return ac, il, cost, (trim_states(B, seed) if trimmed else release_states(B, seed))


def trim_states(B, seed):
    from aircraft_amd.synthetic import TRIM_STATE

    scale = np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0.02, 0.02, 0.02])[:, None]
    return f32_exact(np.repeat(TRIM_STATE[:, None], B, axis=1) + np.random.default_rng(seed).normal(0, 1, (13, B)) * scale)


def release_states(B, seed):
    from aircraft_amd.synthetic import quat_from_euler, quat_rotate

    rng = np.random.default_rng(seed)
    X0 = np.zeros((13, B))
    X0[2] = -200.0
    V = rng.uniform(50, 65, B); al = np.deg2rad(rng.uniform(-1, 1, B)); be = np.deg2rad(rng.uniform(-1, 1, B))
    vb = np.stack([V * np.cos(al) * np.cos(be), V * np.sin(be), V * np.sin(al) * np.cos(be)])
    q = quat_from_euler(np.deg2rad(rng.uniform(-5, 5, B)), np.deg2rad(rng.uniform(-2, 2, B)), np.deg2rad(rng.uniform(-5, 5, B)))
    X0[3:6] = quat_rotate(q, vb); X0[6:10] = q; X0[10:13] = rng.normal(0, 0.02, (3, B))
    return f32_exact(X0)


@pytest.mark.parametrize("model", ["default", "poly"])
def test_iteration_matches_oracle_chain(gpu, model):
    import ilqr_oracle as io
    from aircraft_amd.control import MPPI

    B, K, H, lam = 4, 64, 20, 0.2
    sigma = [1.0, 1.0, 1.0, 0, 0, 0, 0]
    ac, il, cost, X0 = goal_setup(model, B, H, trimmed=True)
    orc = make_oracle(ac)
    U0 = f32_exact(np.random.default_rng(2).normal(0, 0.3, (H, 7, B)) * (np.arange(7) < 3)[None, :, None])
    m = MPPI(il, samples=K, sigma=sigma, temperature=lam, seed=SEED, accept=False)
    x0, U = dev(X0, gpu), dev(U0, gpu)
    X = il.rollout(x0, U)
    Jn, _ = m.iterate(x0, X, U)
    ws = m._workspace(B, gpu)
    # the float64 chain: reference noise, oracle rollouts, NumPy cost, reference update
    Uc = R.sample(U0, sigma, cost.u_min, cost.u_max, SEED, 0, K)
    Xc = orc.rollout(np.tile(X0, (1, K)), Uc, 0.01)
    Jc = io.cost(cost, Xc, Uc)
    assert np.isfinite(Jc).all()
    lam32 = float(np.float32(lam))
    Unew, stats = R.update(Jc, Uc, U0, K, lam32, cost.u_min, cost.u_max)
    Jg = f64(ws["Jc"])
    dJ = np.abs(Jg - Jc)
    assert dJ.max() <= 1e-5 * np.abs(Jc).max()
    w, _ = R.weights(Jc, K, lam32)
    width = np.float64(cost.u_max) - np.float64(cost.u_min)
    spread = np.abs(Uc.reshape(H, 7, K, B) - Unew[:, :, None, :])
    bound = 1e-5 * width[None, :, None] + 2 * (w[None, None] * spread * dJ.reshape(K, B)[None, None]).sum(axis=2) / lam32
    err = np.abs(f64(U) - Unew)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    assert (err[:, width == 0] == 0).all()
    Xn = orc.rollout(X0, Unew, 0.01)
    parity_report(f"mppi_iteration_{model}", candidate_cost_rel=float(dJ.max() / np.abs(Jc).max()),
                  unew_err_over_width=float((err[:, :3] / width[None, :3, None]).max()),
                  unew_err_over_bound=float((err[:, :3] / bound[:, :3]).max()), ess_min=float(stats[1].min()),
                  ess_max=float(stats[1].max()))
    assert np.abs(f64(m.last_stats)[1] - stats[1]).max() <= 1e-2 * stats[1].max()  # (ESS moves with dJ / lambda)
    assert np.array_equal(f64(m.last_stats)[2], stats[2])
    assert np.abs(f64(Jn) - io.cost(cost, Xn, Unew)).max() <= 1e-4 * np.abs(Jc).max()
    assert int(m.iteration) == 1


# ---- 7. the class ------------------------------------------------------------------------------------------------------------------------
def test_iterate_equals_the_low_level_chain(gpu):
    import torch
    from aircraft_amd.control import MPPI

    B, K, H = 5, 48, 12
    ac, il, cost, X0 = goal_setup("poly", B, H)
    for accept in (False, True):
        m = MPPI(il, samples=K, sigma=(1, 1, 1, 0, 0, 0, 0), temperature=0.2, seed=5, accept=accept)
        x0 = dev(X0, gpu)
        U = torch.zeros((H, 7, B), device=gpu)
        X = il.rollout(x0, U)
        Xs, Us = X.clone(), U.clone()
        J, imp = m.iterate(x0, X, U)
        J, imp = J.clone(), imp.clone()
        m.set_iteration(0)
        Uc, X0c = m.sample(Us, x0)
        Xc = il.rollout(X0c, Uc)
        Jc = il.trajectory_cost(Xc, Uc)
        Un, stats = m.update(Jc, Uc, Us)
        Xn = il.rollout(x0, Un)
        Jn = il.trajectory_cost(Xn, Un)
        J0 = il.trajectory_cost(Xs, Us)
        if accept:
            take = Jn < J0
            assert torch.equal(imp, take) and take.any()
            assert torch.equal(U, torch.where(take[None, None], Un, Us)) and torch.equal(X, torch.where(take[None, None], Xn, Xs))
            assert torch.equal(J, torch.where(take, Jn, J0))
        else:
            assert torch.equal(U, Un) and torch.equal(X, Xn) and torch.equal(J, Jn) and bool(imp.all())
        assert torch.equal(m.last_stats, stats)


def straight_track_problem(B, H):
    from aircraft_amd.control import MHTT, MHTTWeights, Track

    ac = make_aircraft("poly")
    P = np.stack([np.linspace(0.0, 150.0, 31), np.zeros(31), np.full(31, -200.0)], axis=1)
    mh = MHTT(system=ac, track=Track(P), dt=0.01, num_nodes=H, weights=MHTTWeights(w_control=0.01))
    rng = np.random.default_rng(5)
    X0 = release_states(B, seed=5)
    X0[0] = rng.uniform(-1, 3, B); X0[1] = rng.uniform(-3, 3, B); X0[2] = -200.0 + rng.uniform(-2, 2, B)
    return ac, mh, f32_exact(X0), f32_exact(rng.uniform(0.0, 0.02, B))


@pytest.mark.parametrize("problem", ["ilqr", "goal", "mhtt"])
def test_solve_descends_from_zero_controls(gpu, problem):
    """5 iterations at B = 8, K = 256, H = 20 from zero controls: the history never increases (accept = True) and every instance
    ends below its start.  White control noise is scored by each loss's actuation terms, so the problems weigh them lightly
    (r = 1e-2; w_rate = 1 with eps_rate = 1 deg^2; w_control = 0.01) and the temperature is of the order of the candidates'
    cost spread."""
    import torch
    from aircraft_amd.control import MPPI, GoalAcquisition

    B, K, H = 8, 256, 20
    if problem == "ilqr":
        ac, prob, cost, X0 = goal_setup("poly", B, H)
        m = MPPI(prob, samples=K, sigma=(1, 1, 1, 0, 0, 0, 0), temperature=0.2, seed=1)
    elif problem == "goal":
        ac = make_aircraft("poly", normalise=True)
        X0 = release_states(B, seed=3)
        rng = np.random.default_rng(4)
        goal = f32_exact(np.stack([np.linalg.norm(X0[3:6], axis=0) * H * 0.01, rng.uniform(-2, 2, B)]))
        prob = GoalAcquisition(system=ac, goal=goal, dt=0.01, num_nodes=H, w_rate=1.0, eps_rate=1.0, w_al=0.0)
        m = MPPI(prob, samples=K, sigma=(0.5, 0.5, 0.5, 0, 0, 0, 0), temperature=100.0, seed=1)
    else:
        ac, prob, X0, s0 = straight_track_problem(B, H)
        prob.set_progress(s0)
        m = MPPI(prob, samples=K, sigma=(1, 1, 1, 0, 0, 0, 0), temperature=1.0, seed=1)
    X, U, hist = m.solve(dev(X0, gpu), torch.zeros((H, 7, B), device=gpu), iters=5)
    h = f64(hist)
    print(problem, "start", h[0].round(4), "end", h[-1].round(4), "ESS", f64(m.last_stats)[1].round(1))
    assert h.shape == (6, B) and np.isfinite(h).all() and torch.isfinite(X).all()
    assert (np.diff(h, axis=0) <= 0).all()
    assert (h[-1] < h[0]).all()
    assert int(m.iteration) == 5
    lo, hi = torch.tensor(prob.cost.u_min, device=gpu)[None, :, None], torch.tensor(prob.cost.u_max, device=gpu)[None, :, None]
    assert bool((U >= lo).all()) and bool((U <= hi).all())
    assert torch.equal(X, prob.rollout(dev(X0, gpu), U))  # the accepted pair is consistent


def test_receding_horizon_eager_equals_graph(gpu):
    import torch
    from aircraft_amd.control import MPPI, RecedingHorizon

    B, K, H = 8, 64, 20
    ac, il, cost, X0 = goal_setup("poly", B, H)
    m = MPPI(il, samples=K, sigma=(1, 1, 1, 0, 0, 0, 0), temperature=0.2, seed=9)
    x0, U0 = dev(X0, gpu), torch.zeros((H, 7, B), device=gpu)
    eager = RecedingHorizon(m, overlap=12, iterations=1).allocate(x0, U0)
    he = eager.run(3, record=True)
    assert int(m.iteration) == 3
    m.set_iteration(0)
    graph = RecedingHorizon(m, overlap=12, iterations=1).allocate(x0, U0).capture()
    m.set_iteration(0)  # (the warm-up cycle of capture() advanced it)
    hg = graph.run(3, record=True)
    torch.cuda.synchronize()
    assert he.shape == (3 * 8 + 1, 13, B) and torch.isfinite(he).all()
    assert torch.equal(he, hg) and torch.equal(eager.x0, graph.x0) and torch.equal(eager.U, graph.U) and torch.equal(eager.cost, graph.cost)
    assert int(m.iteration) == 3 and bool((graph.U != 0).any())


# ---- 8. the example ------------------------------------------------------------------------------------------------------------------------
def test_example_prints_its_json_line(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mppi_goal.py"), "--batch", "8", "--samples", "64",
                        "--horizon", "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["batch"] == 8 and out["samples"] == 64 and out["horizon"] == 20
    assert len(out["mean_cost"]) == out["iters"] + 1 and len(out["effective_sample_size"]) == out["iters"] == len(out["ms_per_iteration"])
    assert all(np.isfinite(v) for v in out["mean_cost"]) and out["mean_cost"][-1] <= out["mean_cost"][0]
    assert all(1.0 <= e <= 64.0 * (1 + 1e-5) for e in out["effective_sample_size"])
