"""GPU tests of the airframe gradients (ac_step_agrad_f32, ac_rollout_agrad_f32) and of
aircraft_amd.autodiff.AirframeParameters.

Reference and metrics: tests/agrad_ref.py — float64 central differences through the oracle over the eight physical numbers at
their float32 rounding; summed gradients per group against the scale S = sum over units of |per-unit reference| (bar 2e-5), single
units per group against the group's largest entry (bar 1e-4); every case first asserts that the references at h_rel = 1e-5 and
3e-5 agree.  The references are computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import agrad_ref as R
from tests.helpers import f32_exact, make_aircraft, parity_report, synthetic_units

pytestmark = pytest.mark.gpu

DT = 0.01


def roll_dt(model):
    """dt of a chained rollout.  The default model is unstable under RK4 at dt = 0.01: on the rollout problems of these tests (and
    on near-trim ones) its float64 trajectory reaches 1e4 after three steps and overflows within six, so its rollouts run at
    dt = 1e-3, where |omega| stays below 0.7 rad/s.  Single steps keep dt = 0.01."""
    return 1e-3 if model == "default" else DT


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def grads_through_params(params, loss_of):
    """the gradient over (mass, Ixx, Iyy, Izz, Ixz, com) that autograd leaves in an AirframeParameters"""
    for p in params.parameters():
        p.grad = None
    loss_of().backward()
    return np.concatenate([host(p.grad).reshape(-1) for p in (params.mass, params.inertia, params.com)])


# ---- 1. step gradient through autodiff.step(..., params=) against central differences --------------------------------------------
STEP_CASES = {  # name -> (model, sub-steps, dt)
    "default": ("default", 1, DT),
    "linear": ("linear", 1, DT),
    "poly": ("poly", 1, DT),
    "poly_sub10": ("poly", 10, 0.1),
}
POOLS = {1: (65, 5), 63: (65, 5), 64: (65, 5), 65: (65, 5), 130: (130, 7), 300: (300, 9), 4099: (4099, 11)}  # n -> (pool, seed)
_STEP_REF = {}


def step_reference(case, n):
    """(units of the pool, dt, per-unit references), once per (case, pool); n = 130 carries per-unit dt"""
    pool, seed = POOLS[n]
    key = (case, pool, seed)
    if key not in _STEP_REF:
        model, ns, dt = STEP_CASES[case]
        X, U, lam = R.units(pool, seed)
        if pool == 130 and ns == 1:
            dt = f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, pool))
        _STEP_REF[key] = (X, U, lam, dt, R.step_reference(R.aircraft(model, substeps=ns), X, U, dt, lam))
    return _STEP_REF[key]


def step_case(gpu, case, n, grid=None):
    """-> (gradient over the eight numbers through autodiff, errors per group, the aircraft, the per-unit reference)"""
    from aircraft_amd import autodiff

    model, ns, _ = STEP_CASES[case]
    X, U, lam, dt, refs = step_reference(case, n)
    ref, agree = R.check_reference(refs, n)  # (the float64 oracle alone, before the code under test)
    ac = R.aircraft(model, substeps=ns)
    if grid is not None:
        ac.set_coef_grad_grid(grid)
    X, U, lam = X[:, :n], U[:, :n], lam[:, :n]
    dtd = dev(dt[:n], gpu) if np.ndim(dt) else dt
    params = autodiff.AirframeParameters(ac)
    got = grads_through_params(params, lambda: (autodiff.step(ac, dev(X, gpu), dev(U, gpu), dtd, params=params) * dev(lam, gpu)).sum())
    assert ac.last_launch()[0] == "k_step_agrad"
    errs = R.summed_errors(got, ref)
    print(f"[agrad step] {case} n={n} grid={ac.last_launch()[1]} errs {errs} reference agreement {agree}")
    parity_report("step_agrad", case=case, n=n, grid=ac.last_launch()[1], worst_group=max(errs.values()), per_group=errs,
                  reference_agreement=agree)
    return got, errs, ac, ref


@pytest.mark.parametrize("model,n", [(m, n) for m in ("default", "linear", "poly") for n in (1, 63, 64, 65, 130)] + [("poly", 4099)])
def test_step_airframe_grad_matches_central_differences(gpu, model, n):
    _, errs, _, _ = step_case(gpu, model, n)
    assert max(errs.values()) <= R.BAR_SUM, errs


@pytest.mark.parametrize("n", [1, 65])
def test_step_airframe_grad_ten_substeps(gpu, n):
    _, errs, ac, _ = step_case(gpu, "poly_sub10", n)
    assert ac.last_launch()[3] == (22 + 30 + 130) * 64 * 4  # accumulators, stage words, ten sub-step inputs
    assert max(errs.values()) <= R.BAR_SUM, errs


@pytest.mark.parametrize("model", ["default", "linear", "poly"])
def test_single_units(gpu, model):
    """the first 16 units of the seed-5 pool, each as a call of its own: no cancellation across units"""
    X, U, lam, dt, refs = step_reference(model, 65)
    ac = R.aircraft(model)
    worst = {}
    for k in range(16):
        ref, _ = R.check_reference([r[:, k:k + 1] for r in refs], bar=R.H_AGREE_UNIT)
        phi = ac.step_airframe_grad(dev(X[:, k:k + 1], gpu), dev(U[:, k:k + 1], gpu), dt, dev(lam[:, k:k + 1], gpu),
                                    need=(False, False, False))[0]
        errs = R.unit_errors(R.chain(ac, host(phi)), ref[:, 0])
        worst = {g: max(e, worst.get(g, 0.0)) for g, e in errs.items()}
    print(f"[agrad single units] {model} worst of 16 {worst}")
    parity_report("step_agrad_single_units", case=model, worst_group=max(worst.values()), per_group=worst)
    assert max(worst.values()) < R.BAR_UNIT, worst


# ---- 2. the persistent loop and a ragged tail ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["default", "poly"])
def test_step_airframe_grad_persistent_loop_and_ragged_tail(gpu, model):
    n = 300  # five tiles, the last of 44 units
    g_auto, e_auto, ac_auto, ref = step_case(gpu, model, n)
    assert ac_auto.last_launch()[1] == 5
    g_two, e_two, ac_two, _ = step_case(gpu, model, n, grid=2)
    assert ac_two.last_launch()[1] == 2
    assert max(e_auto.values()) <= R.BAR_SUM and max(e_two.values()) <= R.BAR_SUM, (e_auto, e_two)
    scale = np.abs(ref).sum(axis=1)
    for g, s in R.GROUPS.items():
        assert np.abs(g_auto[s] - g_two[s]).max() <= 1e-6 * scale[s].max(), g


# ---- 3. rollout --------------------------------------------------------------------------------------------------------------------
_ROLL_REF = {}


def rollout_reference(model, B, H):
    if (model, B, H) not in _ROLL_REF:
        X0, U, G = R.rollout_problem(B, H)
        _ROLL_REF[(model, B, H)] = (X0, U, G, R.rollout_reference(R.aircraft(model), X0, U, roll_dt(model), G))
    return _ROLL_REF[(model, B, H)]


def rollout_case(gpu, B, H, grid=None):
    """-> (errors per group of the rollout gradient through autodiff, the aircraft)"""
    from aircraft_amd import autodiff

    X0, U, G, refs = rollout_reference("poly", B, H)
    ref, agree = R.check_reference(refs)
    ac = R.aircraft("poly")
    if grid is not None:
        ac.set_coef_grad_grid(grid)
    params = autodiff.AirframeParameters(ac)
    got = grads_through_params(params, lambda: (autodiff.rollout(ac, dev(X0, gpu), dev(U, gpu), DT, params=params) * dev(G, gpu)).sum())
    assert ac.last_launch()[0] == "k_rollout_agrad"
    errs = R.summed_errors(got, ref)
    print(f"[agrad rollout] poly B={B} H={H} grid={ac.last_launch()[1]} errs {errs} reference agreement {agree}")
    parity_report("rollout_agrad", case="poly", B=B, H=H, grid=ac.last_launch()[1], worst_group=max(errs.values()), per_group=errs,
                  reference_agreement=agree)
    return errs, ac


@pytest.mark.parametrize("B", [1, 65])
def test_rollout_airframe_grad_matches_central_differences(gpu, B):
    errs, _ = rollout_case(gpu, B, 12)
    assert max(errs.values()) <= R.BAR_SUM, errs


def test_rollout_airframe_grad_persistent_loop_and_ragged_tail(gpu):
    errs, ac = rollout_case(gpu, 70, 3, grid=1)  # one workgroup over two tiles, the second of 6 instances
    assert ac.last_launch()[1] == 1
    assert max(errs.values()) <= R.BAR_SUM, errs


def test_rollout_airframe_grad_zero_horizon(gpu):
    """H = 0: X[0] = x0, no step and no airframe constant enters — G[0] passes through, everything else is zero."""
    import torch

    ac = R.aircraft("default")
    X = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    G = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    phi, x0b, ub, db = ac.rollout_airframe_grad(X, torch.zeros((0, 7, 70), device=gpu), DT, G, out=torch.ones(22, device=gpu))
    assert not phi.any() and torch.equal(x0b, G[0]) and ub.shape == (0, ac.num_controls, 70) and not db.any()


@pytest.mark.parametrize("model", ["default", "poly"])
def test_rollout_airframe_grad_is_the_sum_of_its_steps(gpu, model):
    """Structural: lambda_{k+1} rebuilt on the saved nodes with the existing step_vjp (lambda_H = G_H, lambda_k = G_k + Xbar_k);
    the rollout gradient equals the step gradient over the B H units (X_k, U_k, lambda_{k+1}) to 1e-6 of the scale (the two
    differ in the order of their sums only).  Scale: per group, the sum over instances of |per-instance reference|."""
    import torch

    B, H, dt = 65, 6, roll_dt(model)
    X0, U, G, refs = rollout_reference(model, B, H)
    scale = np.abs(R.check_reference(refs)[0]).sum(axis=1)
    ac = R.aircraft(model)
    Ud, Gd = dev(U, gpu), dev(G, gpu)
    Xtraj = ac.rollout(dev(X0, gpu), Ud, dt)
    assert bool(torch.isfinite(Xtraj).all())
    lam = [None] * (H + 1)
    lam[H] = Gd[H]
    for k in range(H - 1, -1, -1):
        xb, _, _ = ac.step_vjp(Xtraj[k], Ud[k], dt, lam[k + 1])
        lam[k] = Gd[k] + xb
    got, x0b, _, _ = ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd)
    assert torch.equal(x0b, lam[0])  # lambda_0 of the two chains
    Xu = Xtraj[:H].permute(1, 0, 2).reshape(13, H * B)
    Uu = Ud.permute(1, 0, 2).reshape(7, H * B)
    Lu = torch.stack(lam[1:]).permute(1, 0, 2).reshape(13, H * B)
    want = ac.step_airframe_grad(Xu, Uu, dt, Lu, need=(False, False, False))[0]
    diff = np.abs(R.chain(ac, host(got)) - R.chain(ac, host(want)))
    errs = {g: float(diff[s].max() / scale[s].max()) for g, s in R.GROUPS.items()}
    print(f"[agrad rollout = sum of steps] {model} B={B} H={H} errs {errs}")
    parity_report("rollout_agrad_structural", case=model, B=B, H=H, worst_group=max(errs.values()), per_group=errs)
    assert max(errs.values()) <= 1e-6, errs


# ---- 4. the other outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,substeps", [("default", 1), ("linear", 1), ("poly", 1), ("poly", 10)])
def test_other_outputs_equal_the_plain_vjp(gpu, model, substeps):
    import torch

    ac = R.aircraft(model, substeps=substeps)
    n = 130
    X, U, lam = R.units(n, 7)
    dts = dev(f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, n)), gpu)
    args = (dev(X, gpu), dev(U, gpu), dts, dev(lam, gpu))
    _, xb, ub, db = ac.step_airframe_grad(*args)
    xp, up, dp = ac.step_vjp(*args)
    assert ac.last_launch()[0] == "k_step_vjp"  # the fused route
    assert torch.equal(xb, xp) and torch.equal(ub, up) and torch.equal(db, dp)
    B, H = 65, 6
    X0, Ur, G = R.rollout_problem(B, H)
    Ud, Gd = dev(Ur, gpu), dev(G, gpu)
    dt = roll_dt(model)
    Xtraj = ac.rollout(dev(X0, gpu), Ud, dt)
    assert bool(torch.isfinite(Xtraj).all())
    _, x0b, urb, drb = ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd)
    x0p, urp, drp = ac.rollout_vjp(Xtraj, Ud, dt, Gd)
    assert ac.last_launch()[0] == "k_rollout_vjp"
    assert torch.equal(x0b, x0p) and torch.equal(urb, urp) and torch.equal(drb, drp)


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["default", "poly"])
def test_repeats_bit_identical_and_graph_capture(gpu, model):
    import torch

    ac = R.aircraft(model)
    B, H, dt = 300, 4, roll_dt(model)
    X0, U0 = synthetic_units(B, seed=81, flaps=True)
    Ud = dev(np.repeat(f32_exact(U0)[None], H, axis=0), gpu)
    Xtraj = ac.rollout(dev(f32_exact(X0), gpu), Ud, dt)
    assert bool(torch.isfinite(Xtraj).all())
    Gd = torch.randn(Xtraj.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    ref = ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd)[0]
    assert tuple(ref.shape) == (22,) and bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert torch.equal(ref, ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd)[0])
    # NULL x0 / U / dt outputs: the same sweep, the same airframe gradient
    assert torch.equal(ref, ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd, need=(False, False, False))[0])
    x, u, lam = Xtraj[1], Ud[1], Gd[2]
    ref_s = ac.step_airframe_grad(x, u, dt, lam)[0]
    assert torch.equal(ref_s, ac.step_airframe_grad(x, u, dt, lam)[0])
    assert torch.equal(ref_s, ac.step_airframe_grad(x, u, dt, lam, need=(False, False, False))[0])
    ws = ac.airframe_grad_workspace("rollout", B, H)  # allocated before the capture
    out = torch.empty_like(ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd, ws=ws, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ac.rollout_airframe_grad(Xtraj, Ud, dt, Gd, ws=ws, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ref, out)


# ---- 6. coefficients and airframe together -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["linear", "poly"])
def test_tuple_of_coefficient_and_airframe_parameters(gpu, model):
    import torch

    from aircraft_amd import autodiff

    ac = R.aircraft(model)
    X, U, lam = R.units(130, 7)
    X0, Ur, G = R.rollout_problem(65, 4)
    coef, frame = autodiff.CoefficientParameters(ac), autodiff.AirframeParameters(ac)

    def run(params, rollout):
        for p in list(coef.parameters()) + list(frame.parameters()):
            p.grad = None
        x = dev(X0 if rollout else X, gpu).requires_grad_(True)
        if rollout:
            (autodiff.rollout(ac, x, dev(Ur, gpu), DT, params=params) * dev(G, gpu)).sum().backward()
        else:
            (autodiff.step(ac, x, dev(U, gpu), DT, params=params) * dev(lam, gpu)).sum().backward()
        return ([None if p.grad is None else p.grad.clone() for p in coef.parameters()],
                [None if p.grad is None else p.grad.clone() for p in frame.parameters()], x.grad.clone())

    for rollout in (False, True):
        c_both, a_both, x_both = run((coef, frame), rollout)
        assert ac.last_launch()[0] == ("k_rollout_agrad" if rollout else "k_step_agrad")  # the second of the two sweeps
        c_only, a_none, x_c = run(coef, rollout)
        c_none, a_only, x_a = run(frame, rollout)
        assert all(g is None for g in a_none) and all(g is None for g in c_none)
        assert all(torch.equal(a, b) for a, b in zip(c_both, c_only))
        assert all(torch.equal(a, b) for a, b in zip(a_both, a_only))
        assert torch.equal(x_both, x_c) and torch.equal(x_both, x_a)


# ---- 7. the parameters take effect -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["default", "poly"])
def test_updated_parameters_are_what_the_aircraft_runs(gpu, model):
    import torch

    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, autodiff
    from aircraft_amd.synthetic import GLIDER
    from tests.helpers import model_path

    ac = R.aircraft(model)
    X, U, lam = R.units(96, 71)
    params = autodiff.AirframeParameters(ac)
    y0 = autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params)
    (y0 * dev(lam, gpu)).sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in params.parameters())
    torch.optim.Adam(params.parameters(), lr=1e-3).step()
    y1 = autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params).detach()
    assert not torch.equal(y0.detach(), y1)
    m, (ixx, iyy, izz, ixz), com = float(params.mass.detach()), (float(v) for v in params.inertia.detach()), host(params.com)
    assert (ac.mass, ac.Ixx, ac.Iyy, ac.Izz, ac.Ixz) == (m, ixx, iyy, izz, ixz) and np.array_equal(ac.com, com)
    cfg = dict(GLIDER, mass=m, Ixx=ixx, Iyy=iyy, Izz=izz, Ixz=ixz, aero_centre_offset=[float(v) for v in com])
    fresh = Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=model_path(model), aircraft_config=AircraftConfiguration(cfg),
                                  physical_integration_substeps=1))
    fresh.normalise = True
    assert torch.equal(y1, fresh.state_update(dev(X, gpu), dev(U, gpu), DT))
    assert torch.equal(y1, ac.state_update(dev(X, gpu), dev(U, gpu), DT))  # the aircraft itself now runs the new constants


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import warnings

    import torch

    from aircraft_amd import AircraftHipError, Quadrotor, _lib, autodiff

    X, U, lam = R.units(8, 91)
    args = (dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    nn = make_aircraft("nn", normalise=True)
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*MLP surrogate"):
        nn.step_airframe_grad(*args)
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*MLP surrogate"):
        nn.airframe_grad_workspace("step", 8)
    quad = Quadrotor()
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*quadrotor"):
        quad.step_airframe_grad(args[0], dev(U[:4], gpu), DT, args[3])
    for other in (nn, quad):
        with pytest.raises(ValueError, match="AirframeParameters"):
            autodiff.AirframeParameters(other)
    # sub-steps: 40 run, 41 are refused with the limit in the text
    assert bool(torch.isfinite(R.aircraft("poly", substeps=40).step_airframe_grad(args[0], args[1], 0.1, args[3])[0]).all())
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*40 RK4 sub-steps"):
        R.aircraft("poly", substeps=41).step_airframe_grad(args[0], args[1], 0.1, args[3])
    # a short workspace
    poly = R.aircraft("poly")
    ws = poly.airframe_grad_workspace("step", 8)
    assert ws.numel() == 22
    out = torch.empty(22, device=gpu)
    lib = _lib.load()
    rc = lib.ac_step_agrad_f32(poly._handle, args[0].data_ptr(), args[1].data_ptr(), C.c_float(DT), None, 8, args[3].data_ptr(),
                               None, None, None, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == -6 and b"workspace" in lib.ac_last_error()
    with pytest.raises(AircraftHipError, match="AC_ERR_WORKSPACE"):
        poly.rollout_airframe_grad(torch.zeros((3, 13, 8), device=gpu), torch.zeros((2, 7, 8), device=gpu), DT,
                                   torch.zeros((3, 13, 8), device=gpu), ws=torch.empty(16, device=gpu))
    # the routes that existed before stay closed
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*MLP surrogate"):
        poly.step_wgrad(*args)
    with pytest.raises(TypeError, match="params"):
        autodiff.step(poly, args[0], args[1], DT, params=object())
    # a non-positive mass is refused, and the aircraft keeps flying on the last installed constants
    params = autodiff.AirframeParameters(poly)
    y0 = autodiff.step(poly, args[0], args[1], DT, params=params).detach()
    mass0 = float(params.mass)
    with torch.no_grad():
        params.mass.fill_(0.0)
    with pytest.raises(ValueError, match="mass"):
        autodiff.step(poly, args[0], args[1], DT, params=params)
    assert torch.equal(y0, poly.state_update(args[0], args[1], DT))
    # changed constants cannot be installed while a stream is capturing
    with torch.no_grad():
        params.mass.fill_(mass0 * 1.01)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns that the abandoned capture recorded nothing)
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g, stream=s):
                autodiff.step(poly, args[0], args[1], DT, params=params)
    torch.cuda.synchronize()


# ---- 9. the example at a small size ------------------------------------------------------------------------------------------------
def test_fit_airframe_example_reduces_the_loss(gpu):
    import importlib.util
    import os

    from tests.helpers import ROOT

    spec = importlib.util.spec_from_file_location("fit_airframe", os.path.join(ROOT, "examples", "fit_airframe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, rel = mod.main(["--batch", "64", "--horizon", "5", "--iters", "40"])
    assert len(losses) == 40 and np.all(np.isfinite(losses)) and np.all(np.isfinite(rel))
    print(f"[agrad example] loss {losses[0]:.3e} -> {losses[-1]:.3e}, relative errors {rel[0]} -> {rel[-1]}")
    assert losses[-1] < losses[0]  # (the relative errors are reported: weakly identified numbers need not close in 40 iterations)
