"""GPU tests of the coefficient gradients of the cubic-fit and the linear model (ac_step_cgrad_f32, ac_rollout_cgrad_f32;
DESIGN.md §4.10) and of aircraft_amd.autodiff.CoefficientParameters.

Reference (tests/cgrad_ref.py): float64 central differences through the oracle at the float32 rounding of the model data,
h = 1e-5 max(|theta_i|, 0.05); every case first asserts that the references at 1e-5 and 3e-5 agree to 1e-6 per tensor.
Error per tensor: max|g - g_ref| / max|g_ref|; bar 2e-5.  The references are computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest

from tests import cgrad_ref as R
from tests.helpers import f32_exact, make_aircraft, parity_report, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

DT = 0.01


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make(model, **kw):
    return make_aircraft(model, normalise=True, **kw)


def grads_through_params(params, loss_of):
    for p in params.parameters():
        p.grad = None
    loss_of().backward()
    return {k: host(p.grad) for k, p in params.named_parameters()}


# ---- 1. step gradient through autodiff.step(..., params=) against central differences --------------------------------------------
STEP_CASES = {  # name -> (model, sub-steps, dt)
    "poly": ("poly", 1, DT),
    "linear": ("linear", 1, DT),
    "poly_sub10": ("poly", 10, 0.1),
}
POOLS = {1: (1, 5), 63: (65, 5), 64: (65, 5), 65: (65, 5), 130: (130, 7), 300: (300, 9), 4099: (4099, 11)}  # n -> (pool, seed)
_STEP_REF = {}


def step_reference(case, n):
    """(aircraft arguments, units of the pool, dt, per-unit references), once per (case, pool); n = 130 carries per-unit dt"""
    pool, seed = POOLS[n]
    key = (case, pool, seed)
    if key not in _STEP_REF:
        model, ns, dt = STEP_CASES[case]
        ac = make(model, substeps=ns)
        X, U, lam = R.units(pool, seed)
        if pool == 130 and ns == 1:
            dt = f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, pool))
        _STEP_REF[key] = (X, U, lam, dt, R.step_reference(ac, X, U, dt, lam))
    return _STEP_REF[key]


def step_case(gpu, case, n, grid=None):
    """-> (gradients through autodiff, errors per tensor, the aircraft)"""
    from aircraft_amd import autodiff

    model, ns, _ = STEP_CASES[case]
    X, U, lam, dt, refs = step_reference(case, n)
    want, agree = R.check_reference([R.summed(r, n) for r in refs])  # (the float64 oracle alone, before the code under test)
    ac = make(model, substeps=ns)
    if grid is not None:
        ac.set_coef_grad_grid(grid)
    X, U, lam = X[:, :n], U[:, :n], lam[:, :n]
    dtd = dev(dt[:n], gpu) if np.ndim(dt) else dt
    params = autodiff.CoefficientParameters(ac)
    got = grads_through_params(params, lambda: (autodiff.step(ac, dev(X, gpu), dev(U, gpu), dtd, params=params) * dev(lam, gpu)).sum())
    assert ac.last_launch()[0] == "k_step_cgrad"
    errs = R.tensor_errors(got, want)
    print(f"[cgrad step] {case} n={n} grid={ac.last_launch()[1]} errs {errs} reference agreement {agree}")
    parity_report("step_cgrad", case=case, n=n, grid=ac.last_launch()[1], worst_tensor_rel=max(errs.values()), per_tensor=errs,
                  reference_agreement=agree)
    return got, errs, ac


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 4099])
@pytest.mark.parametrize("model", ["poly", "linear"])
def test_step_coef_grad_matches_central_differences(gpu, model, n):
    _, errs, _ = step_case(gpu, model, n)
    assert max(errs.values()) < R.BAR, errs


@pytest.mark.parametrize("n", [1, 65, 130])
def test_step_coef_grad_ten_substeps(gpu, n):
    _, errs, ac = step_case(gpu, "poly_sub10", n)
    assert ac.last_launch()[3] == (210 + 30 + 130) * 64 * 4  # accumulators, stage words, ten sub-step inputs
    assert max(errs.values()) < R.BAR, errs


# ---- 2. the persistent loop and a ragged tail ------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["poly", "linear"])
def test_step_coef_grad_persistent_loop_and_ragged_tail(gpu, model):
    n = 300  # five tiles, the last of 44 units
    g_auto, e_auto, ac_auto = step_case(gpu, model, n)
    assert ac_auto.last_launch()[1] == 5
    g_two, e_two, ac_two = step_case(gpu, model, n, grid=2)
    assert ac_two.last_launch()[1] == 2
    assert max(e_auto.values()) < R.BAR and max(e_two.values()) < R.BAR, (e_auto, e_two)
    for k in g_auto:
        assert np.abs(g_auto[k] - g_two[k]).max() <= 1e-6 * np.abs(g_auto[k]).max(), k


# ---- 3. rollout --------------------------------------------------------------------------------------------------------------------
_ROLL_REF = {}


def rollout_reference(B, H):
    if (B, H) not in _ROLL_REF:
        X0, U, G = R.rollout_problem(B, H)
        _ROLL_REF[(B, H)] = (X0, U, G, R.rollout_reference(make("poly"), X0, U, DT, G))
    return _ROLL_REF[(B, H)]


def rollout_case(gpu, B, H, grid=None):
    """-> (errors per tensor of the rollout gradient through autodiff, the aircraft)"""
    from aircraft_amd import autodiff

    X0, U, G, refs = rollout_reference(B, H)
    want, agree = R.check_reference([R.summed(r) for r in refs])
    ac = make("poly")
    if grid is not None:
        ac.set_coef_grad_grid(grid)
    params = autodiff.CoefficientParameters(ac)
    got = grads_through_params(params, lambda: (autodiff.rollout(ac, dev(X0, gpu), dev(U, gpu), DT, params=params) * dev(G, gpu)).sum())
    assert ac.last_launch()[0] == "k_rollout_cgrad"
    errs = R.tensor_errors(got, want)
    print(f"[cgrad rollout] poly B={B} H={H} grid={ac.last_launch()[1]} errs {errs} reference agreement {agree}")
    parity_report("rollout_cgrad", case="poly", B=B, H=H, grid=ac.last_launch()[1], worst_tensor_rel=max(errs.values()),
                  per_tensor=errs, reference_agreement=agree)
    return errs, ac


@pytest.mark.parametrize("B", [1, 65])
def test_rollout_coef_grad_matches_central_differences(gpu, B):
    errs, _ = rollout_case(gpu, B, 12)
    assert max(errs.values()) < R.BAR, errs


def test_rollout_coef_grad_persistent_loop_and_ragged_tail(gpu):
    errs, ac = rollout_case(gpu, 70, 3, grid=1)  # one workgroup over two tiles, the second of 6 instances
    assert ac.last_launch()[1] == 1
    assert max(errs.values()) < R.BAR, errs


def test_rollout_coef_grad_zero_horizon(gpu):
    """H = 0: X[0] = x0, no step and no coefficient enters — G[0] passes through, everything else is zero."""
    import torch

    ac = make("poly")
    X = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(3))
    G = torch.randn((1, 13, 70), device=gpu, generator=torch.Generator(device=gpu).manual_seed(4))
    th, x0b, ub, db = ac.rollout_coef_grad(X, torch.zeros((0, 7, 70), device=gpu), DT, G, out=torch.ones(210, device=gpu))
    assert not th.any() and torch.equal(x0b, G[0]) and ub.shape == (0, ac.num_controls, 70) and not db.any()


@pytest.mark.parametrize("model,H", [("linear", 6), ("poly", 6)])
def test_rollout_coef_grad_is_the_sum_of_its_steps(gpu, model, H):
    """Structural: lambda_{k+1} rebuilt on the saved nodes with the existing step_vjp (lambda_H = G_H, lambda_k = G_k + Xbar_k);
    the rollout gradient equals the step gradient over the B H units (X_k, U_k, lambda_{k+1})."""
    import torch

    B = 65
    X0, U, G = R.rollout_problem(B, H)
    ac = make(model)
    Ud, Gd = dev(U, gpu), dev(G, gpu)
    Xtraj = ac.rollout(dev(X0, gpu), Ud, DT)
    assert bool(torch.isfinite(Xtraj).all())
    lam = [None] * (H + 1)
    lam[H] = Gd[H]
    for k in range(H - 1, -1, -1):
        xb, _, _ = ac.step_vjp(Xtraj[k], Ud[k], DT, lam[k + 1])
        lam[k] = Gd[k] + xb
    got, x0b, _, _ = ac.rollout_coef_grad(Xtraj, Ud, DT, Gd)
    Xu = Xtraj[:H].permute(1, 0, 2).reshape(13, H * B)
    Uu = Ud.permute(1, 0, 2).reshape(7, H * B)
    Lu = torch.stack(lam[1:]).permute(1, 0, 2).reshape(13, H * B)
    want, _, _, _ = ac.step_coef_grad(Xu, Uu, DT, Lu, need=(False, False, False))
    errs = R.tensor_errors(R.split_theta(model, host(got)), R.split_theta(model, host(want)))
    x0_dev = float(unit_max_rel(host(x0b), host(lam[0])).max())  # (reported: lambda_0 of the two chains)
    print(f"[cgrad rollout = sum of steps] {model} B={B} H={H} errs {errs} x0_bar against the step chain {x0_dev:.2e}")
    parity_report("rollout_cgrad_structural", case=model, B=B, H=H, worst_tensor_rel=max(errs.values()), per_tensor=errs,
                  x0bar_against_step_chain=x0_dev)
    assert max(errs.values()) < R.BAR, errs


# ---- 4. the other outputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,substeps", [("poly", 1), ("linear", 1), ("poly", 10)])
def test_other_outputs_equal_the_plain_vjp(gpu, model, substeps):
    import torch

    ac = make(model, substeps=substeps)
    n = 130
    X, U, lam = R.units(n, 7)
    dts = dev(f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, n)), gpu)
    args = (dev(X, gpu), dev(U, gpu), dts, dev(lam, gpu))
    _, xb, ub, db = ac.step_coef_grad(*args)
    xp, up, dp = ac.step_vjp(*args)
    assert ac.last_launch()[0] == "k_step_vjp"
    same = all(torch.equal(a, b) for a, b in ((xb, xp), (ub, up), (db, dp)))
    got, want = np.concatenate([host(xb), host(ub), host(db)[None]]), np.concatenate([host(xp), host(up), host(dp)[None]])
    worst = float(unit_max_rel(got, want).max())
    B, H = 65, 6
    X0, Ur, G = R.rollout_problem(B, H)
    Ud, Gd = dev(Ur, gpu), dev(G, gpu)
    Xtraj = ac.rollout(dev(X0, gpu), Ud, DT)
    _, x0b, urb, drb = ac.rollout_coef_grad(Xtraj, Ud, DT, Gd)
    x0p, urp, drp = ac.rollout_vjp(Xtraj, Ud, DT, Gd)
    same_r = all(torch.equal(a, b) for a, b in ((x0b, x0p), (urb, urp), (drb, drp)))
    got = np.concatenate([host(x0b), host(urb).reshape(-1, B), host(drb)[None]])
    want = np.concatenate([host(x0p), host(urp).reshape(-1, B), host(drp)[None]])
    worst_r = float(unit_max_rel(got, want).max())
    print(f"[cgrad other outputs] {model} ns={substeps} step worst {worst:.2e} bit-identical {same}; rollout worst {worst_r:.2e} "
          f"bit-identical {same_r}")
    parity_report("cgrad_other_outputs", case=model, substeps=substeps, step_worst=worst, step_bit_identical=same,
                  rollout_worst=worst_r, rollout_bit_identical=same_r)
    assert worst <= 1e-6 and worst_r <= 1e-6


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["poly", "linear"])
def test_repeats_bit_identical_and_graph_capture(gpu, model):
    import torch

    ac = make(model)
    B, H = 300, 4
    X0, U0 = synthetic_units(B, seed=81, flaps=True)
    Ud = dev(np.repeat(f32_exact(U0)[None], H, axis=0), gpu)
    Xtraj = ac.rollout(dev(f32_exact(X0), gpu), Ud, DT)
    Gd = torch.randn(Xtraj.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    ref = ac.rollout_coef_grad(Xtraj, Ud, DT, Gd)[0]
    assert torch.equal(ref, ac.rollout_coef_grad(Xtraj, Ud, DT, Gd)[0])
    # NULL x0 / U / dt outputs: the same sweep, the same coefficient gradient
    assert torch.equal(ref, ac.rollout_coef_grad(Xtraj, Ud, DT, Gd, need=(False, False, False))[0])
    x, u, lam = Xtraj[1], Ud[1], Gd[2]
    ref_s = ac.step_coef_grad(x, u, DT, lam)[0]
    assert torch.equal(ref_s, ac.step_coef_grad(x, u, DT, lam)[0])
    assert torch.equal(ref_s, ac.step_coef_grad(x, u, DT, lam, need=(False, False, False))[0])
    ws = ac.coef_grad_workspace("rollout", B, H)  # allocated before the capture
    out = torch.empty_like(ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.rollout_coef_grad(Xtraj, Ud, DT, Gd, ws=ws, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ac.rollout_coef_grad(Xtraj, Ud, DT, Gd, ws=ws, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ref, out)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import warnings

    import torch

    from aircraft_amd import AircraftHipError, Quadrotor, _lib, autodiff

    X, U, lam = R.units(8, 91)
    args = (dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    for other in (make_aircraft("default", normalise=True), make_aircraft("nn", normalise=True)):
        with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*cubic-fit"):
            other.step_coef_grad(*args)
        with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*cubic-fit"):
            other.coef_grad_floats()
        with pytest.raises(ValueError):
            autodiff.CoefficientParameters(other)
    quad = Quadrotor()
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*cubic-fit"):
        quad.step_coef_grad(args[0], dev(U[:4], gpu), DT, args[3])
    with pytest.raises(ValueError):
        autodiff.CoefficientParameters(quad)
    poly = make("poly")
    assert poly.coef_grad_floats() == 210 and make("linear").coef_grad_floats() == 36
    # sub-steps: 30 run, 31 are refused with the limit in the text
    assert bool(torch.isfinite(make("poly", substeps=30).step_coef_grad(args[0], args[1], 0.1, args[3])[0]).all())
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*30 RK4 sub-steps"):
        make("poly", substeps=31).step_coef_grad(args[0], args[1], 0.1, args[3])
    # a short workspace
    ws = poly.coef_grad_workspace("step", 8)
    out = torch.empty(210, device=gpu)
    lib = _lib.load()
    rc = lib.ac_step_cgrad_f32(poly._handle, args[0].data_ptr(), args[1].data_ptr(), C.c_float(DT), None, 8, args[3].data_ptr(),
                               None, None, None, out.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == -6 and b"workspace" in lib.ac_last_error()
    with pytest.raises(AircraftHipError, match="AC_ERR_WORKSPACE"):
        poly.rollout_coef_grad(torch.zeros((3, 13, 8), device=gpu), torch.zeros((2, 7, 8), device=gpu), DT,
                               torch.zeros((3, 13, 8), device=gpu), ws=torch.empty(16, device=gpu))
    # the routes that existed before stay closed, as tests/test_gpu_wgrad.py pins them
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*MLP surrogate"):
        poly.step_wgrad(*args)
    with pytest.raises(ValueError):
        autodiff.MlpParameters(poly)
    with pytest.raises(TypeError, match="params"):
        autodiff.step(poly, args[0], args[1], DT, params=object())
    with pytest.raises(ValueError, match="another aircraft"):
        autodiff.step(make("poly"), args[0], args[1], DT, params=autodiff.CoefficientParameters(poly))
    # a changed coefficient cannot be installed while a stream is capturing
    params = autodiff.CoefficientParameters(poly)
    with torch.no_grad():
        params.intercept.add_(1e-3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns that the abandoned capture recorded nothing)
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g, stream=s):
                autodiff.step(poly, args[0], args[1], DT, params=params)
    torch.cuda.synchronize()


# ---- 7. the parameters take effect -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["poly", "linear"])
def test_updated_parameters_are_what_the_aircraft_runs(gpu, model):
    import torch

    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, autodiff
    from aircraft_amd.synthetic import GLIDER

    ac = make(model)
    X, U, lam = R.units(96, 71)
    x, u = dev(X, gpu).requires_grad_(True), dev(U, gpu).requires_grad_(True)
    params = autodiff.CoefficientParameters(ac)
    y0 = autodiff.step(ac, x, u, DT, params=params)
    (y0 * dev(lam, gpu)).sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in params.parameters())
    # the state and control gradients of the one sweep are those of the plain route
    x2, u2 = dev(X, gpu).requires_grad_(True), dev(U, gpu).requires_grad_(True)
    (autodiff.step(ac, x2, u2, DT) * dev(lam, gpu)).sum().backward()
    assert unit_max_rel(host(x.grad), host(x2.grad)).max() <= 1e-6 and unit_max_rel(host(u.grad), host(u2.grad)).max() <= 1e-6
    torch.optim.Adam(params.parameters(), lr=1e-4).step()
    y1 = autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params).detach()
    assert not torch.equal(y0.detach(), y1)
    data = {k: host(p) for k, p in params.named_parameters()}
    fresh = Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=data if model == "poly" else data["W"],
                                  aircraft_config=AircraftConfiguration(dict(GLIDER)), physical_integration_substeps=1))
    fresh.normalise = True
    assert torch.equal(y1, fresh.state_update(dev(X, gpu), dev(U, gpu), DT))
    assert torch.equal(y1, ac.state_update(dev(X, gpu), dev(U, gpu), DT))  # the aircraft itself now runs the new coefficients


# ---- 8. the example at a small size ------------------------------------------------------------------------------------------------
def test_fit_polynomial_example_reduces_the_loss(gpu):
    import importlib.util
    import os

    from tests.helpers import ROOT

    spec = importlib.util.spec_from_file_location("fit_polynomial", os.path.join(ROOT, "examples", "fit_polynomial.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, cerr = mod.main(["--batch", "64", "--horizon", "5", "--epochs", "30"])
    assert len(losses) == 30 and np.all(np.isfinite(losses)) and np.all(np.isfinite(cerr))
    print(f"[cgrad example] loss {losses[0]:.3e} -> {losses[-1]:.3e}, coefficient error {cerr[0]:.3e} -> {cerr[-1]:.3e}")
    assert losses[-1] < losses[0]  # (the coefficient error is reported: weakly identified cubic terms need not close in 30 epochs)
