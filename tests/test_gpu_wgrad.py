"""GPU tests of the weight gradients of the MLP surrogate (ac_step_wgrad_seeds_f32, ac_step_wgrad_f32, ac_rollout_wgrad_f32;
DESIGN.md §4.9) and of aircraft_amd.autodiff.MlpParameters.

Reference: float64 central differences of  sum over units of lam . F  over the weights of the ORIGINAL (unfolded) net through
the oracle, the difference formed per unit before the dot product, h = 3e-4 max(|w|, 0.05) (it agrees with h = 1e-3 to
<= 1.2e-7 of each tensor's max norm).  Error per tensor: max|g - g_ref| / max|g_ref|; bar 2e-5, the composed VJP route's."""
import numpy as np
import pytest

from tests.helpers import f32_exact, make_aircraft, parity_report, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

BAR = 2e-5
DT = 0.01
NETS = {  # name -> make_aircraft arguments
    "shipped": dict(),
    "net_3x64": dict(hidden=(64, 64, 64)),
    "net_3x64_valu": dict(hidden=(64, 64, 64), use_mfma=False),
    "net_4x128": dict(hidden=(128, 128, 128, 128)),
    "net_48_80": dict(hidden=(48, 80)),
}


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def make(name, **kw):
    return make_aircraft("nn", normalise=True, **NETS[name], **kw)


def oracle_with(ac, weights=None, biases=None, output_mean=None):
    """the float64 oracle of `ac` with other weights / biases / output mean"""
    from oracle import Oracle

    md = dict(ac.coefficient_model.oracle_data())
    md["weights"] = [np.asarray(w, np.float64) for w in (weights if weights is not None else md["weights"])]
    md["biases"] = [np.asarray(b, np.float64) for b in (biases if biases is not None else md["biases"])]
    if output_mean is not None:
        md["output_mean"] = np.asarray(output_mean, np.float64)
    return Oracle(ac.airframe_dict(), "nn", md, substeps=ac.physical_integration_substeps, normalise=ac.normalise,
                  stall_scaling=ac.stall_scaling, epsilon=ac.epsilon, gravity=ac.gravity)


def tensors_of(ac):
    """the original net's tensors in the order of MlpParameters.parameters(): weights, then biases (float64 copies)"""
    d = ac.coefficient_model.data
    return [np.asarray(w, np.float64) for w in d.weights] + [np.asarray(b, np.float64) for b in d.biases]


def split(ac, tensors):
    L = len(ac.coefficient_model.data.weights)
    return tensors[:L], tensors[L:]


def step_of(h_rel, w):
    return h_rel * max(abs(float(w)), 0.05)


def units(n, seed):
    X, U = synthetic_units(n, seed=seed, flaps=True)
    lam = f32_exact(np.random.default_rng(seed + 1).normal(size=(13, n)))
    return f32_exact(X), f32_exact(U), lam


def fd_entries(ac, X, U, dt, entries, h_rel=3e-4):
    """{(tensor, flat index): per-unit (13, n) central difference of F} over the listed entries"""
    base = tensors_of(ac)
    out = {}
    for t, i in entries:
        h = step_of(h_rel, base[t].flat[i])
        F = []
        for sgn in (1.0, -1.0):
            pert = [a.copy() for a in base]
            pert[t].flat[i] += sgn * h
            F.append(oracle_with(ac, *split(ac, pert)).state_update(X, U, dt))
        out[(t, i)] = (F[0] - F[1]) / (2 * h)
    return out


def fd_direction(ac, f, direction, h=3e-4):
    """central difference of the scalar f(oracle) along `direction` (a list of arrays like tensors_of)"""
    base = tensors_of(ac)
    v = []
    for sgn in (1.0, -1.0):
        pert = [a + sgn * h * d for a, d in zip(base, direction)]
        v.append(f(oracle_with(ac, *split(ac, pert))))
    return v


def random_direction(ac, rng):
    return [rng.normal(size=a.shape) * np.maximum(np.abs(a), 0.05) for a in tensors_of(ac)]


def directional_references(ac, rng, f, reduce, keep=3, draws=6):
    """`keep` random directions over all weights with their central-difference derivatives [(d, ref), ...].
    The measure |<g, d> - ref| / |ref| is only as good as the draw: <g, d> is a sum of thousands of terms of both signs, normal
    with some deviation sigma over the draws, and a draw that lands near zero asks for the cancellation, not for the gradient
    (first seen on the 5-48-80-6 net at n = 4099: one of three draws gave <g_ref, d> = 0.41 where the per-tensor terms are
    +-30 and the other two draws -10 and -61; the kernel's ABSOLUTE error there, 2.5e-5, was that of the other draws, and
    read 6.06e-5 relative).  So `draws` directions are drawn and the `keep` with the largest |ref| are used — a choice made
    from the float64 reference alone, before the code under test is looked at."""
    cand = []
    for _ in range(draws):
        d = random_direction(ac, rng)
        vp, vm = fd_direction(ac, f, d)
        cand.append((d, float(reduce(vp, vm))))
    cand.sort(key=lambda c: -abs(c[1]))
    return cand[:keep]


def grads_through_params(ac, params, loss_of):
    """.grad of every original tensor (weights, then biases) as float64 arrays"""
    for p in params.parameters():
        p.grad = None
    loss_of().backward()
    return [host(p.grad) for p in params.parameters()]


def tensor_errors(got, want):
    return [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want)]


# ---- 1. step gradient against central differences over the original tensors, small n -----------------------------------------
_STEP_REF = {}


def step_reference(name, ac, per_unit_dt):
    """Per-unit differences over the chosen entries, computed once per (net, dt kind) on a pool of units; the cases take
    prefixes of the pool (the gradient is a sum over units)."""
    key = (name, per_unit_dt)
    if key not in _STEP_REF:
        n = 130 if per_unit_dt else 65
        X, U, lam = units(n, 7 if per_unit_dt else 5)
        dt = f32_exact(np.random.default_rng(9).uniform(0.005, 0.02, n)) if per_unit_dt else DT
        rng = np.random.default_rng(3)
        entries = []
        for t, a in enumerate(tensors_of(ac)):
            idx = range(a.size) if name == "shipped" else rng.choice(a.size, size=min(16, a.size), replace=False)
            entries += [(t, int(i)) for i in idx]
        _STEP_REF[key] = (X, U, lam, dt, entries, fd_entries(ac, X, U, dt, entries))
    return _STEP_REF[key]


@pytest.mark.parametrize("n", [1, 63, 65, 130])
@pytest.mark.parametrize("name", list(NETS))
def test_step_wgrad_matches_central_differences(gpu, name, n):
    import torch

    from aircraft_amd import autodiff

    ac = make(name)
    X, U, lam, dt, entries, D = step_reference(name, ac, per_unit_dt=(n == 130))
    X, U, lam = X[:, :n], U[:, :n], lam[:, :n]
    dtd = dev(dt[:n], gpu) if np.ndim(dt) else dt
    params = autodiff.MlpParameters(ac)
    got = grads_through_params(ac, params, lambda: (autodiff.step(ac, dev(X, gpu), dev(U, gpu), dtd, params=params) * dev(lam, gpu)).sum())
    assert ac.last_launch()[0] == "k_mlp_wgrad"
    base = tensors_of(ac)
    errs = []
    for t in range(len(base)):
        idx = [i for tt, i in entries if tt == t]
        ref = np.array([(lam * D[(t, i)][:, :n]).sum() for i in idx])
        g = got[t].reshape(-1)[idx]
        errs.append(float(np.abs(g - ref).max() / np.abs(ref).max()))
    print(f"[wgrad step] {name} n={n} worst tensor err {max(errs):.3e}")
    parity_report("step_wgrad", net=name, n=n, worst_tensor_rel=max(errs), per_tensor=errs)
    assert max(errs) < BAR, errs


# ---- 2. several partials, a ragged last tile: directional differences over all weights -----------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_step_wgrad_multi_workgroup_directional(gpu, name):
    from aircraft_amd import autodiff

    ac = make(name)
    n = 4099
    X, U, lam = units(n, 21)
    params = autodiff.MlpParameters(ac)
    got = grads_through_params(ac, params, lambda: (autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params) * dev(lam, gpu)).sum())
    rng = np.random.default_rng(22)
    errs = []
    for d, ref in directional_references(ac, rng, lambda o: o.state_update(X, U, DT),
                                         lambda Fp, Fm: (lam * ((Fp - Fm) / (2 * 3e-4))).sum()):  # (per unit before the dot product)
        g = float(sum((a * b).sum() for a, b in zip(got, d)))
        errs.append(abs(g - ref) / abs(ref))
    print(f"[wgrad directional] {name} n={n} errs {errs}")
    parity_report("step_wgrad_directional", net=name, n=n, errs=errs)
    assert max(errs) < BAR, errs


# ---- 3. the seeds alone: differences over output_mean ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shipped", "net_4x128"])
def test_seeds_match_output_mean_differences(gpu, name):
    ac = make(name)
    n = 130
    X, U, lam = units(n, 31)
    Z, Yb = ac.step_wgrad_seeds(dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    assert tuple(Z.shape) == (4, 5, n) and tuple(Yb.shape) == (4, 6, n)
    d = ac.coefficient_model.data
    om, os_ = np.asarray(d.output_mean, np.float64), np.asarray(d.output_std, np.float64)
    got = host(Yb).sum(axis=0) / os_[:, None]   # d(lam . F)/d(mean_k) per unit
    want = np.zeros((6, n))
    for k in range(6):
        h = step_of(3e-4, om[k])
        F = []
        for sgn in (1.0, -1.0):
            m = om.copy(); m[k] += sgn * h
            F.append(oracle_with(ac, output_mean=m).state_update(X, U, DT))
        want[k] = (lam * (F[0] - F[1]) / (2 * h)).sum(axis=0)
    err = unit_max_rel(got, want)
    print(f"[wgrad seeds] {name} worst unit {err.max():.3e}")
    assert err.max() < BAR, (int(err.argmax()), float(err.max()))
    # stage 0's z is the normalised input at the unit's own state
    a = make_oracle_aero(ac, X, U)
    z0 = (a - np.asarray(d.input_mean, np.float64)[:, None]) / np.asarray(d.input_std, np.float64)[:, None]
    assert np.abs(host(Z)[0] - z0).max() < 1e-5 * max(1.0, np.abs(z0).max())


def make_oracle_aero(ac, X, U):
    from tests.helpers import make_oracle

    o = make_oracle(ac)
    a = o.aero(X, U)
    return np.stack([a[o.AERO_ROWS["qbar"]], a[o.AERO_ROWS["alpha"]], a[o.AERO_ROWS["beta"]], U[0], U[1]])


# ---- 4. the weight-gradient kernel alone: torch float64 autograd on the kernel's own seeds ------------------------------------
def torch_wgrad_on_seeds(params, Z, Yb, dtype):
    """[dW_0, db_0, dW_1, ...] of sum(ybar . mlp(z)) over the folded net by torch autograd in `dtype`"""
    import torch

    layers = [(W.detach().to(Z.device, dtype).requires_grad_(True), b.detach().to(Z.device, dtype).requires_grad_(True))
              for W, b in params.folded()]
    h = Z.to(dtype).permute(0, 2, 1).reshape(-1, 5)
    yb = Yb.to(dtype).permute(0, 2, 1).reshape(-1, 6)
    for l, (W, b) in enumerate(layers):
        h = h @ W.T + b
        if l < len(layers) - 1:
            h = torch.tanh(h)
    (h * yb).sum().backward()
    return [t.grad for W, b in layers for t in (W, b)]


def split_flat(params, flat):
    out, off = [], 0
    for W, b in params.folded():
        for t in (W, b):
            out.append(flat[off:off + t.numel()].reshape(t.shape)); off += t.numel()
    assert off == flat.numel()
    return out


@pytest.mark.parametrize("n", [1, 130, 4099])
@pytest.mark.parametrize("name", list(NETS))
def test_wgrad_kernel_matches_torch_float64_on_own_seeds(gpu, name, n):
    import torch

    from aircraft_amd import autodiff

    ac = make(name)
    X, U, lam = units(n, 41)
    Z, Yb = ac.step_wgrad_seeds(dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    g = ac.step_wgrad(dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    params = autodiff.MlpParameters(ac)
    assert g.numel() == ac.mlp_grad_floats() == params.flat().numel()
    assert ac.mlp_folded_shape() == [5] + [W.shape[0] for W, _ in params.folded()]
    want = torch_wgrad_on_seeds(params, Z, Yb, torch.float64)
    errs = tensor_errors([host(t) for t in split_flat(params, g)], [host(t) for t in want])
    print(f"[wgrad kernel] {name} n={n} worst tensor err {max(errs):.3e}")
    parity_report("wgrad_kernel", net=name, n=n, worst_tensor_rel=max(errs))
    assert max(errs) < BAR, errs


# ---- 5. the two flavours of the matrix product --------------------------------------------------------------------------------
def test_mfma_and_vector_flavours_agree(gpu):
    import torch

    from aircraft_amd import autodiff

    X, U, lam = units(1000, 51)
    g = {}
    for name in ("net_3x64", "net_3x64_valu"):
        ac = make(name)
        g[name] = ac.step_wgrad(dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
        params = autodiff.MlpParameters(ac)
    a, b = (split_flat(params, g[k]) for k in ("net_3x64", "net_3x64_valu"))
    errs = tensor_errors([host(t) for t in a], [host(t) for t in b])
    print(f"[wgrad flavours] worst tensor difference {max(errs):.3e}; bit-identical: {torch.equal(g['net_3x64'], g['net_3x64_valu'])}")
    # (measured on an MI355X: 2.0e-7 and NOT bit-identical — the two flavours of the forward pass that produce the seeds differ
    # in their first and last layers, which the matrix-core engine runs on the vector ALUs in another summation order)
    assert max(errs) < 1e-6, errs


# ---- 6. rollout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(5, 7), (70, 3)])
@pytest.mark.parametrize("name", list(NETS))
def test_rollout_wgrad_directional(gpu, name, B, H):
    from aircraft_amd import autodiff

    ac = make(name)
    X0, U0 = synthetic_units(B, seed=61, flaps=True)
    X0, U0 = f32_exact(X0), f32_exact(U0)
    rng = np.random.default_rng(62)
    U = f32_exact(U0[None] + 0.01 * rng.normal(size=(H, 7, B)) * (np.abs(U0[None]) + 0.1))
    G = f32_exact(rng.normal(size=(H + 1, 13, B)))
    params = autodiff.MlpParameters(ac)
    got = grads_through_params(ac, params, lambda: (autodiff.rollout(ac, dev(X0, gpu), dev(U, gpu), DT, params=params) * dev(G, gpu)).sum())
    errs = []
    for d, ref in directional_references(ac, rng, lambda o: float((G * o.rollout(X0, U, DT)).sum()),
                                         lambda Lp, Lm: (Lp - Lm) / (2 * 3e-4)):
        g = float(sum((a * b).sum() for a, b in zip(got, d)))
        errs.append(abs(g - ref) / abs(ref))
    print(f"[wgrad rollout] {name} B={B} H={H} errs {errs}")
    parity_report("rollout_wgrad_directional", net=name, B=B, H=H, errs=errs)
    assert max(errs) < BAR, errs


# ---- 7. autograd end to end ------------------------------------------------------------------------------------------------------
def test_autograd_fills_every_parameter_and_equals_wrappers(gpu):
    import torch

    from aircraft_amd import autodiff

    ac = make("shipped")
    X, U, lam = units(96, 71)
    params = autodiff.MlpParameters(ac)
    x = dev(X, gpu).requires_grad_(True)
    u = dev(U, gpu).requires_grad_(True)
    y = autodiff.step(ac, x, u, DT, params=params)
    (y * dev(lam, gpu)).sum().backward()
    assert len(list(params.parameters())) == 6  # 5-16-32-6: three weights, three biases
    for p in params.parameters():  # both tensors of the folded pair (layers 0 and 1) included
        assert p.grad is not None and float(p.grad.abs().max()) > 0
    # ... equal to the explicit wrapper pushed through the fold
    g = ac.step_wgrad(dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    flat = params.flat()
    want = torch.autograd.grad(flat, list(params.parameters()), grad_outputs=g.to(flat.device))
    assert all(torch.equal(p.grad, w) for p, w in zip(params.parameters(), want))
    # the state and control gradients do not depend on `params`
    x2 = dev(X, gpu).requires_grad_(True)
    u2 = dev(U, gpu).requires_grad_(True)
    (autodiff.step(ac, x2, u2, DT) * dev(lam, gpu)).sum().backward()
    assert torch.equal(x.grad, x2.grad) and torch.equal(u.grad, u2.grad)
    # rollout: the same two properties
    Ut = dev(np.repeat(U[None], 4, axis=0), gpu).requires_grad_(True)
    for p in params.parameters():
        p.grad = None
    Xr = autodiff.rollout(ac, dev(X, gpu), Ut, DT, params=params)
    Gt = torch.randn(Xr.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    (Xr * Gt).sum().backward()
    gr = ac.rollout_wgrad(Xr.detach(), Ut.detach(), DT, Gt)
    want = torch.autograd.grad(params.flat(), list(params.parameters()), grad_outputs=gr.to(flat.device))
    assert all(torch.equal(p.grad, w) for p, w in zip(params.parameters(), want))
    Ut2 = Ut.detach().clone().requires_grad_(True)
    (autodiff.rollout(ac, dev(X, gpu), Ut2, DT) * Gt).sum().backward()
    assert torch.equal(Ut.grad, Ut2.grad)
    # an optimiser step changes the parameters: the next forward pass re-installs them
    y0 = autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params).detach().clone()
    opt = torch.optim.SGD(params.parameters(), lr=1e-2)
    opt.step()
    y1 = autodiff.step(ac, dev(X, gpu), dev(U, gpu), DT, params=params).detach()
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, ac.state_update(dev(X, gpu), dev(U, gpu), DT))  # the aircraft itself now runs the new weights
    with pytest.raises(ValueError):
        autodiff.step(make("shipped"), dev(X, gpu), dev(U, gpu), DT, params=params)  # params of another aircraft


# ---- 8. repeatability and graph capture ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shipped", "net_4x128"])
def test_wgrad_repeats_bit_identical_and_graph_capture(gpu, name):
    import torch

    ac = make(name)
    B, H = 300, 4
    X0, U0 = synthetic_units(B, seed=81, flaps=True)
    Ud = dev(np.repeat(f32_exact(U0)[None], H, axis=0), gpu)
    Xtraj = ac.rollout(dev(f32_exact(X0), gpu), Ud, DT)
    Gd = torch.randn(Xtraj.shape, device=gpu, generator=torch.Generator(device=gpu).manual_seed(7))
    ref = ac.rollout_wgrad(Xtraj, Ud, DT, Gd)
    assert torch.equal(ref, ac.rollout_wgrad(Xtraj, Ud, DT, Gd))
    x, u, lam = Xtraj[1], Ud[1], Gd[2]
    ref_s = ac.step_wgrad(x, u, DT, lam)
    assert torch.equal(ref_s, ac.step_wgrad(x, u, DT, lam))
    ws = ac.wgrad_workspace("rollout", B, H)  # allocated before the capture
    out = torch.empty_like(ref)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ac.rollout_wgrad(Xtraj, Ud, DT, Gd, ws=ws, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ac.rollout_wgrad(Xtraj, Ud, DT, Gd, ws=ws, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ref, out)


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import ctypes as C

    import torch

    from aircraft_amd import AircraftHipError, _lib, autodiff

    X, U, lam = units(8, 91)
    args = (dev(X, gpu), dev(U, gpu), DT, dev(lam, gpu))
    poly = make_aircraft("poly", normalise=True)
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*MLP surrogate"):
        poly.step_wgrad(*args)
    with pytest.raises(ValueError):
        autodiff.MlpParameters(poly)
    sub = make("shipped", substeps=2)
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*sub-step"):
        sub.step_wgrad(*args)
    with pytest.raises(AircraftHipError, match="AC_ERR_UNSUPPORTED.*sub-step"):
        sub.step_wgrad_seeds(*args)
    ac = make("shipped")
    ws = ac.wgrad_workspace("step", 8)
    out = torch.empty(ac.mlp_grad_floats(), device=gpu)
    lib = _lib.load()
    rc = lib.ac_step_wgrad_f32(ac._handle, args[0].data_ptr(), args[1].data_ptr(), C.c_float(DT), None, 8, args[3].data_ptr(),
                               out.data_ptr(), ws.data_ptr(), ws.numel() - 1, None)
    assert rc == -6 and b"workspace" in lib.ac_last_error()
    with pytest.raises(AircraftHipError, match="AC_ERR_WORKSPACE"):
        ac.rollout_wgrad(torch.zeros((3, 13, 8), device=gpu), torch.zeros((2, 7, 8), device=gpu), DT,
                         torch.zeros((3, 13, 8), device=gpu), ws=torch.empty(16, device=gpu))
    # a changed weight cannot be installed while a stream is capturing
    params = autodiff.MlpParameters(ac)
    with torch.no_grad():
        params.biases[0].add_(1e-3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (torch warns that the abandoned capture recorded nothing)
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g, stream=s):
                autodiff.step(ac, args[0], args[1], DT, params=params)
    torch.cuda.synchronize()


# ---- 10. the example at a small size -----------------------------------------------------------------------------------------------
def test_fit_surrogate_example_recovers_the_loss(gpu):
    import importlib.util
    import os

    from tests.helpers import ROOT

    spec = importlib.util.spec_from_file_location("fit_surrogate", os.path.join(ROOT, "examples", "fit_surrogate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses = mod.main(["--batch", "64", "--horizon", "8", "--iters", "40"])
    assert len(losses) == 40 and np.all(np.isfinite(losses))
    # measured on an MI355X at this size: 1.718e-1 -> 1.023e-3, a reduction by 168; the assertion asks for half of it
    print(f"[wgrad example] loss {losses[0]:.3e} -> {losses[-1]:.3e} (x{losses[0] / losses[-1]:.0f})")
    assert losses[-1] < losses[0] / 84.0, (losses[0], losses[-1])
