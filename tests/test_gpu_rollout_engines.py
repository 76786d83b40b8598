"""Every rollout-engine instance, open loop (ac_rollout_f32) and closed loop (ac_rollout_policy_f32), against the float64 oracle.

The rows are tests/rollout_matrix.py: one net per template instance the host can pick (tests/test_mlp_model_host.py pins, on
the CPU, that each net reaches the instance it is listed for; here ac.last_launch() is asserted per row).

What carries these tests is the ONE-STEP check: from every node the GPU stored, one float64 step of the oracle must land on
the next stored node within STATE_TOL = 1e-5 (block-relative) — every instance, every node, nothing excluded.  The kernels
carry the state in float64 and store it rounded to fp32, so the restart differs from the kernel's own state by at most one
fp32 rounding, and a single RK4 step does not amplify: the bar is the one tests/test_gpu_parity.py::test_state_update holds
on random states without a mask.  The chained comparison (helpers.check_against_conditioning: within 1e-5, or within 8 x
what a one-ulp perturbation of x0 does to the float64 reference) and the bit-exact placement invariance come on top.

Closed loop: constructed gains (not a backward pass), a control box tight enough that both limits are hit, and every stored
control compared with the float64 restatement of the policy from the GPU's own stored state, within the bound of an fp32 dot
product:  16 * 2^-24 * (|U| + |alpha kff| + sum_m |K_m| |dx_m|)  + sum_m |K_m| (ulp(x_m) + ulp(xnom_m)).

Every case appends its figures to the parity report (helpers.parity_report)."""
import numpy as np
import pytest

from tests.helpers import (GLIDER, block_rel_err, check_against_conditioning, conditioning, f32_exact, instance_err,
                           make_aircraft, make_oracle, near_trim_problem, parity_report)
from tests.rollout_matrix import ANALYTIC_ROWS, MLP_ROW_IDS, MLP_ROWS, mlp_data

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-5
DT = float(np.float32(0.01))  # the step as the fp32 ABI passes it, for both sides
B_OPEN = 37                   # three 16-instance slabs, the last one ragged
U32 = 2.0 ** -24              # unit round-off of fp32
POLICY_ROWS = [r for r in MLP_ROWS if r.policy_kernel is not None]
CLOSED_IDS = [r.id for r in POLICY_ROWS] + ANALYTIC_ROWS
# (B, n_alpha): Bout = 40 with every slab straddling three or four line-search candidates and the ABI's maximum of eight; a
# lone instance; and the shape of tests/test_gpu_ilqr.py
SHAPES = [(5, 8), (1, 1), (20, 3)]
ALPHAS = {8: [1.0, 0.75, 0.5, 0.375, 0.25, 0.125, 0.0625, 0.03125], 1: [1.0], 3: [1.0, 0.5, 0.125]}  # exact in fp32
SURFACE_BOX = 1.5             # degrees either side of zero (the nominal surface deflections stay within +-1.2 deg)
QUAD_HOVER = -9.81 / 4        # thrust per rotor in hover; the quadrotor's box is SURFACE_BOX newtons either side of it
# seeds of the constructed gains per shape (the lone instance has 12 .. 24 boxed entries: a seed whose draw reaches both
# limits at H = 4 and at H = 6, chosen on the float64 restatement)
CLOSED_SEEDS = {(5, 8): 101, (1, 1): 184, (20, 3): 103}


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def flat(X):
    """(n, rows, B) -> (rows, n * B): the nodes of a trajectory as independent units"""
    return np.ascontiguousarray(X.transpose(1, 0, 2).reshape(X.shape[1], -1))


# ---- one aircraft + oracle per row, built once -------------------------------------------------------------------------------
_CTX = {}


def build_row(row):
    if row.act is None:
        return make_aircraft("nn", hidden=row.hidden, normalise=True, use_mfma=row.use_mfma)
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts

    ac = Aircraft(AircraftOpts(coeff_model_type="nn", coeff_model_path=mlp_data(row), physical_integration_substeps=1,
                               aircraft_config=AircraftConfiguration(dict(GLIDER)), use_mfma=row.use_mfma))
    ac.normalise = True
    return ac


def context(key):
    """key: a row id of the matrix, or 'default' / 'linear' / 'poly' / 'quad'.  -> dict(ac, orc, row, H, X0, U)"""
    if key in _CTX:
        return _CTX[key]
    row = MLP_ROWS[MLP_ROW_IDS.index(key)] if key in MLP_ROW_IDS else None
    H = row.H if row else 6
    if key == "quad":
        from aircraft_amd import Quadrotor
        from tests.test_gpu_quadrotor import quad_units

        ac = Quadrotor()
        ac.normalise = True
        X0, _ = quad_units(B_OPEN, seed=17)
        rng = np.random.default_rng(18)
        U = np.zeros((H, 7, B_OPEN))
        U[:, :4] = QUAD_HOVER + np.cumsum(rng.normal(0, 0.2, (H, 4, B_OPEN)), axis=0)
        U = f32_exact(U)
    else:
        ac = build_row(row) if row else make_aircraft(key, normalise=True)
        X0, U = near_trim_problem(B_OPEN, H, seed=17)
        if key == "default":
            # The analytic model's pitch damping is stiff: explicit RK4 leaves its stability region at about V dt = 0.55 m.
            # Measured on the float64 oracle, these 37 instances (45 .. 78 m/s), open loop, six steps, worst |omega|:
            #   dt = 0.005: 0.23 rad/s at every speed;  dt = 0.01: <= 0.17 up to 54 m/s, 1 .. 3 at 57 .. 59, 1.4e2 at 63,
            #   4.4e9 at 70, 1e158 at 75, inf at 78;  dt = 0.02: 71 at 45 m/s, 1.5e97 at 51, inf from 57 m/s on.
            # From 61 m/s on the reference overflows fp32 inside the horizon and one step from a stored node is inf.  Gliders
            # at 20 .. 26 m/s stay inside the region up to the largest step of the time-row case, 0.02 s (worst 0.3 rad/s);
            # one set of initial states serves every closed-loop case of the model.
            V = np.linalg.norm(X0[3:6], axis=0)
            X0[3:6] *= (20.0 + (V - 45.0) * 6.0 / 35.0) / V
        X0, U = f32_exact(X0), f32_exact(U)
    _CTX[key] = dict(key=key, ac=ac, orc=make_oracle(ac), row=row, H=H, X0=X0, U=U)
    return _CTX[key]


def open_loop(c, gpu):
    """The full open-loop call of the row (B_OPEN instances), its float64 reference and the reference's conditioning: once."""
    if "out" not in c:
        c["out"] = c["ac"].rollout(dev(c["X0"], gpu), dev(c["U"], gpu), DT)
        c["launch"] = c["ac"].last_launch()
        c["ref"], c["dev"] = conditioning(c["orc"], c["X0"], c["U"], DT)
    return c["out"]


def one_step_error(orc, X, U, dt=DT):
    """Worst block-relative distance between the stored node k+1 and one float64 step from the stored node k, over every
    node and instance.  X (H+1, 13, n), U (H, 7, n); dt a number or (H, n)."""
    dtf = dt if np.ndim(dt) == 0 else np.ascontiguousarray(np.asarray(dt, dtype=np.float64).reshape(-1))
    return block_rel_err(flat(X[1:]), orc.state_update(flat(X[:-1]), flat(U), dtf))


def check_open_loop(name, orc, X0, U, out, ref, cond):
    assert out.shape == ref.shape and np.isfinite(out).all()
    assert np.array_equal(out[0], X0.astype(np.float32))
    step = one_step_error(orc, out, U)
    parity_report(name, one_step_max=step, reference_deviation_max=float(cond.max()))
    assert step < STATE_TOL, (name, "one step from the stored nodes", step)
    err, frac = check_against_conditioning(name + "[chained]", out, ref, cond, STATE_TOL)
    return step, float(err.max()), frac


# ---- open loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", MLP_ROW_IDS)
def test_open_loop_rollout(gpu, rid):
    c = context(rid)
    out = open_loop(c, gpu)
    assert c["launch"][0] == c["row"].open_kernel, c["launch"]
    assert c["ac"].mlp_folded_shape()[0] == 5 and len(c["ac"].mlp_folded_shape()) == c["row"].layers + 1
    check_open_loop(f"rollout_engines[{rid}]", c["orc"], c["X0"], c["U"], f64(out), c["ref"], c["dev"])


@pytest.mark.parametrize("rid", MLP_ROW_IDS)
def test_open_loop_placement_invariance(gpu, rid):
    """An instance's trajectory does not depend on where in the batch it sits, to the bit: the last 21 columns on their own
    (other slabs, other lanes), a lone instance with 15 shadowing lanes, a full slab, one live lane in the second slab — and
    a repeat of the full call."""
    import torch

    c = context(rid)
    ac, full = c["ac"], open_loop(c, gpu)
    X0, U = dev(c["X0"], gpu), dev(c["U"], gpu)
    again = ac.rollout(X0, U, DT)
    assert ac.last_launch()[0] == c["row"].open_kernel
    assert torch.equal(again, full)
    tail = ac.rollout(X0[:, 16:].contiguous(), U[:, :, 16:].contiguous(), DT)
    assert torch.equal(tail, full[:, :, 16:])
    for n in (1, 16, 17):
        head = ac.rollout(X0[:, :n].contiguous(), U[:, :, :n].contiguous(), DT)
        assert ac.last_launch()[0] == c["row"].open_kernel
        assert torch.equal(head, full[:, :, :n]), n


def test_open_loop_tiled32_past_the_small_batch_threshold(gpu):
    """k_nn_rollout_tiled<32> (64 instances per wave) takes over from the small-batch tile past kRolloutUnits * 4 * CUs
    instances: 8 * 4 * 256 + 5 = 8197 on an MI355X — a ragged last wave."""
    import torch

    c = context("tiled8-32-ragged")
    B, H = 8 * 4 * 256 + 5, 3
    X0, U = near_trim_problem(B, H, seed=17)
    X0, U = f32_exact(X0), f32_exact(U)
    out = c["ac"].rollout(dev(X0, gpu), dev(U, gpu), DT)
    assert c["ac"].last_launch()[0] == "k_nn_rollout_tiled", c["ac"].last_launch()
    ref, cond = conditioning(c["orc"], X0, U, DT)
    check_open_loop("rollout_engines[tiled-32-ragged-8197]", c["orc"], X0, U, f64(out), ref, cond)
    assert torch.equal(c["ac"].rollout(dev(X0, gpu), dev(U, gpu), DT), out)
    # one instance fewer than the threshold allows stays on the small-batch tile
    c["ac"].rollout(dev(X0[:, :8192], gpu), dev(U[:, :, :8192], gpu), DT)
    assert c["ac"].last_launch()[0] == "k_nn_rollout_tiled8"


def test_width_128_without_matrix_cores_has_no_closed_loop(gpu):
    """k_nn_rollout<8, false> has no policy counterpart: ac_rollout_policy_f32 refuses the net loudly."""
    import torch
    from aircraft_amd import AircraftHipError
    from aircraft_amd.control import ILQR, QuadraticCost

    c = context("seq8-valu")
    il = ILQR(system=c["ac"], dt=DT, num_nodes=c["H"], cost=QuadraticCost())
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
    with pytest.raises(AircraftHipError, match="needs hidden width 32 or 64"):
        il.forward(dev(c["X0"][:, :5], gpu), z(c["H"] + 1, 13, 5), dev(c["U"][:, :, :5], gpu), z(c["H"], 7, 13, 5),
                   z(c["H"], 7, 5), alphas=[1.0])


# ---- closed loop -------------------------------------------------------------------------------------------------------------
def control_box(key, time_row=0, dt_bounds=None):
    if key == "quad":
        lo, hi = [QUAD_HOVER - SURFACE_BOX] * 4 + [0.0] * 3, [QUAD_HOVER + SURFACE_BOX] * 4 + [0.0] * 3
    else:
        lo, hi = [-SURFACE_BOX] * 3 + [0.0] * 4, [SURFACE_BOX] * 3 + [0.0, 0.0, 0.0, 1.0]
    lo, hi = [float(np.float32(v)) for v in lo], [float(np.float32(v)) for v in hi]
    if time_row:
        lo[time_row], hi[time_row] = float(np.float32(dt_bounds[0])), float(np.float32(dt_bounds[1]))
    return lo, hi


def closed_loop_problem(c, B, na, seed, time_row=0):
    """The first B instances of the row's open-loop problem with constructed gains: K ~ 0.3 N(0, 1), kff ~ N(0, 1)."""
    H = c["H"]
    rng = np.random.default_rng(seed)
    X0, U = c["X0"][:, :B].copy(), c["U"][:, :, :B].copy()
    K = 0.3 * rng.standard_normal((H, 7, 13, B))
    kff = rng.standard_normal((H, 7, B))
    if time_row:  # steps spread over and beyond dt_bounds = (0.005, 0.02); gains of that row in seconds, not degrees
        U[:, time_row] = rng.uniform(0.003, 0.024, (H, B))
        K[:, time_row] *= 0.02
        kff[:, time_row] *= 0.004
    return X0, f32_exact(U), f32_exact(K), f32_exact(kff), ALPHAS[na]


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def check_controls(name, Xc, Uc, Xnom, U, K, kff, alphas, lo, hi, rows):
    """Every stored control against the float64 policy evaluated at the GPU's own stored state.  Returns the worst ratio of
    error to bound, and the fractions of the entries of `rows` at the lower limit, at the upper limit and inside."""
    H, _, B = U.shape
    lo, hi = np.asarray(lo)[:, None], np.asarray(hi)[:, None]
    worst, n_lo, n_hi, n_in = 0.0, 0, 0, 0
    for a, al in enumerate(alphas):
        sl = slice(a * B, (a + 1) * B)
        for k in range(H):
            x, got = Xc[k][:, sl], Uc[k][:, sl]
            dx = x - Xnom[k]
            raw = U[k] + al * kff[k] + np.einsum("imb,mb->ib", K[k], dx)
            bound = 16 * U32 * (np.abs(U[k]) + np.abs(al * kff[k]) + np.einsum("imb,mb->ib", np.abs(K[k]), np.abs(dx))) \
                + np.einsum("imb,mb->ib", np.abs(K[k]), ulp32(x) + ulp32(Xnom[k]))
            above, below = raw > hi + bound, raw < lo - bound
            inside = (raw < hi - bound) & (raw > lo + bound)
            assert np.array_equal(got[above], np.broadcast_to(hi, raw.shape)[above]), (name, "upper limit", a, k)
            assert np.array_equal(got[below], np.broadcast_to(lo, raw.shape)[below]), (name, "lower limit", a, k)
            err = np.abs(got - raw)
            edge = ~(above | below | inside)  # within the bound of a limit: the limit itself, or the unclipped value
            err = np.where(edge & ((got == lo) | (got == hi)), 0.0, err)
            ok = above | below | (err <= bound)
            assert ok.all(), (name, "control beyond the fp32 dot-product bound", a, k, float((err / np.maximum(bound, 1e-300))[~ok].max()))
            free = ~(above | below) & (bound > 0)
            if free.any():
                worst = max(worst, float((err[free] / bound[free]).max()))
            n_lo += int(below[rows].sum()); n_hi += int(above[rows].sum()); n_in += int(inside[rows].sum())
    n = float(len(alphas) * H * B * len(range(*rows.indices(7))))
    return worst, n_lo / n, n_hi / n, n_in / n


def closed_loop_conditioning(orc, cost, X0, Xnom, U, K, kff, alphas, eps=1e-7, draws=3, seed=0):
    """helpers.conditioning for the closed loop: the float64 restatement, and how far it moves under a one-ulp perturbation
    of x0 (random signs, worst of `draws`), per output instance."""
    import ilqr_oracle as io

    rng = np.random.default_rng(seed)
    with np.errstate(all="ignore"):
        Xr, Ur = io.forward(orc, cost, X0, Xnom, U, K, kff, alphas, DT)
        worst = np.zeros(Xr.shape[-1])
        for _ in range(draws):
            Xp, _ = io.forward(orc, cost, X0 * (1.0 + eps * rng.choice([-1.0, 1.0], X0.shape)), Xnom, U, K, kff, alphas, DT)
            worst = np.maximum(worst, np.nan_to_num(instance_err(Xp, Xr), nan=np.inf))
    return Xr, Ur, worst


def run_closed_loop(gpu, key, B, na, seed, time_row=0, dt_bounds=(0.005, 0.02)):
    from aircraft_amd.control import ILQR, QuadraticCost

    c = context(key)
    ac, orc, H = c["ac"], c["orc"], c["H"]
    lo, hi = control_box(key, time_row, dt_bounds)
    cost = QuadraticCost(u_min=lo, u_max=hi)
    if time_row:
        # (the box as the fp32 ABI passes it, so that the float64 restatement clips at the very values the kernel clips at)
        il = ILQR(system=ac, dt=DT, num_nodes=H, cost=cost, time="variable",
                  dt_bounds=tuple(float(np.float32(v)) for v in dt_bounds))
        assert il.time_row == time_row and il.cost.dt_row == time_row
        assert list(il.cost.u_min) == lo and list(il.cost.u_max) == hi
    else:
        il = ILQR(system=ac, dt=DT, num_nodes=H, cost=cost)
    assert ac.normalise is True
    X0, U, K, kff, alphas = closed_loop_problem(c, B, na, seed, time_row)
    Ud = dev(U, gpu)
    if time_row:  # the nominal trajectory at the nodes' own (clipped) steps: the policy rollout with zero gains
        import torch

        z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731
        Xnom_d, _ = il.forward(dev(X0, gpu), z(H + 1, 13, B), Ud, z(H, 7, 13, B), z(H, 7, B), alphas=[0.0])
    else:
        Xnom_d = ac.rollout(dev(X0, gpu), Ud, DT)
    Xc, Uc = il.forward(dev(X0, gpu), Xnom_d, Ud, dev(K, gpu), dev(kff, gpu), alphas=alphas)
    launch = ac.last_launch()
    Xc, Uc, Xnom = f64(Xc), f64(Uc), f64(Xnom_d)
    name = f"policy_engines[{key}-{B}x{na}{'-dt' if time_row else ''}]"
    assert Xc.shape == (H + 1, 13, na * B) and Uc.shape == (H, 7, na * B)
    assert np.isfinite(Xc).all() and np.isfinite(Uc).all()
    assert np.array_equal(Xc[0], np.tile(X0, (1, na)))
    rows = slice(0, 4) if key == "quad" else slice(0, 3)
    ratio, f_lo, f_hi, f_in = check_controls(name, Xc, Uc, Xnom, U, K, kff, alphas, lo, hi, rows)
    step = one_step_error(orc, Xc, Uc, Uc[:, time_row] if time_row else DT)
    Xr, Ur, cond = closed_loop_conditioning(orc, il.cost, X0, Xnom, U, K, kff, alphas)
    parity_report(name, kernel=launch[0], one_step_max=step, control_err_over_bound_max=ratio, clipped_low=f_lo, clipped_high=f_hi,
                  inside=f_in, reference_deviation_max=float(cond.max()))
    assert step < STATE_TOL, (name, "one step from the stored nodes", step)
    check_against_conditioning(name + "[chained]", Xc, Xr, cond, STATE_TOL)
    return dict(launch=launch, clip=(f_lo, f_hi, f_in), Uc=Uc, Ur=Ur, lo=lo, hi=hi, name=name)


@pytest.mark.parametrize("B,na", SHAPES, ids=[f"{b}x{n}" for b, n in SHAPES])
@pytest.mark.parametrize("key", CLOSED_IDS)
def test_closed_loop_rollout(gpu, key, B, na):
    r = run_closed_loop(gpu, key, B, na, seed=CLOSED_SEEDS[(B, na)])
    row = context(key)["row"]
    assert r["launch"][0] == (row.policy_kernel if row else "k_rollout_policy"), r["launch"]
    # the clip is exercised: both limits are hit, and most nodes stay inside
    f_lo, f_hi, f_in = r["clip"]
    assert f_lo > 0 and f_hi > 0 and f_in > 0.5, (r["name"], r["clip"])


@pytest.mark.parametrize("rid", [r.id for r in POLICY_ROWS])
def test_closed_loop_with_zero_gains_is_the_open_loop_rollout(gpu, rid):
    """The candidate alpha = 0 with K = 0 runs the same engine with the same arithmetic as ac_rollout_f32: bit-identical
    (the nominal controls lie inside the box)."""
    import torch
    from aircraft_amd.control import ILQR, QuadraticCost

    c = context(rid)
    ac, H, B = c["ac"], c["H"], 20
    lo, hi = control_box(rid)
    assert np.abs(c["U"][:, :3]).max() < SURFACE_BOX
    il = ILQR(system=ac, dt=DT, num_nodes=H, cost=QuadraticCost(u_min=lo, u_max=hi))
    X0, U = dev(c["X0"][:, :B], gpu), dev(c["U"][:, :, :B], gpu)
    want = ac.rollout(X0, U, DT)
    assert ac.last_launch()[0] == c["row"].open_kernel
    kff = dev(np.random.default_rng(7).standard_normal((H, 7, B)), gpu)
    Xc, Uc = il.forward(X0, want, U, torch.zeros((H, 7, 13, B), device=gpu), kff, alphas=[0.0])
    assert ac.last_launch()[0] == c["row"].policy_kernel
    assert torch.equal(Uc, U) and torch.equal(Xc, want)


@pytest.mark.parametrize("key,time_row", [("coop2-shipped", 3), ("tiled8-32-ragged", 3), ("default", 3), ("quad", 4)])
def test_closed_loop_with_time_as_a_decision_variable(gpu, key, time_row):
    """ILQR(time='variable'): control row 3 (quadrotor: 4) carries dt_k; node k is integrated with its own CLIPPED step.  The
    nominal steps are spread over and beyond dt_bounds, so both ends of that box are hit too."""
    r = run_closed_loop(gpu, key, 20, 3, seed=104, time_row=time_row)
    row = context(key)["row"]
    assert r["launch"][0] == (row.policy_kernel if row else "k_rollout_policy"), r["launch"]
    dts, lo, hi = r["Uc"][:, time_row], r["lo"][time_row], r["hi"][time_row]
    assert lo == float(np.float32(0.005)) and hi == float(np.float32(0.02))
    assert (dts >= lo).all() and (dts <= hi).all()
    ref = r["Ur"][:, time_row]  # the float64 restatement clips at both ends and leaves most steps inside
    assert (ref == lo).any() and (ref == hi).any() and ((ref > lo) & (ref < hi)).mean() > 0.5
    assert (dts == lo).any() and (dts == hi).any()


def test_time_row_refusals(gpu):
    """AC_ERR_BAD_ARG, each with its own message: a time row the force model reads, and a step box that admits dt <= 0."""
    import torch
    from aircraft_amd import AircraftHipError
    from aircraft_amd.control import ILQR, QuadraticCost

    ROW = "AC_ERR_BAD_ARG dt_row must be a control row without effect"
    BOX = "AC_ERR_BAD_ARG the time row's lower bound"
    z = lambda *s: torch.zeros(s, device=gpu)  # noqa: E731

    def args(key, B=5):
        c = context(key)
        H = c["H"]
        return (dev(c["X0"][:, :B], gpu), z(H + 1, 13, B), dev(c["U"][:, :, :B], gpu), z(H, 7, 13, B), z(H, 7, B))

    def solver(key, dt_bounds=(0.005, 0.02)):
        c = context(key)
        return ILQR(system=c["ac"], dt=DT, num_nodes=c["H"], cost=QuadraticCost(), time="variable", dt_bounds=dt_bounds)

    il = solver("default")
    il.forward(*args("default"), alphas=[1.0])  # accepted as built
    il.cost.dt_row = 1                          # the elevator
    with pytest.raises(AircraftHipError, match=ROW):
        il.forward(*args("default"), alphas=[1.0])
    with pytest.raises(AircraftHipError, match=BOX):
        solver("default", dt_bounds=(0.0, 0.02)).forward(*args("default"), alphas=[1.0])
    il = solver("quad")
    assert il.time_row == 4
    il.forward(*args("quad"), alphas=[1.0])     # accepted as built
    il.cost.dt_row = 3                          # the fourth rotor
    with pytest.raises(AircraftHipError, match=ROW):
        il.forward(*args("quad"), alphas=[1.0])
