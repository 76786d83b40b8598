"""The width-128 sensitivity kernels run their hidden layers on two-plane f16 MFMA where the net passes the range gate
(MlpEngine::layer_bf, f16 form), with the three-plane bf16 kernels as the fall-back.  16 384 + 100 units of the
headline net (5-128-128-128-128-6): one full round through k_nn_step_sens and a remainder through k_nn_step_sens_pair, the
route forced in turn on one handle each."""
import numpy as np
import pytest

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
from tests.helpers import GLIDER, block_rel_err, make_aircraft, make_oracle, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

N = 16384 + 100


def routed(route, hidden=(128, 128, 128, 128)):
    ac = make_aircraft("nn", hidden=hidden, normalise=True)
    ac.hidden_route = route
    return ac


def run(ac, Xd, Ud):
    return tuple(t.cpu().numpy() for t in ac.step_sens(Xd, Ud, 0.01))


@pytest.fixture(scope="module")
def units(gpu):
    import torch

    X, U = synthetic_units(N, seed=5)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(gpu)
    Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(gpu)
    return X, U, Xd, Ud


def unit_err_F(F, Fr):
    """x+ per unit, the metric of block_rel_err taken column by column  -> (n,)"""
    return np.array([block_rel_err(F[:, k:k + 1], Fr[:, k:k + 1]) for k in range(F.shape[1])])


def test_f16_hidden_layers_every_unit_against_the_oracle_and_against_bf16(units):
    X, U, Xd, Ud = units
    af, ab = routed("f16"), routed("bf16")
    F, A, Bm, c = run(af, Xd, Ud)
    assert af.hidden_route_in_use() == ("f16", 0)
    assert af.last_launch()[0] == "k_nn_step_sens"
    lds_f16 = af.last_launch()[3]
    Fb, Ab, Bb, cb = run(ab, Xd, Ud)
    assert ab.hidden_route_in_use() == ("bf16", 0) and ab.last_launch()[3] > lds_f16  # 3 x 49 KiB regions against 3 x 33
    Fr, Ar, Br, cr = make_oracle(af).step_sens(X.astype(np.float32).astype(np.float64), U.astype(np.float32).astype(np.float64), 0.01)
    eF, eA, eB = float(block_rel_err(F, Fr)), unit_max_rel(A, Ar), unit_max_rel(Bm, Br)
    bF, bA, bB = float(block_rel_err(Fb, Fr)), unit_max_rel(Ab, Ar), unit_max_rel(Bb, Br)
    print(f"f16 hidden layers:  F {eF:.2e} A {eA.max():.2e} B {eB.max():.2e}")
    print(f"bf16 hidden layers: F {bF:.2e} A {bA.max():.2e} B {bB.max():.2e}")
    assert eF < 5e-6 and eA.max() < 5e-6 and eB.max() < 5e-6, (eF, eA.max(), eB.max())
    # c = dF/ddt of both routes, every unit, at the suite's line for it (SENS_TOL, tests/test_gpu_parity.py).  (The per-block bar
    # of tests/test_gpu_plane_routes.py is not taken here: at this dt = 0.01 the fp32 format of A's diagonal alone puts e_ref of
    # the (v, v) and (omega, omega) blocks above its cap — see tests/sens_blocks_ref.py::DT.)
    ec, bc = float(unit_max_rel(c, cr).max()), float(unit_max_rel(cb, cr).max())
    print(f"c: f16 {ec:.2e} bf16 {bc:.2e}")
    assert ec < 1e-5 and bc < 1e-5, (ec, bc)
    # f16 against bf16, unit by unit: no further apart than the two routes' own measured errors against the oracle allow
    dA, dB = unit_max_rel(A, Ab), unit_max_rel(Bm, Bb)
    sA = (eA + bA) * np.abs(Ar).reshape(-1, N).max(axis=0) / np.abs(Ab).reshape(-1, N).max(axis=0)
    sB = (eB + bB) * np.abs(Br).reshape(-1, N).max(axis=0) / np.abs(Bb).reshape(-1, N).max(axis=0)
    print(f"f16 against bf16: A {dA.max():.2e} B {dB.max():.2e} (worst ratio to the bound {np.max(dA / sA):.2f} / {np.max(dB / sB):.2f})")
    assert (dA <= sA * (1 + 1e-12)).all() and (dB <= sB * (1 + 1e-12)).all()
    dF = np.abs(F.astype(np.float64) - Fb.astype(np.float64))
    assert (dF <= np.abs(F - Fr) + np.abs(Fb - Fr)).all()
    # the remainder (k_nn_step_sens_pair) computes the same bits as the one-wave kernel
    tail = slice(16384, N)
    F2, A2, B2, c2 = run(af, Xd[:, tail].contiguous(), Ud[:, tail].contiguous())
    assert af.last_launch()[0] == "k_nn_step_sens_pair"
    assert np.array_equal(F2, F[:, tail]) and np.array_equal(A2, A[..., tail]) and np.array_equal(B2, Bm[..., tail])
    assert np.array_equal(c2, c[..., tail])
    # repeats are bit-identical
    F3, A3, B3, c3 = run(af, Xd, Ud)
    assert np.array_equal(F3, F) and np.array_equal(A3, A) and np.array_equal(B3, Bm) and np.array_equal(c3, c)
    # "auto" takes the f16 route on this net: the same bits
    F4, A4, B4, c4 = run(routed("auto"), Xd, Ud)
    assert np.array_equal(F4, F) and np.array_equal(A4, A) and np.array_equal(B4, Bm)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_f16_small_batches(units, n):
    X, U, Xd, Ud = units
    af, ab = routed("f16"), routed("bf16")
    F, A, Bm, c = run(af, Xd[:, :n].contiguous(), Ud[:, :n].contiguous())
    Fr, Ar, Br, cr = make_oracle(af).step_sens(X[:, :n].astype(np.float32).astype(np.float64), U[:, :n].astype(np.float32).astype(np.float64), 0.01)
    eF, eA, eB = float(block_rel_err(F, Fr)), float(unit_max_rel(A, Ar).max()), float(unit_max_rel(Bm, Br).max())
    print(f"n = {n} ({af.last_launch()[0]}): F {eF:.2e} A {eA:.2e} B {eB:.2e}")
    assert eF < 5e-6 and eA < 5e-6 and eB < 5e-6, (eF, eA, eB)


def rejected_net():
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    W = [w.copy() for w in syn.weights]
    W[0] = W[0] * np.float32(2.0 ** -20)  # uniformly tiny tangents: the gate's verdict 3
    return MlpData(W, syn.biases, syn.act, syn.input_mean, syn.input_std, syn.output_mean, syn.output_std)


def aircraft_of(net, route):
    opts = AircraftOpts(coeff_model_type="nn", coeff_model_path=net, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                        physical_integration_substeps=1, use_mfma=True)  # (as tests.helpers.make_aircraft)
    ac = Aircraft(opts)
    ac.normalise = True
    ac.hidden_route = route
    return ac


def test_a_net_the_gate_rejects_runs_the_bf16_kernels(units):
    X, U, Xd, Ud = units
    n = 4096 + 100
    Xs, Us = Xd[:, :n].contiguous(), Ud[:, :n].contiguous()
    net = rejected_net()
    auto, forced = aircraft_of(net, "auto"), aircraft_of(net, "bf16")
    Fa, Aa, Ba, ca = run(auto, Xs, Us)
    assert auto.hidden_route_in_use() == ("bf16", 3)
    la = auto.last_launch()
    Fb, Ab, Bb, cb = run(forced, Xs, Us)
    assert forced.last_launch() == la
    # ... which is the launch (kernel, grid, block, the bf16 ring's LDS size) of the headline net forced to bf16, not the f16 one
    ref, f16 = routed("bf16"), routed("f16")
    ref.step_sens(Xs, Us, 0.01)
    f16.step_sens(Xs, Us, 0.01)
    assert la == ref.last_launch() and la[3] > f16.last_launch()[3]
    assert np.array_equal(Fa, Fb) and np.array_equal(Aa, Ab) and np.array_equal(Ba, Bb) and np.array_equal(ca, cb)
    # forcing f16 on it is an error, not a fall-back
    bad = aircraft_of(net, "f16")
    with pytest.raises(Exception, match="hidden route f16"):
        bad.step_sens(Xs, Us, 0.01)
