"""The one-wave f16 sensitivity kernel streams its hidden layers through a four-region ring (two slots of a whole layer, one
workgroup barrier per hidden layer, the next layer requested piece by piece in the gaps of slabs 2 to 4: MlpEngine::acquire,
DESIGN.md §4.3); the wave-pair kernel keeps the two-region ring.  Nets with 1 to 4 streamed width-128 layers, the f16 route
forced, every unit bit-identical to the same handle's pair kernel and within 5e-6 of the float64 oracle.

How each kernel is reached through the product dispatch (ac_step_sens_f32; the library reads no environment): a batch of at
most half a round (32 units per CU) goes to k_nn_step_sens_pair alone, so the pair-only reference is the batch run in such
chunks; whole rounds go to k_nn_step_sens.  With R = 64 x CUs units to a round:
  * 16 384 + 100 units — on a 256-CU card one whole round for the one-wave kernel and the remainder for the pair kernel;
  * 100 units — a single partial task (the dispatcher hands it to the pair kernel);
  * 2 R + R / 2 + 100 units — more than half a round left over, so ALL of it runs on the one-wave kernel: two or three tasks
    to a workgroup (the ring wraps across task boundaries, with both slot parities for odd layer counts) and a partial last
    task."""
import numpy as np
import pytest

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
from tests.helpers import GLIDER, block_rel_err, make_aircraft, make_oracle, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

KIB = 1024
EDGE = 8 * KIB                                  # first and last layer blocks of plan_sens at width 128
LDS_RING4 = EDGE + 4 * 33 * KIB                 # 140 KiB
LDS_BF16 = EDGE + 3 * 49 * KIB                  # the bf16 route's three regions, as before
LDS_F16_PAIR = EDGE + 2 * 33 * KIB + 2 * 8 * KIB + 2 * 16 * 36 * 4  # two regions + the pairs' exchanges, as before
STREAMED = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def cus(gpu):
    import torch

    return torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.fixture(scope="module")
def units(gpu, cus):
    import torch

    n = max(16384 + 100, 2 * 64 * cus + 32 * cus + 100)
    X, U = synthetic_units(n, seed=11)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(gpu)
    Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(gpu)
    return X, U, Xd, Ud


def run(ac, Xd, Ud):
    return tuple(t.cpu().numpy() for t in ac.step_sens(Xd, Ud, 0.01))


def run_pair_only(ac, Xd, Ud, cus):
    """The batch through k_nn_step_sens_pair alone: chunks of at most half a round."""
    half, n = 32 * cus, Xd.shape[1]
    parts = []
    for k in range(0, n, half):
        parts.append(run(ac, Xd[:, k:k + half].contiguous(), Ud[:, k:k + half].contiguous()))
        assert ac.last_launch()[0] == "k_nn_step_sens_pair" and ac.last_launch()[3] == LDS_F16_PAIR
    return tuple(np.concatenate([p[i] for p in parts], axis=-1) for i in range(4))


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("streamed", STREAMED)
def test_ring4_against_the_pair_kernel_and_the_oracle(units, cus, streamed):
    X, U, Xd, Ud = units
    ac = make_aircraft("nn", hidden=(128,) * (streamed + 1), normalise=True)
    ac.hidden_route = "f16"
    orc = make_oracle(ac)
    R = 64 * cus
    for n in (16384 + 100, 100, 2 * R + R // 2 + 100):
        rem = n % R
        one_wave = (n - rem if 0 < rem <= R // 2 else n) > 0  # the dispatcher's rule: whole rounds to the one-wave kernel
        Xs, Us = Xd[:, :n].contiguous(), Ud[:, :n].contiguous()
        out = run(ac, Xs, Us)
        assert ac.hidden_route_in_use() == ("f16", 0)
        name, grid, block, lds = ac.last_launch()
        if one_wave:
            assert (name, block, lds) == ("k_nn_step_sens", 256, LDS_RING4), (name, grid, block, lds)
        else:
            assert (name, lds) == ("k_nn_step_sens_pair", LDS_F16_PAIR)
        if n == 2 * R + R // 2 + 100:
            assert grid == cus and -(-n // 64) > 2 * grid and n % 64 != 0  # two or three tasks each, a partial last task
        assert same(run(ac, Xs, Us), out), f"n = {n}: repeats differ"
        assert same(run_pair_only(ac, Xs, Us, cus), out), f"n = {n}: one-wave and pair kernels differ"
        if n <= 16384 + 100:  # (the third batch is the same units again and more of them: the pair kernel ties it to these)
            Fr, Ar, Br, cr = orc.step_sens(X[:, :n].astype(np.float32).astype(np.float64),
                                           U[:, :n].astype(np.float32).astype(np.float64), 0.01)
            F, A, Bm, c = out
            eF, eA, eB = float(block_rel_err(F, Fr)), float(unit_max_rel(A, Ar).max()), float(unit_max_rel(Bm, Br).max())
            print(f"{streamed} streamed, n = {n} ({name}): F {eF:.2e} A {eA:.2e} B {eB:.2e}")
            assert eF < 5e-6 and eA < 5e-6 and eB < 5e-6, (eF, eA, eB)


def test_a_net_the_gate_rejects_launches_as_before(units, cus):
    X, U, Xd, Ud = units
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    W = [w.copy() for w in syn.weights]
    W[0] = W[0] * np.float32(2.0 ** -20)  # uniformly tiny tangents: the gate's verdict 3 (tests/test_gpu_f16_planes.py)
    net = MlpData(W, syn.biases, syn.act, syn.input_mean, syn.input_std, syn.output_mean, syn.output_std)
    opts = AircraftOpts(coeff_model_type="nn", coeff_model_path=net, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                        physical_integration_substeps=1, use_mfma=True)
    ac = Aircraft(opts)
    ac.normalise = True
    n = 64 * cus + 100
    ac.step_sens(Xd[:, :n].contiguous(), Ud[:, :n].contiguous(), 0.01)
    assert ac.hidden_route_in_use() == ("bf16", 3)
    assert ac.last_launch() == ("k_nn_step_sens", cus, 256, LDS_BF16)
