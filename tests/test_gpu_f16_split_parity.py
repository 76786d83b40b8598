"""The two f16 sensitivity kernels at the smallest batches that reach each of them, the route forced to f16 on the headline net
(5-128-128-128-128-6): 100 units (k_nn_step_sens_pair alone) and 64 x CUs + 100 units (one whole round of k_nn_step_sens over
the chip and the remainder through the pair kernel).  Against the float64 oracle at the tolerances of tests/test_gpu_f16_planes.py
(5e-6 on F, A, B; 1e-5 on c); the pair kernel computes the bits of the one-wave kernel — the same units are also run inside a
batch of exactly one round, which has no remainder; repeats are bit-identical."""
import numpy as np
import pytest

from tests.helpers import block_rel_err, make_aircraft, make_oracle, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu

REM = 100


def run(ac, Xd, Ud):
    return tuple(t.cpu().numpy() for t in ac.step_sens(Xd, Ud, 0.01))


def same(a, b, sl=slice(None)):
    return all(np.array_equal(x[..., sl], y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def case(gpu):
    import torch

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = 64 * cus + REM
    X, U = synthetic_units(n, seed=11)
    X, U = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(U, dtype=np.float32)
    ac = make_aircraft("nn", hidden=(128, 128, 128, 128), normalise=True)
    ac.hidden_route = "f16"
    ref = make_oracle(ac).step_sens(X.astype(np.float64), U.astype(np.float64), 0.01)  # once, shared, read-only
    for r in ref:
        r.setflags(write=False)
    return ac, cus, n, torch.from_numpy(X).to(gpu), torch.from_numpy(U).to(gpu), ref


def against_oracle(out, ref, sl, what):
    (F, A, Bm, c), (Fr, Ar, Br, cr) = out, (r[..., sl] for r in ref)
    eF, eA, eB = float(block_rel_err(F, Fr)), float(unit_max_rel(A, Ar).max()), float(unit_max_rel(Bm, Br).max())
    ec = float(unit_max_rel(c, cr).max())
    print(f"{what}: F {eF:.2e} A {eA:.2e} B {eB:.2e} c {ec:.2e}")
    assert eF < 5e-6 and eA < 5e-6 and eB < 5e-6, (eF, eA, eB)
    assert ec < 1e-5, ec


def test_pair_kernel_alone(case):
    ac, cus, n, Xd, Ud, ref = case
    head = slice(0, REM)
    out = run(ac, Xd[:, head].contiguous(), Ud[:, head].contiguous())
    assert ac.hidden_route_in_use() == ("f16", 0)
    assert ac.last_launch()[0] == "k_nn_step_sens_pair"
    against_oracle(out, ref, head, f"{REM} units, pair kernel")
    # the same units inside exactly one round: the one-wave kernel, no remainder
    rnd = slice(0, 64 * cus)
    one = run(ac, Xd[:, rnd].contiguous(), Ud[:, rnd].contiguous())
    assert ac.last_launch()[:2] == ("k_nn_step_sens", cus)
    assert same(one, out, head), "pair kernel != one-wave kernel"
    assert same(run(ac, Xd[:, head].contiguous(), Ud[:, head].contiguous()), out), "repeat differs"


def test_one_round_and_the_pair_remainder(case):
    ac, cus, n, Xd, Ud, ref = case
    out = run(ac, Xd, Ud)
    assert ac.hidden_route_in_use() == ("f16", 0)
    assert ac.last_launch()[:2] == ("k_nn_step_sens", cus)  # (the main kernel's launch is the one kept; the remainder follows it)
    against_oracle(out, ref, slice(None), f"{n} units, one round + pair remainder")
    # the remainder's units through the one-wave kernel: the last REM of a batch of exactly one round
    rnd = slice(REM, n)
    one = run(ac, Xd[:, rnd].contiguous(), Ud[:, rnd].contiguous())
    assert ac.last_launch()[:2] == ("k_nn_step_sens", cus)
    tail = tuple(x[..., 64 * cus:] for x in out)
    assert same(one, tail, slice(64 * cus - REM, None)), "pair remainder != one-wave kernel"
    # ... and the round's units do not depend on where in the batch they stand
    assert same(out, tuple(x[..., :64 * cus - REM] for x in one), slice(REM, 64 * cus))
    assert same(run(ac, Xd, Ud), out), "repeat differs"
