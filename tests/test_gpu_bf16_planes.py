"""The width-128 sensitivity kernels run their hidden layers on bf16 MFMA with three-plane operands (MlpEngine::layer_bf,
DESIGN.md §4.3).  16 384 + 100 units of the headline net (5-128-128-128-128-6): one full round through k_nn_step_sens and a
remainder through k_nn_step_sens_pair, every unit's x+ / A / B against the float64 oracle."""
import numpy as np
import pytest

from tests.helpers import block_rel_err, make_aircraft, make_oracle, synthetic_units, unit_max_rel

pytestmark = pytest.mark.gpu


def test_bf16_hidden_layers_every_unit_against_the_oracle(gpu):
    import torch

    ac = make_aircraft("nn", hidden=(128, 128, 128, 128), normalise=True)
    n = 16384 + 100
    X, U = synthetic_units(n, seed=5)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(gpu)
    Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(gpu)
    F, A, Bm, c = (t.cpu().numpy() for t in ac.step_sens(Xd, Ud, 0.01))
    Fr, Ar, Br, cr = make_oracle(ac).step_sens(X.astype(np.float32).astype(np.float64), U.astype(np.float32).astype(np.float64), 0.01)
    # every unit on its own: x+ (max over the state block), A and B (max norm over the unit's block)
    eF = float(block_rel_err(F, Fr))
    eA = float(unit_max_rel(A, Ar).max())
    eB = float(unit_max_rel(Bm, Br).max())
    print(f"bf16 hidden layers: F {eF:.2e} A {eA:.2e} B {eB:.2e}")
    assert eF < 5e-6 and eA < 5e-6 and eB < 5e-6, (eF, eA, eB)
    # c = dF/ddt, every unit, at the suite's line for it (SENS_TOL, tests/test_gpu_parity.py).  (The per-block bar of tests/test_gpu_plane_routes.py is not taken here: at this
    # dt = 0.01 the fp32 format of A's diagonal alone puts e_ref of the (v, v) and (omega, omega) blocks above its cap — see
    # tests/sens_blocks_ref.py::DT.)
    ec = float(unit_max_rel(c, cr).max())
    print(f"bf16 hidden layers: c {ec:.2e}")
    assert ec < 1e-5, ec
    # the remainder (k_nn_step_sens_pair) computes the same bits as the one-wave kernel
    tail = slice(16384, n)
    F2, A2, B2, c2 = ac.step_sens(Xd[:, tail].contiguous(), Ud[:, tail].contiguous(), 0.01)
    assert ac.last_launch()[0] == "k_nn_step_sens_pair"
    assert np.array_equal(F2.cpu().numpy(), F[:, tail]) and np.array_equal(A2.cpu().numpy(), A[..., tail])
    assert np.array_equal(B2.cpu().numpy(), Bm[..., tail])
