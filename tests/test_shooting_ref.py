"""CPU checks of tests/shooting_ref.py, the float64 reference of the multiple-shooting kernels:
 1. with F = X[1:] (zero gaps) the restatement IS the single-shooting backward pass of oracle/ilqr_oracle.py;
 2. (dX, dU, lam) equal ONE dense KKT solve of the iteration's QP, for all five variants, with indefinite Hz and dx_0 != 0;
 3. three mutations of the recursion each leave the GPU bar (8 x e32) on every case of the GPU matrix's parent batch."""
import numpy as np
import pytest

import ilqr_oracle as io
from tests import riccati_ref as rf
from tests import shooting_ref as sr

# float64 against float64 of a different operation order (Cholesky + triangular solves against np.linalg.solve, batched matmul
# against per-instance products): the issue measured 2e-13 at these sizes; 1e-11 leaves room for other seeds and is eight orders
# below any effect of the defect terms
ZERO_GAP_BOUND = 1e-11
KKT_BOUND = 1e-9


@pytest.mark.parametrize("variant", list(rf.VARIANTS))
def test_zero_gaps_is_the_single_shooting_pass(variant):
    worst = 0.0
    for H in (1, 9, 23):
        inp = sr.shoot_inputs(variant, 7, H, 31 + H, gap=0.0)
        assert np.array_equal(inp["F"], inp["X"][1:])
        got = sr.run_np(np.float64, inp)
        K, kff, dV = io.backward(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"], uglin=inp["uglin"])
        e = max(rf.node_rel(got["K"], K).max(), rf.node_rel(got["kff"], kff).max(), rf.row_rel(got["dV"], dV).max())
        worst = max(worst, float(e))
        # and riccati_ref's own restatement, bit for bit in float64 (the same operations)
        K2, k2, dV2, _ = rf.backward_np(np.float64, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"],
                                        uglin=inp["uglin"])
        assert np.array_equal(got["K"], K2) and np.array_equal(got["kff"], k2) and np.array_equal(got["dV"], dV2)
    print(f"zero gaps vs io.backward [{variant}]: worst {worst:.2e}")
    assert worst <= ZERO_GAP_BOUND


@pytest.mark.parametrize("variant", list(rf.VARIANTS))
@pytest.mark.parametrize("H", [1, 2, 5, 6])
def test_direction_and_multipliers_equal_the_dense_kkt_solve(variant, H):
    B = 3
    inp = sr.shoot_inputs(variant, B, H, 77 + H)
    if inp["Hz"] is not None:
        assert min(np.linalg.eigvalsh(inp["Hz"][k, :, :, b]).min() for k in range(H) for b in range(B)) < 0   # indefinite
    bw = sr.run_np(np.float64, inp)
    dx0 = np.random.default_rng(5).normal(size=(13, B))
    worst = 0.0
    for zero in (True, False):
        d0 = None if zero else dx0
        dX, dU, Lam = sr.direction_np(np.float64, inp["X"], inp["F"], inp["A"], inp["Bm"], bw["K"], bw["kff"], bw["Vx"], bw["Vxx"], dx0=d0)
        for b in range(B):
            kX, kU, kL = sr.kkt_np(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], inp["F"], b, node=inp["node"], Hz=inp["Hz"],
                                   uglin=inp["uglin"], dx0=None if zero else dx0[:, b])
            for got, ref in ((dX[:, :, b], kX), (dU[:, :, b], kU), (Lam[:, :, b], kL)):
                worst = max(worst, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)))
    print(f"KKT [{variant} H={H}]: worst {worst:.2e}")
    assert worst <= KKT_BOUND
    assert (dX[0] == dx0).all()


@pytest.mark.parametrize("mutation", [m for m in sr.MUTATIONS if m])
def test_mutations_leave_the_gpu_bar(mutation):
    """every case of the GPU matrix at the parent batch: a wrong recursion is beyond 8 x e32 in kff (and the multipliers' inputs)"""
    for variant, B, H in rf.matrix():
        if B != rf.PARENT_B:
            continue
        c = sr.shoot_case(variant, B, H)
        bar = rf.bar_of(c["e32"], f"{variant}-H{H}")
        mut = sr.run_np(np.float64, c["inp"], mutation=mutation)
        e = max(v.max() for v in sr.errors(mut, c["ref"]).values())
        assert e > 100 * bar, (mutation, variant, H, e, bar)


def test_case_conditions_of_the_gpu_matrix():
    worst = 0.0
    for variant, B, H in rf.matrix():
        if B != rf.PARENT_B:
            continue
        c = sr.shoot_case(variant, B, H)
        assert c["e32"] <= rf.E32_MAX and c["quu_min"] >= rf.QUU_MIN, (variant, H, c["e32"], c["quu_min"])
        worst = max(worst, c["e32"])
    print(f"e32 of the fp32 restatement over the parent-batch matrix: worst {worst:.2e}")


def test_merit_pieces():
    rng = np.random.default_rng(3)
    R = rng.normal(size=(4, 13, 6)); J = rng.normal(size=6); mu = np.array([1.0, 3.0])
    phi, dinf, sabs = sr.merit_np(np.float64, J, mu, R)
    assert np.allclose(phi, J + np.tile(mu, 3) * np.abs(R).sum(axis=(0, 1))) and np.array_equal(dinf, np.abs(R).max(axis=(0, 1)))
    assert (sabs >= np.abs(phi)).all()
    m = sr.merit_weight_f32(np.array([1.0, 50.0], np.float32), rng.normal(size=(4, 13, 2)).astype(np.float32), 2.0)
    assert m[1] == 50.0 and m[0] > 1.0
