"""CPU tests of the Riccati test infrastructure (tests/riccati_ref.py): the fp32 restatement meets the e32 condition on every
case the GPU matrix runs, the per-node metric flags each kind of mistake exactly where that mistake can reach, and the
whole-tensor norm the suite used before misses a stale node that the per-node bar catches."""
import numpy as np
import pytest

import ilqr_oracle as io
from tests import riccati_ref as rr
from tests.helpers import make_oracle, rel_fro


def test_float64_restatement_is_the_oracle():
    """backward_np is the recursion of io.backward: in float64 they agree to rounding (this is what licenses its Quu
    eigenvalues and, in float32, its e32)."""
    for v in rr.VARIANTS:
        c = rr.riccati_case(v, rr.PARENT_B, 11)
        i = c["inp"]
        K, kff, dV, _ = rr.backward_np(np.float64, i["cost"], i["X"], i["U"], i["A"], i["Bm"], node=i["node"], Hz=i["Hz"], uglin=i["uglin"])
        assert rr.e32_of(c["ref"], (K, kff, dV)) < 1e-12


def test_matrix_covers_the_ring_edges():
    rows = rr.matrix()
    for v, (_, newton, _) in rr.VARIANTS.items():
        d = rr.k_depth(newton)
        hs = {H for vv, B, H in rows if vv == v and B == rr.PARENT_B}
        assert {1, 2, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 23} == hs
        assert [(B, H) for vv, B, H in rows if vv == v and B != rr.PARENT_B] == [(rr.WIDE_B, d + 1)]
    assert len(rows) == 5 * 10


@pytest.mark.parametrize("variant", list(rr.VARIANTS))
def test_fp32_restatement_meets_the_condition_on_every_matrix_case(variant):
    """e32 <= 1.25e-5 (so the bar 8 x e32 never exceeds 1e-4) and min eig Quu >= 0.3 on every row of the GPU matrix.
    Measured: e32 2.4e-7 .. 1.5e-6, smallest Quu eigenvalue 0.44."""
    worst, lo = 0.0, np.inf
    for v, B, H in rr.matrix():
        if v != variant:
            continue
        c = rr.riccati_case(v, B, H)
        assert 0 < c["e32"] <= rr.E32_MAX, (v, B, H, c["e32"])
        assert c["quu_min"] >= rr.QUU_MIN, (v, B, H, c["quu_min"])
        assert (c["ref"][2][0] < 0).all()          # a descent direction on every instance
        worst, lo = max(worst, c["e32"]), min(lo, c["quu_min"])
    print(f"riccati e32[{variant}] worst {worst:.3e}  min eig Quu {lo:.3f}")
    assert rr.FACTOR * worst <= 1e-4


def test_costate_restatement_meets_the_condition():
    for nodef in (False, True):
        for H in (1, 2, 9):
            c = rr.costate_parent(nodef, H)
            print(f"costate e32[node={nodef}, H={H}] {c['e32']:.3e}")
            assert 0 < c["e32"] <= rr.E32_MAX


# ---- the metric can fail, and only where the mistake can reach ----------------------------------------------------------
MB, MH, MK, MI = 5, 11, 6, 2   # batch, horizon, the node and the instance the local mutants touch


def _goal_case():
    return rr.riccati_case("goal", MB, MH)


def _mutants():
    """name -> (mutated inputs, reach mask (H, B) of (node, instance) pairs the change can move, touched nodes, kff only)"""
    base = _goal_case()["inp"]
    every = np.ones((MH, MB), dtype=bool)
    upto = np.zeros((MH, MB), dtype=bool); upto[:MK + 1] = True
    one = np.zeros((MH, MB), dtype=bool); one[:MK + 1, MI] = True

    def edit(**kw):
        m = dict(base)
        for k, f in kw.items():
            m[k] = f(np.array(base[k]))   # (a writable copy)
        return m

    def stale(k):
        def f(a):
            a[k] = a[k + 1]
            return a
        return f

    def neighbour(a):
        a[MK, :, :, MI] = a[MK, :, :, MI + 1]
        return a

    def zero_ux(a):
        a[:, 13:20, :13] = 0.0
        return a

    def zero_ug(a):
        a[MK] = 0.0
        return a

    def corner(a):
        a[:, 19, 19] *= 1.01
        return a

    import copy
    reg = dict(base); reg["cost"] = copy.deepcopy(base["cost"]); reg["cost"].reg = base["cost"].reg * 1.001
    return {
        "stale_node": (edit(A=stale(MK), Bm=stale(MK)), upto, [MK], False),
        "neighbour_instance": (edit(A=neighbour), one, [MK], False),
        "reg_x_1.001": (reg, every, range(MH), False),
        "Hz_ux_zeroed": (edit(Hz=zero_ux), every, range(MH), False),
        "uglin_node_zeroed": (edit(uglin=zero_ug), upto, [MK], True),
        "Hz_19_19_x_1.01": (edit(Hz=corner), every, range(MH), False),
    }


@pytest.mark.parametrize("name", ["stale_node", "neighbour_instance", "reg_x_1.001", "Hz_ux_zeroed", "uglin_node_zeroed",
                                  "Hz_19_19_x_1.01"])
def test_metric_flags_each_mutant_where_it_can_reach(name):
    """Each mistake, applied to the float64 oracle's inputs of a <NODE, NEWTON, uglin> case, is above 1e-4 — the largest bar
    the condition allows — on every instance it reaches at the node(s) it touches, and exactly zero at every (node, instance)
    it cannot reach (nodes after the touched one; other instances).  Measured, smallest per-instance figure at the touched
    node(s), in the order of the list: 1.1, 0.21, 3.2e-4, 0.18, 0.25, 3.9e-4 (printed by the test)."""
    case = _goal_case()
    mut, reach, nodes, kff_only = _mutants()[name]
    K, kff, dV = rr.reference(mut)
    eK, ek = rr.node_rel(K, case["ref"][0]), rr.node_rel(kff, case["ref"][1])
    e = ek if kff_only else np.maximum(eK, ek)
    if kff_only:
        assert not eK.any()                       # a control gradient moves no gain
    assert not e[~reach].any(), (name, "moved a (node, instance) it cannot reach", np.argwhere((e > 0) & ~reach)[:4])
    touched = e[list(nodes)]                      # (touched nodes, B)
    cols = reach[list(nodes)].any(axis=0)
    print(f"riccati mutant[{name}] worst {e.max():.3e}  smallest per-instance worst at the touched nodes {touched.max(axis=0)[cols].min():.3e}")
    assert (touched.max(axis=0)[cols] > 1e-4).all(), (name, touched.max(axis=0))
    # ... and check_riccati itself raises on it (the oracle's own result passes)
    rr.check_riccati(name, *case["ref"], case["ref"], case["f32"], quu_min=case["quu_min"], report=False)
    with pytest.raises(AssertionError):
        rr.check_riccati(name, K, kff, dV, case["ref"], case["f32"], report=False)


def test_whole_tensor_norm_misses_a_stale_node_that_the_per_node_bar_catches():
    """On the smooth glider inputs of test_gpu_ilqr.py::test_backward_pass_matches_numpy (B = 24, H = 30, poly; rebuilt here
    from the oracle's rollout and step_sens), node 10 reading node 11's A and B on every instance stays below the 2e-3 bar of
    the whole-tensor Frobenius norm in K, kff and dV — the old assertions pass — and is far above the per-node bar."""
    from tests.test_gpu_ilqr import setup

    ac, il, cost, X0, U = setup(None, "poly", None)
    orc = make_oracle(ac)
    H, B = U.shape[0], U.shape[2]
    X = rr.f32_exact(orc.rollout(X0, U, 0.01))
    flatX = np.ascontiguousarray(X[:H].transpose(1, 0, 2).reshape(13, -1)); flatU = np.ascontiguousarray(U.transpose(1, 0, 2).reshape(7, -1))
    _, A, Bm, _ = orc.step_sens(flatX, flatU, 0.01)
    A = rr.f32_exact(A.reshape(13, 13, H, B).transpose(2, 0, 1, 3)); Bm = rr.f32_exact(Bm.reshape(13, 7, H, B).transpose(2, 0, 1, 3))
    ref = io.backward(cost, X, U, A, Bm)
    f32 = rr.backward_f32(cost, X, U, A, Bm)
    e32 = rr.e32_of(ref, f32)
    bar = rr.bar_of(e32, "glider")
    As, Bs = A.copy(), Bm.copy()
    As[10], Bs[10] = A[11], Bm[11]
    K, kff, dV = io.backward(cost, X, U, As, Bs)
    fro = [rel_fro(K, ref[0]), rel_fro(kff, ref[1]), rel_fro(dV, ref[2])]
    per_node = max(rr.node_rel(K, ref[0]).max(), rr.node_rel(kff, ref[1]).max())
    print(f"glider stale node: Frobenius K {fro[0]:.2e} kff {fro[1]:.2e} dV {fro[2]:.2e}; per node {per_node:.2e}; e32 {e32:.2e} bar {bar:.2e}")
    assert max(fro) < 2e-3                        # the old assertions do not see it
    assert per_node > 1e-4 > bar                  # the new one does, at any bar the condition allows
    with pytest.raises(AssertionError):
        rr.check_riccati("glider-stale", K, kff, dV, ref, f32, report=False)
