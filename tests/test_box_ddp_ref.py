"""The NumPy restatement of the box-constrained Riccati pass (tests/box_ddp_ref.py) checked on the CPU: the projected-Newton QP
against enumeration of the active sets, the recursion against the oracle when the box is far away, the mutations the metric has to
flag, and the conditions and the inventory of the cases the GPU tests run."""
import os

import numpy as np
import pytest

import ilqr_oracle as io
from tests import box_ddp_ref as bx
from tests import riccati_rate_ref as rr
from tests import riccati_ref as rf


# ---- 1. the QP against enumeration -----------------------------------------------------------------------------------------------------
def test_boxqp_matches_enumeration_of_the_active_sets():
    P = bx.qp_problems()
    assert bx.N_QPS >= 200
    counts, pinned, iters = set(), 0, 0
    for p in range(bx.N_QPS):
        (xe, ae), (x, a, it, capped) = P["enum"][p], P["f64"][p]
        assert not capped, p
        assert np.array_equal(a, ae), (p, a, ae)
        assert np.abs(x - xe).max() <= 1e-12 * max(1.0, np.abs(xe).max()), (p, np.abs(x - xe).max())
        assert (x >= P["lo"][p]).all() and (x <= P["hi"][p]).all()
        counts.add(int(((a == 1) | (a == -1)).sum()) if not (a == 2).any() else -1)
        pinned += int((a == 2).any())
        iters = max(iters, it)
    print("boxqp_np(float64):", bx.N_QPS, "problems, clamp counts", sorted(counts - {-1}), "problems with pinned rows", pinned,
          "most iterations", iters, "conditioned", int(P["conditioned"].sum()))
    assert {0, 7} <= counts and counts >= set(range(8)) and pinned >= 20
    assert iters <= 8
    assert P["conditioned"].sum() >= 150


def test_boxqp_fp32_restatement_keeps_the_active_set_on_conditioned_problems():
    P = bx.qp_problems()
    for p in np.flatnonzero(P["conditioned"]):
        x, a, it, capped = P["f32"][p]
        assert not capped and np.array_equal(a, P["enum"][p][1]), p
        cl = a != 0
        bound = np.where(a == 1, P["hi"][p], P["lo"][p])
        assert np.array_equal(x[cl], bound[cl].astype(np.float32)), p      # exactly the bound


# ---- 2. far bounds: the oracle's recursion ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(bx.VARIANTS))
def test_wide_box_equals_the_unboxed_reference(variant):
    c = bx.wide_case(variant, bx.PARENT_B, 23)
    inp = c["inp"]
    got = bx.run_np(np.float64, inp, c["rate"])
    assert not got["act"].any() and not got["stat"][1].any() and got["stat"][0].max() == 1
    if c["rate"] is None:   # tie to the oracle itself, not only to riccati_ref's copy of it
        K, kff, dV = io.backward(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"], uglin=inp["uglin"])
        ref = dict(K=K, kff=kff, dV=dV, Kp=None)
    else:
        K, Kp, kff, dV, _ = rr.backward_rate_np(np.float64, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], c["rate"][0],
                                                c["rate"][1], node=inp["node"], Hz=inp["Hz"])
        ref = dict(K=K, kff=kff, dV=dV, Kp=Kp)
    worst = max(rf.node_rel(got["K"], ref["K"]).max(), rf.node_rel(got["kff"], ref["kff"]).max(), rf.row_rel(got["dV"], ref["dV"]).max())
    if ref["Kp"] is not None:
        worst = max(worst, rf.node_rel(got["Kp"], ref["Kp"]).max())
    print(f"wide box {variant}: worst (node, instance) {worst:.2e}")
    assert worst <= 1e-12


# ---- 3. mutations ------------------------------------------------------------------------------------------------------------------------
def _errors(got, ref):
    e = [rf.node_rel(got["K"], ref["K"]), rf.node_rel(got["kff"], ref["kff"])]
    if ref["Kp"] is not None:
        e.append(rf.node_rel(got["Kp"], ref["Kp"]))
    return np.max(e, axis=0)   # (H, B)


@pytest.mark.parametrize("variant", ["goal", "rate_node_newton"])
@pytest.mark.parametrize("mutation", ["keep_K", "clip", "delta", "abs_bounds"])
def test_metric_flags_mutation(variant, mutation):
    c = bx.box_case(variant, "sym", bx.PARENT_B, 2 * rf.k_depth(True) + 1)
    bar = rf.FACTOR * c["e32"]
    bad = bx.run_np(np.float64, c["inp"], c["rate"], mutation=mutation)
    e = _errors(bad, c["ref"])
    print(f"{variant} {mutation}: {(e > bar).sum()} of {e.size} (node, instance) beyond the bar {bar:.1e}, worst {e.max():.2e}")
    assert (e > bar).any()
    if mutation in ("clip", "delta", "abs_bounds"):
        assert not np.array_equal(bad["act"], c["ref"]["act"])


# ---- 4. case conditions and inventory ------------------------------------------------------------------------------------------------
CASES = bx.matrix()


def test_committed_seeds_cover_the_matrix():
    assert set(bx.SEEDS) == set(CASES)


@pytest.mark.parametrize("variant,family,B,H", CASES, ids=[f"{v}-{f}-B{B}-H{H}" for v, f, B, H in CASES])
def test_case_conditions(variant, family, B, H):
    c = bx.box_case(variant, family, B, H)   # asserts the conditions on the float64 reference and the fp32 restatement
    fig = c["fig"]
    assert fig["margin_g"] >= bx.MARGIN and fig["margin_x"] >= bx.MARGIN and fig["same_act"] and fig["e32"] <= rf.E32_MAX
    assert fig["capped"] == 0
    U, cost = c["inp"]["U"], c["inp"]["cost"]
    assert (U >= np.asarray(cost.u_min)[None, :, None]).all() and (U <= np.asarray(cost.u_max)[None, :, None]).all()
    act = c["ref"]["act"]
    assert act.shape == (H, 7, B)           # every instance: none excluded
    if family == "pinned":
        assert (act[:, list(bx.PINNED_ROWS)] == 2).all() and not (np.delete(act, bx.PINNED_ROWS, axis=1) == 2).any()
    else:
        assert not (act == 2).any()
    if H > 1:   # a node whose active set differs from its neighbour's
        assert (act[1:] != act[:-1]).any(axis=(1, 2)).any()
    # the committed seed IS what the committed search returns; a wide case takes up to five minutes to search, so it is re-derived
    # on request only (BOX_DDP_RESEARCH_WIDE=1) — its conditions are asserted above in every run
    if B == bx.PARENT_B or os.environ.get("BOX_DDP_RESEARCH_WIDE") == "1":
        assert bx.find_seed(variant, family, B, H)[0] == bx.SEEDS[(variant, family, B, H)]


def test_case_inventory():
    counts, lower, upper, pinned = set(), np.zeros(7, bool), np.zeros(7, bool), False
    for key in CASES:
        if key[2] != bx.PARENT_B:
            continue
        act = bx.box_case(*key)["ref"]["act"]
        counts |= set(((act == 1) | (act == -1)).sum(axis=1).ravel().tolist())
        lower |= (act == -1).any(axis=(0, 2)); upper |= (act == 1).any(axis=(0, 2))
        pinned |= bool((act == 2).any())
    assert counts >= set(range(8)), counts
    assert lower.all() and upper.all() and pinned
