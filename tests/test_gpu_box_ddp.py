"""The box-constrained Riccati kernels k_ilqr_backward<NODE, NEWTON, true> and k_ilqr_backward_rate<NODE, NEWTON, true>
(aircraft_amd/csrc/ilqr_backward_inst.hip) against the float64 restatement of tests/box_ddp_ref.py, and ILQR(box="qp") end to end.

Matrix: the five ways the plain kernel is fed and the four rate kernels, B = 7 at H in {1, 2, kDepth + 1, 2 kDepth + 1}, B = 65 at
H = kDepth + 1, a symmetric box and one with rows 3-5 pinned.  Per case: the active set equal to the reference's everywhere; every
(node, instance) of K, kff, Kp and every dV entry within 8 x the error of the fp32 restatement on the same inputs; rows of K / Kp at
clamped and pinned controls bitwise +0.0f; kff there bitwise fl32(bound - U_k); no QP at a cap.  Nothing is excluded."""
import numpy as np
import pytest

from tests import box_ddp_ref as bx
from tests import riccati_ref as rf
from tests.helpers import make_aircraft, parity_report
from tests.test_gpu_riccati import assert_guards, bits_equal, dev, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ac(gpu):
    return make_aircraft("poly")


def run_box(ac, gpu, inp, rate):
    """One launch through ILQR.backward(box=True) on float32 copies; guarded float outputs; inputs bit-unchanged
    -> dict of host arrays K, kff, dV, Kp (or None), act, stat"""
    import torch
    from aircraft_amd.control import ILQR

    H, _, B = inp["U"].shape
    il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=inp["cost"], box="qp")
    t = {k: dev(inp[k], gpu) for k in ("X", "U", "A", "Bm")}
    for k in ("Hz", "uglin"):
        t[k] = dev(inp[k], gpu) if inp[k] is not None else None
    if rate is not None:
        t["g"], t["h"] = dev(rate[0], gpu), dev(rate[1], gpu)
    node = None if inp["node"] is None else tuple(dev(a, gpu) for a in inp["node"])
    before = {k: v.clone() for k, v in t.items() if v is not None}
    bufs = {"K": guarded((H, 7, 13, B), gpu), "kff": guarded((H, 7, B), gpu), "dV": guarded((2, B), gpu)}
    if rate is not None:
        bufs["Kp"] = guarded((H, 7, 7, B), gpu)
    PADB = 64
    actbuf = torch.full((H * 7 * B + 2 * PADB,), 99, dtype=torch.int8, device=gpu)
    statbuf = torch.full((2 * B + 2 * PADB,), -77, dtype=torch.int32, device=gpu)
    act, stat = actbuf[PADB:PADB + H * 7 * B].view(H, 7, B), statbuf[PADB:PADB + 2 * B].view(2, B)
    out = tuple(bufs[k][1] for k in (("K", "kff", "dV", "Kp") if rate is not None else ("K", "kff", "dV"))) + (act, stat)
    res = il.backward(t["X"], t["U"], t["A"], t["Bm"], out=out, Hz=t["Hz"], node=node, uglin=t["uglin"],
                      rate=(t["g"], t["h"]) if rate is not None else None, box=True)
    torch.cuda.synchronize()
    assert ac.last_launch()[:3] == ("k_ilqr_backward_rate_box" if rate is not None else "k_ilqr_backward_box", B, 64)
    assert_guards(bufs, "backward_box")
    assert bool((actbuf[:PADB] == 99).all()) and bool((actbuf[-PADB:] == 99).all()) and bool((act != 99).all()), "act: padding / unwritten"
    assert bool((statbuf[:PADB] == -77).all()) and bool((statbuf[-PADB:] == -77).all()) and bool((stat != -77).all()), "stat: padding / unwritten"
    for k, v in before.items():
        assert bits_equal(t[k], v), (k, "input modified")
    assert len(res) == len(out)
    h = {k: bufs[k][1].cpu().numpy() for k in bufs}
    h.setdefault("Kp", None)
    h["act"], h["stat"] = act.cpu().numpy(), stat.cpu().numpy()
    return h


def check_values(name, got, ref, e32):
    """every (node, instance) of K, kff, Kp and every dV entry within 8 x e32; one parity_report line; figures printed first"""
    bar = rf.bar_of(e32, name)
    errs = {"K": rf.node_rel(got["K"], ref["K"]), "kff": rf.node_rel(got["kff"], ref["kff"]), "dV": rf.row_rel(got["dV"], ref["dV"])}
    if ref["Kp"] is not None:
        errs["Kp"] = rf.node_rel(got["Kp"], ref["Kp"])
    worst = {k: float(e.max()) for k, e in errs.items()}
    H, B = errs["K"].shape
    parity_report(f"box_ddp[{name}]", H=int(H), B=int(B), e32=e32, bar=bar, worst_over_e32=float(max(worst.values()) / max(e32, 1e-300)),
                  violations=int(sum((e > bar).sum() for e in errs.values())), **{"worst_" + k: v for k, v in worst.items()})
    print(f"box_ddp[{name}] " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  e32 {e32:.2e} bar {bar:.2e}")
    for what, e in errs.items():
        assert (e <= bar).all(), (name, what, "beyond", bar, "at", [tuple(int(i) for i in w) for w in np.argwhere(e > bar)[:8]], "worst", float(e.max()))


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


CASES = bx.matrix()


@pytest.mark.parametrize("variant,family,B,H", CASES, ids=[f"{v}-{f}-B{B}-H{H}" for v, f, B, H in CASES])
def test_box_backward_every_node_and_instance(gpu, ac, variant, family, B, H):
    c = bx.box_case(variant, family, B, H)   # the conditions on the inputs are asserted there, before any GPU result
    inp, ref = c["inp"], c["ref"]
    got = run_box(ac, gpu, inp, c["rate"])
    name = f"{variant}-{family}-B{B}-H{H}"
    print(f"box_ddp[{name}] stat: most iterations {int(got['stat'][0].max())} (reference {int(ref['stat'][0].max())}), capped {int(got['stat'][1].sum())}; "
          f"act mismatches {int((got['act'] != ref['act']).sum())}; clamped rows {int((ref['act'] != 0).sum())} of {ref['act'].size}")
    assert np.array_equal(got["act"], ref["act"]), ("active set differs at (node, row, instance)", np.argwhere(got["act"] != ref["act"])[:8].tolist())
    assert (got["stat"][1] == 0).all() and (got["stat"][0] >= 1).all() and (got["stat"][0] <= bx.MAX_ITERS).all()
    check_values(name, got, ref, c["e32"])
    cl = ref["act"] != 0                                            # (H, 7, B)
    assert (f32_bits(got["K"])[np.broadcast_to(cl[:, :, None, :], got["K"].shape)] == 0).all(), "a clamped row of K is not +0.0f"
    if got["Kp"] is not None:
        assert (f32_bits(got["Kp"])[np.broadcast_to(cl[:, :, None, :], got["Kp"].shape)] == 0).all(), "a clamped row of Kp is not +0.0f"
    U32 = inp["U"].astype(np.float32)
    lo = (np.asarray(inp["cost"].u_min, np.float32)[None, :, None] - U32).astype(np.float32)
    hi = (np.asarray(inp["cost"].u_max, np.float32)[None, :, None] - U32).astype(np.float32)
    bound = np.where(ref["act"] == 1, hi, lo)
    assert np.array_equal(f32_bits(got["kff"])[cl], f32_bits(bound)[cl]), "kff at a clamped row is not fl32(bound - U_k)"
    assert (got["kff"] >= lo).all() and (got["kff"] <= hi).all()
    assert (got["dV"][0] <= 0).all()


WIDE = [(v, bx.PARENT_B, 2 * rf.k_depth(bx.VARIANTS[v][1]) + 1) for v in bx.VARIANTS] + \
       [(v, bx.WIDE_B, rf.k_depth(bx.VARIANTS[v][1]) + 1) for v in ("goal", "rate_node_newton")]


@pytest.mark.parametrize("variant,B,H", WIDE, ids=[f"{v}-B{B}-H{H}" for v, B, H in WIDE])
def test_wide_box_reproduces_the_unboxed_reference(gpu, ac, variant, B, H):
    c = bx.wide_case(variant, B, H)
    assert c["e32"] <= rf.E32_MAX
    got = run_box(ac, gpu, c["inp"], c["rate"])
    assert not got["act"].any() and (got["stat"][1] == 0).all() and (got["stat"][0] == 1).all()
    check_values(f"wide-{variant}-B{B}-H{H}", got, c["ref"], c["e32"])


def test_box_argument_checks(gpu, ac):
    import copy
    import torch
    from aircraft_amd import _lib
    from aircraft_amd.control import ILQR

    c = bx.box_case("gn", "sym", bx.PARENT_B, 2)
    inp = c["inp"]
    t = {k: dev(inp[k], gpu) for k in ("X", "U", "A", "Bm")}
    for bad in ((0.5, -0.5), (float("nan"), 0.5), (-float("inf"), 0.5), (-0.5, float("inf"))):
        cost = copy.deepcopy(inp["cost"])
        cost.u_min, cost.u_max = list(cost.u_min), list(cost.u_max)
        cost.u_min[2], cost.u_max[2] = bad
        il = ILQR(system=ac, dt=0.01, num_nodes=2, cost=cost, box="qp")
        with pytest.raises(_lib.AircraftHipError, match="AC_ERR_BAD_ARG"):
            il.backward(t["X"], t["U"], t["A"], t["Bm"], box=True)
    il = ILQR(system=ac, dt=0.01, num_nodes=2, cost=inp["cost"], box="qp")
    lib, p = ac._sync(), lambda x: x.data_ptr()  # noqa: E731
    for node_q, Hz in ((None, p(t["A"])), (p(t["X"]), None)):   # uglin needs node arrays AND Hz
        rc = lib.ac_ilqr_backward_box_f32(ac._handle, il._cstruct(), node_q, node_q, node_q, p(t["U"]), Hz, p(t["X"]), p(t["U"]), p(t["A"]),
                                          p(t["Bm"]), bx.PARENT_B, 2, p(t["A"]), p(t["A"]), p(t["A"]), None, None, ac._stream())
        assert rc == -1
    K, kff, dV, act, stat = il.backward(t["X"], t["U"], t["A"], t["Bm"], box=True)   # buffers of its own; act / stat may also be NULL
    rc = lib.ac_ilqr_backward_box_f32(ac._handle, il._cstruct(), None, None, None, None, None, p(t["X"]), p(t["U"]), p(t["A"]), p(t["Bm"]),
                                      bx.PARENT_B, 2, p(K), p(kff), p(dV), None, None, ac._stream())
    assert rc == 0 and act.dtype == torch.int8 and stat.dtype == torch.int32
    torch.cuda.synchronize()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _assert_solve(name, prob, x0, U0, iters, lo, hi):
    import torch

    U = U0.clone()
    if prob.time_row > 0:
        U[:, prob.time_row, :] = prob.dt
    X = prob.rollout(x0, U)
    J = prob.trajectory_cost(X, U).clone()
    hist, active, capped, free_clamped = [J], 0, 0, 0
    for _ in range(iters):
        J, _ = prob.iterate(x0, X, U)
        hist.append(J.clone())
        assert bool(((U >= lo[None, :, None]) & (U <= hi[None, :, None])).all()), (name, "an accepted U left the box")
        active += int((prob.last_active != 0).sum())
        now = int(((prob.last_active == 1) | (prob.last_active == -1)).sum())
        free_clamped += now
        capped += int(prob.qp_stat[1].sum())
        print(f"{name}: sweep {len(hist) - 1} mean cost {float(J.mean()):.6g} clamped (not pinned) rows {now} most QP iterations {int(prob.qp_stat[0].max())}")
    hist = torch.stack(hist).cpu().numpy()
    assert np.isfinite(hist).all()
    assert (hist[1:] <= hist[:-1]).all(), (name, "the cost history increases somewhere")
    assert (hist[-1] < hist[0]).any()
    assert active > 0 and capped == 0
    return hist, free_clamped


def test_ilqr_box_qp_end_to_end(gpu):
    import torch
    from aircraft_amd.control import ILQR, QuadraticCost

    ac = make_aircraft("poly")
    B, H = 8, 20
    lim = 2.0
    results = {}
    for box in ("qp", "clip"):
        cost = QuadraticCost.goal((30.0, 2.0), reg=1.0)
        cost.u_min, cost.u_max = [-lim, -lim, -lim, 0, 0, 0, 0], [lim, lim, lim, 0, 0, 0, 1]
        prob = ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost, box=box)
        g = torch.Generator().manual_seed(5)
        x0 = torch.zeros(13, B)
        x0[2], x0[3], x0[9] = -100.0, 40.0, 1.0
        x0[3] += 2.0 * torch.randn(B, generator=g)
        x0[10:13] = 0.2 * torch.randn(3, B, generator=g)
        x0 = x0.to(gpu)
        U0 = torch.zeros(H, 7, B, device=gpu)
        lo, hi = torch.tensor(cost.u_min, device=gpu), torch.tensor(cost.u_max, device=gpu)
        if box == "qp":
            hist, clamped = _assert_solve("ilqr-box-qp", prob, x0, U0, 6, lo, hi)
            assert clamped > 0, "the surface limits never bound: the case does not test the box"
            results[box] = hist[-1]
        else:
            results[box] = prob.solve(x0, U0, iters=6)[2][-1].cpu().numpy()
    print("final cost per instance  box=qp:", np.array2string(results["qp"], precision=5), " box=clip:", np.array2string(results["clip"], precision=5))


def test_goal_acquisition_box_qp_end_to_end(gpu):
    import torch
    from aircraft_amd.control import GoalAcquisition

    ac = make_aircraft("poly")
    B, H = 8, 20
    results = {}
    for box in ("qp", "clip"):
        prob = GoalAcquisition(system=ac, goal=(30.0, 2.0), num_nodes=H, rate="exact", reg=1.0, box=box)
        g = torch.Generator().manual_seed(6)
        x0 = torch.zeros(13, B)
        x0[2], x0[3], x0[9] = -100.0, 40.0, 1.0
        x0[10:13] = 0.2 * torch.randn(3, B, generator=g)
        x0 = x0.to(gpu)
        U0 = torch.zeros(H, 7, B)
        U0[:, 0] = 1.0   # the reference's aileron guess
        U0 = U0.to(gpu)
        c = prob.cost
        lo, hi = torch.tensor(list(c.u_min), device=gpu), torch.tensor(list(c.u_max), device=gpu)
        prob._goal_ws(B, gpu)
        if box == "qp":
            hist, clamped = _assert_solve("goal-box-qp", prob, x0, U0, 6, lo, hi)
            assert clamped > 0, "the surface limits never bound: the case does not test the box"
            assert bool((prob.last_active[:, 3:6] == 2).all())      # the thrust rows are pinned
            results[box] = hist[-1]
        else:
            results[box] = prob.solve(x0, U0, iters=6)[2][-1].cpu().numpy()
    print("final loss per instance  box=qp:", np.array2string(results["qp"], precision=5), " box=clip:", np.array2string(results["clip"], precision=5))
