"""The Riccati backward kernel k_ilqr_backward<NODE, NEWTON> and the costate kernel k_ilqr_costate<NODE>
(aircraft_amd/csrc/ac_ilqr.hpp) against oracle/ilqr_oracle.py node by node, at every edge of the LDS-DMA ring.

Inputs are synthetic (tests/riccati_ref.py: every node of every instance differs by O(1) from its neighbours) and go
straight into ILQR.backward / ILQR.costate: no dynamics kernel runs.  Every (node, instance) of K and kff and every entry of
dV is held to 8 x the error of an fp32 NumPy restatement of the same recursion on the same inputs (about 5e-6).  Horizons:
a ring that is never full (1, 2, kDepth-1), exactly full (kDepth), the first refill (kDepth+1), a slot reused twice
(2 kDepth-1 .. 2 kDepth+1), and 23.  At H = kDepth+1 a batch of 65 is also re-run in pieces: one wave per instance, so a piece
must reproduce its columns bit for bit."""
import numpy as np
import pytest

from tests import riccati_ref as rr
from tests.helpers import make_aircraft

pytestmark = pytest.mark.gpu

PAD = 96                   # guard floats on both sides of every output
NAN_BITS = 0x7FC0BEEF      # a quiet NaN with a recognisable payload


@pytest.fixture(scope="module")
def ac(gpu):
    return make_aircraft("poly")


def dev(a, gpu):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(gpu)


def guarded(shape, gpu):
    """(buffer, view): a view of `shape` into a larger buffer, everything pre-filled with the NaN bit pattern"""
    import torch

    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), NAN_BITS, dtype=torch.int32, device=gpu).view(torch.float32)
    return buf, buf[PAD:PAD + n].view(*shape)


def assert_guards(bufs, what):
    import torch

    for name, (buf, view) in bufs.items():
        bits = buf.view(torch.int32)
        assert bool((bits[:PAD] == NAN_BITS).all()) and bool((bits[-PAD:] == NAN_BITS).all()), (what, name, "padding overwritten")
        assert bool(torch.isfinite(view).all()), (what, name, "an element was not written, or is not finite")


def bits_equal(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_backward(ac, gpu, inp, newton_zero=False, uglin_zero=False):
    """One launch through ILQR.backward on float32 copies of `inp`; outputs are guarded views; the inputs are checked to be
    bit-unchanged.  newton_zero / uglin_zero: pass all-zero Hz / uglin arrays where `inp` has none.  -> K, kff, dV (device)."""
    import torch
    from aircraft_amd.control import ILQR

    H, _, B = inp["U"].shape
    il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=inp["cost"])
    t = {k: dev(inp[k], gpu) for k in ("X", "U", "A", "Bm")}
    t["Hz"] = dev(inp["Hz"], gpu) if inp["Hz"] is not None else (torch.zeros((H, 21, 21, B), device=gpu) if newton_zero else None)
    t["uglin"] = dev(inp["uglin"], gpu) if inp["uglin"] is not None else (torch.zeros((H, 7, B), device=gpu) if uglin_zero else None)
    node = None if inp["node"] is None else tuple(dev(a, gpu) for a in inp["node"])
    before = {k: v.clone() for k, v in t.items() if v is not None}
    node_before = None if node is None else [a.clone() for a in node]
    bufs = {"K": guarded((H, 7, 13, B), gpu), "kff": guarded((H, 7, B), gpu), "dV": guarded((2, B), gpu)}
    out = tuple(bufs[k][1] for k in ("K", "kff", "dV"))
    il.backward(t["X"], t["U"], t["A"], t["Bm"], out=out, Hz=t["Hz"], node=node, uglin=t["uglin"])
    torch.cuda.synchronize()
    name, grid, block, _ = ac.last_launch()
    assert (name, grid, block) == ("k_ilqr_backward", B, 64)
    assert_guards(bufs, "backward")
    for k, v in before.items():
        assert bits_equal(t[k], v), (k, "input modified")
    if node is not None:
        assert all(bits_equal(a, b) for a, b in zip(node, node_before)), "node arrays modified"
    return out


CASES = rr.matrix()


@pytest.mark.parametrize("variant,B,H", CASES, ids=[f"{v}-B{B}-H{H}" for v, B, H in CASES])
def test_backward_every_node_and_instance_matches_oracle(gpu, ac, variant, B, H):
    c = rr.riccati_case(variant, B, H)
    # conditions on the inputs, before the GPU result is looked at
    assert c["e32"] <= rr.E32_MAX and c["quu_min"] >= rr.QUU_MIN
    K, kff, dV = run_backward(ac, gpu, c["inp"])
    again = run_backward(ac, gpu, c["inp"])
    assert all(bits_equal(a, b) for a, b in zip((K, kff, dV), again)), "a repeat of the call differs"
    Kh, kh, dVh = (a.cpu().numpy() for a in (K, kff, dV))
    worst = rr.check_riccati(f"{variant}-B{B}-H{H}", Kh, kh, dVh, c["ref"], c["f32"], quu_min=c["quu_min"])
    print(f"riccati[{variant}-B{B}-H{H}] K {worst[0]:.2e} kff {worst[1]:.2e} dV {worst[2]:.2e}  e32 {c['e32']:.2e} bar {worst[3]:.2e}")
    assert (dVh[0] <= 0).all()   # descent direction on every instance
    if B == rr.WIDE_B:
        # one wave per instance, the only cross-instance quantity is the stride: a piece of the batch reproduces its columns
        for sl in (slice(0, 1), slice(31, 32), slice(64, 65), slice(16, 65)):
            sub = run_backward(ac, gpu, rr.columns(c["inp"], sl))
            for name, a, b in zip(("K", "kff", "dV"), sub, (K, kff, dV)):
                assert bits_equal(a, b[..., sl]), (name, "columns", sl, "differ from the parent batch")


@pytest.mark.parametrize("H", [9, 23])
def test_zero_second_order_blocks_reproduce_the_gauss_newton_pass(gpu, ac, H):
    """<true, true> fed Hz == 0 (and uglin == 0, or none: the dummy gather of u_k) is the <true, false> pass: both within
    the bar of the SAME float64 reference, and of each other."""
    c = rr.riccati_case("node", rr.PARENT_B, H)
    bar = rr.bar_of(c["e32"])
    base = [a.cpu().numpy() for a in run_backward(ac, gpu, c["inp"])]
    for uglin_zero in (False, True):
        got = [a.cpu().numpy() for a in run_backward(ac, gpu, c["inp"], newton_zero=True, uglin_zero=uglin_zero)]
        rr.check_riccati(f"node-as-newton-uglin{int(uglin_zero)}-H{H}", *got, c["ref"], c["f32"], quu_min=c["quu_min"])
        assert rr.node_rel(got[0], base[0]).max() <= bar and rr.node_rel(got[1], base[1]).max() <= bar
        assert rr.row_rel(got[2], base[2]).max() <= bar


@pytest.mark.parametrize("nodef,B,H", rr.COSTATE_CASES, ids=[f"{'node' if n else 'const'}-B{B}-H{H}" for n, B, H in rr.COSTATE_CASES])
def test_costate_every_node_and_instance_matches_oracle(gpu, ac, nodef, B, H):
    import torch
    from aircraft_amd.control import ILQR

    p = rr.costate_parent(nodef, H)
    assert p["e32"] <= rr.E32_MAX
    inp = rr.columns(p["inp"], slice(0, B))     # the leading columns of the parent batch
    il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=inp["cost"])
    X, A = dev(inp["X"], gpu), dev(inp["A"], gpu)
    node = None if inp["node"] is None else tuple(dev(a, gpu) for a in inp["node"])
    keep = [t.clone() for t in (X, A) + (node or ())]
    outs = []
    for _ in range(2):
        bufs = {"Lam": guarded((H, 13, B), gpu)}
        il.costate(X, A, node=node, out=bufs["Lam"][1])
        torch.cuda.synchronize()
        name, grid, block, _ = ac.last_launch()
        assert (name, grid, block) == ("k_ilqr_costate", (B + rr.COSTATE_BLOCK - 1) // rr.COSTATE_BLOCK, rr.COSTATE_BLOCK)
        assert_guards(bufs, "costate")
        outs.append(bufs["Lam"][1])
    assert bits_equal(outs[0], outs[1]), "a repeat of the call differs"
    assert all(bits_equal(a, b) for a, b in zip((X, A) + (node or ()), keep)), "input modified"
    worst, bar = rr.check_costate(f"{'node' if nodef else 'const'}-B{B}-H{H}", outs[0].cpu().numpy(), p["ref"][..., :B], p["e32"])
    print(f"costate[node={nodef}, B={B}, H={H}] worst {worst:.2e} e32 {p['e32']:.2e} bar {bar:.2e}")
