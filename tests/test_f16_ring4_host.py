"""The four-region weight ring of the one-wave f16 sensitivity kernel, on the host (aircraft_amd/csrc/ac_mlp_plan.hpp compiled
with g++; no GPU): where the fourth region lies, and the order in which slots are read and overwritten.

The kernel's protocol (MlpEngine::acquire, four-region form): the prologue loads the first streamed layer into slot 0.  At the
head of every hidden layer a wave waits for its own pieces of that layer and passes ONE workgroup barrier, which proves every
wave done with the layer before; the layer is then read from slot ring_pos & 1 and, during it, the next layer of the cyclic
sequence is requested into the other slot.  The walk below replays f16_ring4_step over 2 tasks x 4 RK4 stages and checks,
for nets with 1 to 4 streamed layers (odd counts flip the slot parity between forward() calls):
  * the layer acquired is the one that was requested into the slot it is read from;
  * a request never targets the slot being read, never overwrites a layer that was requested and not yet read, and the last
    reader of the target slot is a layer instance that the barrier in front of the request has retired."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_mlp_model_host import PLAN, Model, random_net

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "host_mlp", "mlp_model_host.cpp"), os.path.join(HERE, "host_mlp", "ring4_host.cpp")]
LDS, KIB = 160 * 1024, 1024
STREAMED = [1, 2, 3, 4]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ring4") / "libring4_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, *SRCS], check=True)
    L = C.CDLL(so)
    L.host_mlp_build.restype = C.c_void_p
    L.host_mlp_build.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.host_mlp_free.argtypes = [C.c_void_p]
    L.host_mlp_rc.argtypes = [C.c_void_p]
    L.host_mlp_err.argtypes = [C.c_void_p]
    L.host_mlp_err.restype = C.c_char_p
    L.host_mlp_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.host_mlp_vplan.argtypes = [C.c_void_p, C.c_void_p]
    L.host_mlp_scalars.argtypes = [C.c_void_p, C.c_void_p]
    for f in (L.host_mlp_blob, L.host_mlp_vimage):
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_void_p]
    L.host_mlp_folded_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in (L.host_mlp_folded_W, L.host_mlp_folded_b):
        f.restype = C.POINTER(C.c_float)
        f.argtypes = [C.c_void_p, C.c_int]
    L.host_ring4_lds.argtypes = [C.c_void_p, C.c_int]
    L.host_ring4_slot.argtypes = [C.c_void_p, C.c_int]
    L.host_ring4_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.host_ring4_of_net.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.host_mlp_plan_ints() * 4 == PLAN.itemsize
    return L


def net_of(streamed):
    """5-128-...-128-6 with `streamed` hidden products (width x width layers: the ones the ring streams)"""
    return random_net((128,) * (streamed + 1), 20 + streamed)


def plan_ptr(p):
    a = np.array([p], PLAN)
    return a, a.ctypes.data


def ring4_of_net(lib, Ws, bs, act):
    Ws = [np.ascontiguousarray(W, np.float32) for W in Ws]
    bs = [np.ascontiguousarray(b, np.float32) for b in bs]
    n = len(Ws)
    widths = (C.c_int * (n + 1))(Ws[0].shape[1], *[W.shape[0] for W in Ws])
    pw = (C.c_void_p * n)(*[W.ctypes.data for W in Ws])
    pb = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
    return lib.host_ring4_of_net(n, widths, (C.c_int * n)(*act), pw, pb)


@pytest.mark.parametrize("streamed", STREAMED)
def test_four_regions_and_resident_blocks(lib, streamed):
    Ws, bs, act = net_of(streamed)
    m = Model(lib, Ws, bs, act, 1)
    assert m.rc == 0 and m.wt == 8 and m.has_bf
    p = m.plan_f16
    keep, ptr = plan_ptr(p)
    front, layer = lib.host_ring4_front_bytes(8), lib.host_ring4_layer_bytes(8)
    assert front == 33 * KIB and layer == 65 * KIB
    total = lib.host_ring4_lds(ptr, front)
    assert total == ring4_of_net(lib, Ws, bs, act)  # what the dispatcher launches with
    assert total == p["lds_total"] + front == 140 * KIB and total <= LDS and total % KIB == 0
    assert p["n_streamed"] == streamed
    regions = [int(r) for r in p["bf_region"]] + [int(p["lds_total"])]  # the fourth region follows the third
    last = int(p["n_layers"]) - 1
    spans = [(int(p["lds_off"][l]), int(p["bytes"][l])) for l in (0, last)] + [(r, front) for r in regions]
    for off, size in spans:
        assert off >= 0 and off % KIB == 0 and size % KIB == 0 and off + size <= total
    order = sorted(spans)
    for (a, na), (b, _) in zip(order, order[1:]):
        assert a + na <= b, "overlap"
    # a slot is (front, back): a whole layer image from its first byte stays inside its two regions
    for k in (0, 1):
        s = lib.host_ring4_slot(ptr, k)
        assert s == regions[2 * k] and regions[2 * k + 1] == s + front and s + layer <= regions[2 * k + 1] + front
    # the plan itself is what it was: three regions, the pair plan derived from it
    assert p["lds_total"] == 8 * KIB + 3 * front and m.plan_f16_pair["lds_total"] == p["bf_region"][2]


def test_a_ring_that_does_not_fit_keeps_three_regions(lib):
    Ws, bs, act = net_of(3)
    p = Model(lib, Ws, bs, act, 1).plan_f16.copy()
    front = lib.host_ring4_front_bytes(8)
    keep, ptr = plan_ptr(p)
    assert lib.host_ring4_lds(ptr, front) == 140 * KIB
    for grow in (20 * KIB, 21 * KIB):  # 160 KiB fits exactly, one piece more does not
        q = p.copy()
        q["bf_region"] += grow
        q["lds_total"] += grow
        keep, ptr = plan_ptr(q)
        assert lib.host_ring4_lds(ptr, front) == (160 * KIB if grow == 20 * KIB else 0)
    q = p.copy()
    q["bf_region"][2] += KIB  # regions not adjacent: a layer is no longer one run of pieces
    q["lds_total"] += KIB
    keep, ptr = plan_ptr(q)
    assert lib.host_ring4_lds(ptr, front) == 0
    keep, ptr = plan_ptr(p)
    assert lib.host_ring4_lds(ptr, front + KIB) == 0  # region size is not the front half's
    # a net without width-128 hidden products has no ring at all
    Ws, bs, act = random_net((64, 64, 64), 2)
    assert ring4_of_net(lib, Ws, bs, act) == 0
    Ws, bs, act = random_net((128,), 3)
    assert ring4_of_net(lib, Ws, bs, act) == 0


@pytest.mark.parametrize("streamed", STREAMED)
def test_slot_walk_over_two_tasks(lib, streamed):
    Ws, bs, act = net_of(streamed)
    p = Model(lib, Ws, bs, act, 1).plan_f16
    keep, ptr = plan_ptr(p)
    seq = [int(l) for l in p["streamed"][:streamed]]
    assert seq == list(range(1, streamed + 1))
    content = {0: seq[0], 1: None}    # the prologue: first streamed layer into slot 0
    unread = {0: True, 1: False}      # requested and not yet read
    last_reader = {0: None, 1: None}  # layer instance (running count) that read the slot last
    ring_pos, snext = 0, (1 if streamed > 1 else 0)
    inst = 0
    out = np.zeros(4, np.int32)
    parities = set()
    for task in range(2):
        for stage in range(4):
            for i, l in enumerate(seq):
                # head of layer instance `inst`: own pieces waited for, then the barrier: instances < inst are retired
                retired_below = inst
                lib.host_ring4_step(ptr, ring_pos, snext, out.ctypes.data)
                rd, nl, ns, snext = (int(v) for v in out)
                ring_pos += 1
                assert rd in (0, 1) and ns == 1 - rd, "a request never targets the slot being read"
                assert content[rd] == l and unread[rd], (task, stage, l, content)
                assert nl == seq[(i + 1) % streamed], "the next layer of the cyclic sequence (wraps into the next forward())"
                assert not unread[ns], "would overwrite a layer nobody has read"
                assert last_reader[ns] is None or last_reader[ns] < retired_below, "previous reader not retired by a barrier"
                unread[rd], last_reader[rd] = False, inst
                content[ns], unread[ns] = nl, True  # requested during the layer, behind the barrier
                if i == 0:
                    parities.add(rd)
                inst += 1
    # odd counts: the first layer of a forward() alternates between the slots; even counts: always slot 0
    assert parities == ({0, 1} if streamed % 2 else {0})
