"""The width-128 plane routes (k_nn_step_sens<8, true, HID> and k_nn_step_sens_pair<8, HID>; three-plane bf16 and two-plane
f16 hidden layers, MlpEngine::layer_bf) block by block over depth and ring phase.

A net with n_hid hidden x hidden products moves the weight ring by 2 n_hid mod 3 regions per evaluation: 0 for the headline
net (n_hid = 3), 2, 1, 0, 2, 1, 0 for n_hid = 1 .. 6.  Every depth runs on both routes, through a persistent grid whose
workgroups take a second and a third task (so the ring enters them in every phase it can reach), through the pair kernel in
chunks that must reproduce the one-wave kernel bit for bit, and every block of every sampled unit is held to 8 x e_ref of the
case (tests/sens_blocks_ref.py: e_ref is the fp32 restatement's own error against the float64 oracle on the same units, capped
at 1.25e-5 before a GPU number is read).  Gate-edge nets and the argument forms (per-unit dt, the shooting layout,
normalise=False, sub-steps) run at 101 units through whichever kernel the dispatch picks.

Measured worst GPU error / e_ref per case: parity_report.jsonl, lines plane_blocks[...]; DESIGN.md section 5."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import sens_blocks_ref as R
from tests.helpers import block_rel_err, parity_report

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-5  # as tests/test_gpu_parity.py
PAD = 4096        # floats of NaN on either side of every output
_NAN_BITS = np.float32(np.nan).view(np.int32)


@pytest.fixture(scope="module")
def device_units(gpu):
    """the depth cases' units on the card, once per module (every depth x route case shares seed and size)"""
    import torch

    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    case = R.depth_cases()[0]
    X, U, dt, idx = R.case_units(case, cus)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(gpu)
    Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(gpu)
    return cus, Xd, Ud, dt, idx


def padded(shape, device):
    """(buffer, view): a NaN-filled flat buffer and the contiguous view of `shape` inside it, PAD floats from either end"""
    import torch

    size = int(np.prod(shape))
    buf = torch.full((size + 2 * PAD,), float("nan"), device=device, dtype=torch.float32)
    return buf, buf[PAD:PAD + size].view(*shape)


def bits(t):
    import torch

    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    import torch

    return torch.equal(bits(a), bits(b))


def call_into_padded(ac, Xd, Ud, dt):
    """step_sens into views of NaN-filled buffers: the padding stays bit-unchanged, the inside is finite"""
    import torch

    n = Xd.shape[1]
    bufs, outs = zip(*[padded(s, Xd.device) for s in ((13, n), (13, 13, n), (13, 7, n), (13, n))])
    ac.step_sens(Xd, Ud, dt, out=outs)
    torch.cuda.synchronize()
    for buf, out in zip(bufs, outs):
        edge = torch.cat([bits(buf[:PAD]), bits(buf[-PAD:])])
        assert bool((edge == int(_NAN_BITS)).all()), "an output's padding was written"
        assert bool(torch.isfinite(out).all()), "an output has unwritten or non-finite entries"
    return outs


def report_and_assert(case, got, cus, launch):
    ratio, bad, gF, eF = R.check_case_blocks(case, got, cus)
    worst = max(ratio, key=ratio.get)
    net, scale = R.case_net(case)
    print(f"{case.name} ({launch[0]}, grid {launch[1]}): units {got[0].shape[1]} worst GPU / e_ref {ratio[worst]:.2f} ({worst}); "
          f"x+ {gF:.2e} (host {eF:.2e})")
    parity_report(f"plane_blocks[{case.name}]", kernel=launch[0], grid=launch[1], units=int(got[0].shape[1]), hidden_scale=scale,
                  worst_block=worst, worst_over_e_ref=ratio[worst], over_e_ref=ratio, state=gF, state_host=eF,
                  violations=int(sum(v[0] for v in bad.values())))
    assert not bad, (case.name, "blocks beyond 8 x e_ref: {block: (units, worst, e_ref)}", bad)
    assert gF < STATE_TOL and gF <= R.BAR_FACTOR * eF, (case.name, gF, eF)


@pytest.mark.parametrize("name", [c.name for c in R.depth_cases()])
def test_depth_and_route_over_three_rounds(device_units, name):
    import torch

    case = {c.name: c for c in R.depth_cases()}[name]
    cus, Xd, Ud, dt, idx = device_units
    n, n3, chunk = R.depth_sizes(cus)
    assert n % (64 * cus) > 32 * cus and n3 % (64 * cus) > 32 * cus  # no remainder for the pair kernel
    X0, U0 = Xd.clone(), Ud.clone()
    ac = R.case_aircraft(case)
    pair_name = "k_nn_step_sens_pair" if case.use_mfma else "k_nn_step_sens"  # (the exact-fp32 form has no pair kernel at this width)
    try:
        # three rounds: half of the workgroups run a third task, the last one ragged
        big3 = call_into_padded(ac, Xd, Ud, dt)
        launch = ac.last_launch()
        assert launch[0] == "k_nn_step_sens" and launch[1] == cus, launch
        if case.route in ("bf16", "f16"):
            assert ac.hidden_route_in_use() == (case.route, 0)
        # the issue's size, one and a half rounds: the same units give the same bits whatever round and task they fall in
        Xn_, Un_ = Xd[:, :n].contiguous(), Ud[:, :n].contiguous()
        big = call_into_padded(ac, Xn_, Un_, dt)
        assert ac.last_launch()[0] == "k_nn_step_sens" and ac.last_launch()[1] == cus
        for a, b in zip(big, big3):
            assert same_bits(a, b[..., :n])
        # a repeat is bit-identical
        again = ac.step_sens(Xn_, Un_, dt)
        for a, b in zip(again, big):
            assert same_bits(a, b)
        # the pair kernel, in chunks of at most half a round: bit-identical to the one-wave kernel
        for s in range(0, n3, chunk):
            e = min(s + chunk, n3)
            part = ac.step_sens(Xd[:, s:e].contiguous(), Ud[:, s:e].contiguous(), dt)
            assert ac.last_launch()[0] == pair_name, (s, ac.last_launch())
            for a, b, what in zip(part, big3, "FABc"):
                assert same_bits(a, b[..., s:e]), (name, what, "chunk at", s)
        assert same_bits(Xd, X0) and same_bits(Ud, U0), "an input was written"
        ii = torch.from_numpy(idx).to(Xd.device)
        got = tuple(t.index_select(-1, ii).cpu().numpy() for t in big3)
    finally:
        ac.close()
    report_and_assert(case, got, cus, launch)


def run_small(case, ac, X, U, dt, gpu):
    """the case's call at 101 (111) units -> (F, A, B, c) as numpy, unit-last"""
    import torch

    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(gpu)
    Ud = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(gpu)
    if case.arg != "shoot":
        dtd = torch.from_numpy(np.ascontiguousarray(dt, dtype=np.float32)).to(gpu) if np.ndim(dt) > 0 else dt
        return tuple(t.cpu().numpy() for t in ac.step_sens(Xd, Ud, dtd))
    B, H = R.SHOOT_B, R.SHOOT_H
    # unit u = k B + b is node k of instance b: rollout-shaped buffers used in place, blk = B != n
    Xs = Xd.view(13, H, B).permute(1, 0, 2).contiguous()
    Us = Ud.view(7, H, B).permute(1, 0, 2).contiguous()
    F = torch.empty((H, 13, B), device=gpu); A = torch.empty((H, 13, 13, B), device=gpu)
    Bm = torch.empty((H, 13, 7, B), device=gpu); c = torch.empty((H, 13, B), device=gpu)
    lib = ac._sync()
    _lib.check(lib.ac_shoot_sens_f32(ac._handle, Xs.data_ptr(), Us.data_ptr(), C.c_float(float(dt)), None, B, H, F.data_ptr(),
                                     A.data_ptr(), Bm.data_ptr(), c.data_ptr(), ac._stream()), "ac_shoot_sens_f32")
    torch.cuda.synchronize()
    return (F.permute(1, 0, 2).reshape(13, H * B).cpu().numpy(), A.permute(1, 2, 0, 3).reshape(13, 13, H * B).cpu().numpy(),
            Bm.permute(1, 2, 0, 3).reshape(13, 7, H * B).cpu().numpy(), c.permute(1, 0, 2).reshape(13, H * B).cpu().numpy())


@pytest.mark.parametrize("name", [c.name for c in R.edge_cases() + R.arg_cases()])
def test_gate_edges_and_arguments(gpu, name):
    import torch

    case = {c.name: c for c in R.edge_cases() + R.arg_cases()}[name]
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    X, U, dt, idx = R.case_units(case, cus)
    ac = R.case_aircraft(case)
    try:
        got = run_small(case, ac, X, U, dt, gpu)
        launch = ac.last_launch()
        route = ac.hidden_route_in_use()
    finally:
        ac.close()
    # 101 units are a remainder under half a round: the pair kernel, except for sub-stepped updates (one-wave kernel only)
    assert launch[0] == ("k_nn_step_sens" if case.substeps > 1 else "k_nn_step_sens_pair"), launch
    assert route == {"edge-f16": ("f16", 0), "edge-bf16": ("bf16", 0), "rejected-auto": ("bf16", 3)}.get(name, (case.route, 0))
    if case.substeps > 1:
        # no host restatement of sub-steps: the suite's existing lines (tests/test_gpu_parity.py)
        from tests.test_gpu_parity import assert_sens

        ref = R.case_reference(case, cus)[0]
        eF = block_rel_err(got[0], ref[0])
        print(f"{name}: x+ {eF:.2e}")
        assert eF < STATE_TOL
        assert_sens(f"plane_blocks[{name}]", {"A": got[1], "B": got[2], "c": got[3]}, {"A": ref[1], "B": ref[2], "c": ref[3]})
        R.assert_exact_structure(got[1], got[2])
        return
    report_and_assert(case, got, cus, launch)
