"""Host-side checks of the multiple-shooting mode (ILQR(shooting="multiple"), csrc/ac_shoot.hpp, csrc/ilqr_shoot_inst.hip,
csrc/ilqr_backward_inst.hip):
 1. the five ABI functions are declared in the header and the ctypes table, and the library exports them;
 2. the option, its refusals, and the call sequence of one iteration (the default mode's sequence is pinned by test_host_box.py);
 3. registers, scratch and LDS of the eight k_ilqr_backward_shoot kernels from the compiler's resource remarks."""
import ctypes as C
import os
import re
import subprocess

import pytest

from aircraft_amd import _lib
from tests import riccati_ref as rr
from tests.helpers import make_aircraft
from tests.test_host_box import _iterate

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ABI = {"ac_ilqr_backward_shoot_f32": 23, "ac_shoot_direction_f32": 17, "ac_shoot_merit_weight_f32": 7,
       "ac_shoot_candidates_f32": 13, "ac_shoot_merit_f32": 12}


def test_abi_prototypes():
    header = open(os.path.join(ROOT, "include", "aircraft_hip.h")).read()
    for name, n in ABI.items():
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == n, name
        decl = re.search(r"\nint " + name + r"\(([^;]*)\);", header).group(1)
        assert decl.count(",") + 1 == n, name
        assert decl.rstrip().endswith("void* stream")
    _, args = _lib.PROTOTYPES["ac_ilqr_backward_shoot_f32"]
    assert args[12] is C.c_long and args[13] is C.c_long and args[19] is C.c_int
    decl = re.search(r"\nint ac_ilqr_backward_shoot_f32\(([^;]*)\);", header).group(1)
    for piece in ("const float* F", "float* Vx", "float* Vxx", "int box", "signed char* act", "int* stat"):
        assert piece in decl, piece


def test_library_exports_the_shoot_functions():
    lib = _lib.load()
    for name in ABI:
        assert getattr(lib, name)


def _ilqr(**kw):
    from aircraft_amd.control import ILQR, QuadraticCost

    return ILQR(system=make_aircraft("poly"), dt=0.01, num_nodes=6, cost=QuadraticCost.goal((30.0, 2.0)), **kw)


def _goal(**kw):
    from aircraft_amd.control import GoalAcquisition

    return GoalAcquisition(system=make_aircraft("poly"), goal=(30.0, 2.0), num_nodes=6, **kw)


def test_option_and_refusals():
    p = _ilqr()
    assert p.shooting == "single" and p.last_multipliers is None and p.last_defect is None and p.merit_weight is None
    m = _ilqr(shooting="multiple", defect_weight=3.0, merit_factor=1.5)
    assert m.shooting == "multiple" and m.defect_weight == 3.0 and m.merit_factor == 1.5
    assert _goal(shooting="multiple").shooting == "multiple" and _goal(shooting="multiple", box="qp").box == "qp"
    with pytest.raises(AssertionError, match="shooting"):
        _ilqr(shooting="both")
    with pytest.raises(AssertionError, match="rate_weight"):
        _ilqr(shooting="multiple", rate_weight=2.0)
    with pytest.raises(AssertionError, match="time"):
        _ilqr(shooting="multiple", time="variable")
    with pytest.raises(AssertionError, match="hessian"):
        _ilqr(shooting="multiple", hessian="exact")
    with pytest.raises(AssertionError, match="rate='exact'"):
        _goal(shooting="multiple", rate="exact")
    with pytest.raises(AssertionError, match="defect_weight"):
        _ilqr(shooting="multiple", defect_weight=0.0)
    import torch

    with pytest.raises(AssertionError, match="X0"):
        _ilqr().solve(torch.zeros(13, 2), torch.zeros(6, 7, 2), X0=torch.zeros(7, 13, 2))


SEARCH = ["ac_shoot_direction_f32", "ac_shoot_merit_weight_f32", "ac_shoot_candidates_f32", "ac_shoot_defect_f32"]
TAIL = ["ac_shoot_merit_f32", "ac_shoot_merit_f32", "ac_ilqr_accept_f32"]


def test_call_sequence_of_one_iteration():
    """no rollout, ONE step launch for all candidates, the merit twice (candidates, iterate), the unchanged acceptance"""
    assert _iterate(_ilqr(shooting="multiple")) == ["linearise", "ac_ilqr_backward_shoot_f32"] + SEARCH + \
        ["ac_ilqr_cost_f32", "ac_ilqr_cost_f32"] + TAIL
    assert _iterate(_ilqr(shooting="multiple", box="qp")) == _iterate(_ilqr(shooting="multiple"))
    assert _iterate(_goal(shooting="multiple")) == ["linearise", "ac_goal_model_f32", "ac_ilqr_backward_shoot_f32"] + SEARCH + \
        ["ac_ilqr_cost_f32", "ac_goal_cost_f32", "ac_ilqr_cost_f32", "ac_goal_cost_f32"] + TAIL
    p = _ilqr(shooting="multiple", box="qp")
    assert p.last_multipliers is None and p.last_defect is None
    import torch

    p._workspace(3, torch.device("cpu"))      # the buffers exist, nothing has filled them yet
    assert p.last_multipliers is None and p.last_defect is None and tuple(p.merit_weight.shape) == (3,)
    _iterate(p)
    assert tuple(p.last_multipliers.shape) == (6, 13, 3) and tuple(p.last_defect.shape) == (3,) and tuple(p.merit_weight.shape) == (3,)
    assert tuple(p.last_active.shape) == (6, 7, 3)


def test_shoot_kernels_registers_scratch_and_lds(tmp_path):
    from aircraft_amd import build as B

    res = rr.backward_unit_resources()   # the eight kernels are in the unit of all backward kernels
    mine = {name: k for name, k in res.items() if k["family"] == "shoot"}
    assert len(mine) == 8
    names = set()
    for name, k in mine.items():
        sw = re.search(r"k_ilqr_backward_shootILb([01])ELb([01])ELb([01])EE", name).groups()   # NODE, NEWTON, BOX
        names.add(sw)
        newton = sw[1] == "1"
        vgpr, scratch, lds = k["vgpr"], k["scratch"], k["lds"]
        print(name[:48], "VGPRs", vgpr, "scratch", scratch, "LDS", lds)
        assert scratch == 0 and vgpr <= 256, (name, vgpr, scratch)   # two waves per SIMD, as the unswitched kernels
        # work area + ring: depth x (node image + 26 floats of F_k, x_{k+1})
        assert lds == 4 * (736 + (5 * (768 + 26) if newton else 8 * (320 + 26))), (name, lds)
    assert len(names) == 8   # every <NODE, NEWTON, BOX>
    # the four small kernels stay in ilqr_shoot_inst.hip
    src = os.path.join(B.CSRC, "ilqr_shoot_inst.hip")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("ilqr_shoot_inst", []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "shoot.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    small = [b for b in blocks if re.match(r"_ZN2ac\d+k_shoot_", b)]
    assert len(small) == 4
    for b in small:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b.split("\n")[0]
