"""Host-side checks of the box-constrained backward pass (ILQR(box="qp"), csrc/ac_boxqp.hpp, csrc/ilqr_backward_inst.hip):
 1. the two ABI functions are declared, the solvers take the option, and box="clip" calls exactly what it called before;
 2. the QP routine itself, compiled as plain C++ into a stand-alone program (tests/host_boxqp/boxqp_host.cpp) under
    -fsanitize=address,undefined, against tests/box_ddp_ref.py on the random problems of test_box_ddp_ref.py;
 3. registers, scratch and LDS of all 24 backward kernels, the eight box kernels among them, from the compiler's resource remarks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import box_ddp_ref as bx
from tests import riccati_ref as rr
from tests.helpers import make_aircraft

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_boxqp")


# ---- 1. ABI table, construction, call sequence -----------------------------------------------------------------------------------------
def test_abi_prototypes():
    res, args = _lib.PROTOTYPES["ac_ilqr_backward_box_f32"]
    assert res is C.c_int and len(args) == 19 and args[11] is C.c_long and args[12] is C.c_long
    res, args = _lib.PROTOTYPES["ac_ilqr_backward_rate_box_f32"]
    assert res is C.c_int and len(args) == 21 and args[12] is C.c_long and args[13] is C.c_long
    header = open(os.path.join(os.path.dirname(HERE), "..", "include", "aircraft_hip.h")).read()
    for name, n in (("ac_ilqr_backward_box_f32", 19), ("ac_ilqr_backward_rate_box_f32", 21)):
        decl = re.search(r"\nint " + name + r"\(([^;]*)\);", header).group(1)
        assert decl.count(",") + 1 == n, name
        assert "signed char* act" in decl and "int* stat" in decl


def test_library_exports_the_box_functions():
    lib = _lib.load()
    assert lib.ac_ilqr_backward_box_f32 and lib.ac_ilqr_backward_rate_box_f32


class Recorder:
    """stands in for the loaded library: every ac_* call is noted and succeeds"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ac_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            return 0

        return call


def _stubbed(problem):
    rec = Recorder()
    ac = problem.system
    ac._sync = lambda: rec
    ac._stream = lambda: C.c_void_p(0)
    problem.linearise = lambda *a, **k: rec.calls.append("linearise")
    return rec


def _iterate(problem, B=3):
    import torch

    rec = _stubbed(problem)
    H = problem.num_nodes
    x0, X, U = torch.zeros(13, B), torch.zeros(H + 1, 13, B), torch.zeros(H, 7, B)
    problem.iterate(x0, X, U)
    return rec.calls


PLAIN = ["linearise", "ac_ilqr_backward_newton_f32", "ac_rollout_policy_f32", "ac_ilqr_cost_f32", "ac_ilqr_cost_f32", "ac_ilqr_accept_f32"]
RATE = ["linearise", "ac_ilqr_rate_model_f32", "ac_ilqr_backward_rate_f32", "ac_rollout_policy_rate_f32", "ac_ilqr_cost_f32",
        "ac_ilqr_rate_cost_f32", "ac_ilqr_cost_f32", "ac_ilqr_rate_cost_f32", "ac_ilqr_accept_f32"]
GOAL_FROZEN = ["linearise", "ac_goal_model_f32", "ac_ilqr_backward_goal_f32", "ac_rollout_policy_f32", "ac_ilqr_cost_f32", "ac_goal_cost_f32",
               "ac_ilqr_cost_f32", "ac_goal_cost_f32", "ac_ilqr_accept_f32"]
GOAL_EXACT = ["linearise", "ac_goal_model_rate_f32", "ac_ilqr_backward_rate_f32", "ac_rollout_policy_rate_f32", "ac_ilqr_cost_f32",
              "ac_goal_cost_f32", "ac_ilqr_cost_f32", "ac_goal_cost_f32", "ac_ilqr_accept_f32"]


def _swap(seq, old, new):
    assert old in seq
    return [new if s == old else s for s in seq]


def test_box_option_and_call_sequence():
    from aircraft_amd.control import ILQR, GoalAcquisition, QuadraticCost

    def ilqr(**kw):
        return ILQR(system=make_aircraft("poly"), dt=0.01, num_nodes=6, cost=QuadraticCost.goal((30.0, 2.0)), **kw)

    def goal(**kw):
        return GoalAcquisition(system=make_aircraft("poly"), goal=(30.0, 2.0), num_nodes=6, **kw)

    assert ilqr().box == "clip" and ilqr(box="qp").box == "qp" and goal(box="qp").box == "qp" and goal().box == "clip"
    assert goal(box="qp", time="variable").time_row > 0
    with pytest.raises(AssertionError):
        ilqr(box="project")
    # the default: the calls of the parent, in their order, and nothing of the box
    assert _iterate(ilqr()) == PLAIN == _iterate(ilqr(box="clip"))
    assert _iterate(ilqr(rate_weight=2.0)) == RATE
    assert _iterate(goal()) == GOAL_FROZEN and _iterate(goal(rate="exact")) == GOAL_EXACT
    # box="qp": the backward call alone is replaced
    assert _iterate(ilqr(box="qp")) == _swap(PLAIN, "ac_ilqr_backward_newton_f32", "ac_ilqr_backward_box_f32")
    assert _iterate(ilqr(box="qp", rate_weight=2.0)) == _swap(RATE, "ac_ilqr_backward_rate_f32", "ac_ilqr_backward_rate_box_f32")
    assert _iterate(goal(box="qp")) == _swap(GOAL_FROZEN, "ac_ilqr_backward_goal_f32", "ac_ilqr_backward_box_f32")
    assert _iterate(goal(box="qp", rate="exact")) == _swap(GOAL_EXACT, "ac_ilqr_backward_rate_f32", "ac_ilqr_backward_rate_box_f32")
    p = ilqr(box="qp")
    assert p.last_active is None and p.qp_stat is None
    _iterate(p)
    assert tuple(p.last_active.shape) == (6, 7, 3) and tuple(p.qp_stat.shape) == (2, 3)
    q = ilqr()
    _iterate(q)
    assert q.last_active is None and q.qp_stat is None


# ---- 2. the routine as a host program under the sanitizers ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("boxqp")
    exe = str(tmp / "boxqp_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-DAC_HOST_CHECK", "-ffp-contract=off", "-Wno-unknown-pragmas",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "boxqp_host.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    P = bx.qp_problems()
    path = str(tmp / "problems.txt")
    with open(path, "w") as f:
        f.write(f"{bx.N_QPS}\n")
        for p in range(bx.N_QPS):
            row = np.concatenate([P["Q"][p].ravel(), P["g"][p], P["lo"][p], P["hi"][p]]).astype(np.float32)
            f.write(" ".join(f"{v:.9g}" for v in row) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-3000:])
    rows = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().split("\n")])
    assert rows.shape == (bx.N_QPS, 16)
    return dict(x=rows[:, :7], act=rows[:, 7:14].astype(np.int8), iters=rows[:, 14].astype(int), capped=rows[:, 15].astype(int))


def test_host_program_active_sets(host_results):
    P = bx.qp_problems()
    cond = np.flatnonzero(P["conditioned"])
    assert cond.size >= 150
    for p in cond:
        assert np.array_equal(host_results["act"][p], P["enum"][p][1]), (p, host_results["act"][p], P["enum"][p][1])
    assert not host_results["capped"].any()
    assert host_results["iters"].max() <= 8 and host_results["iters"].min() >= 1
    # whatever the margins: feasible, and clamped rows exactly on their bound
    lo, hi = P["lo"].astype(np.float32), P["hi"].astype(np.float32)
    x, act = host_results["x"].astype(np.float32), host_results["act"]
    assert (x >= lo).all() and (x <= hi).all()
    assert np.array_equal(x[act == -1], lo[act == -1]) and np.array_equal(x[act == 1], hi[act == 1]) and np.array_equal(x[act == 2], lo[act == 2])


def test_host_program_solution_within_the_fp32_bar(host_results):
    """per problem max|x - x*| / max(|x*|, widest box row) against the enumerated float64 solution; the bar is 8 x the worst such
    error of the fp32 NumPy restatement over the conditioned problems"""
    P = bx.qp_problems()
    cond = np.flatnonzero(P["conditioned"])

    def rel(x, p):
        xe = P["enum"][p][0]
        return np.abs(np.asarray(x, np.float64) - xe).max() / max(np.abs(xe).max(), (P["hi"][p] - P["lo"][p]).max())

    e32 = max(rel(P["f32"][p][0], p) for p in cond)
    got = np.array([rel(host_results["x"][p], p) for p in cond])
    print(f"host box-QP: worst {got.max():.2e}, fp32 restatement {e32:.2e}, bar {8 * e32:.2e}")
    assert 0 < e32 <= 1e-5
    assert (got <= 8 * e32).all(), (cond[got > 8 * e32], got.max())


# ---- 3. resources of the kernels ---------------------------------------------------------------------------------------------------
def test_box_kernels_registers_and_scratch():
    res = rr.backward_unit_resources()
    assert len(res) == 24   # every <NODE, NEWTON, BOX> of k_ilqr_backward, _shoot and _rate, from the one unit
    for name, k in res.items():
        print(name[:60], "VGPRs", k["vgpr"], "scratch", k["scratch"], "LDS", k["lds"])
        assert k["scratch"] == 0 and k["vgpr"] <= 256, (name, k)
        assert k["lds"] == rr.ring_lds_bytes(k["newton"], shoot=k["family"] == "shoot", rate=k["family"] == "rate"), (name, k)
    mine = [name for name, k in res.items() if k["box"] and k["family"] != "shoot"]
    assert len(mine) == 8
    assert sum("k_ilqr_backward_rate" in name for name in mine) == 4
    for name in mine:
        assert "Lb1EEEv" in name, name   # BOX = true instantiations only
