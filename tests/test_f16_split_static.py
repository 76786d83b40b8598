"""The five-instruction activation split of the two f16 units (nn_inst_wt8_f16_sens / _pair; MlpEngine::split_pair and the f16
branch of bf_stage), compiled here with their product flags: one v_cvt_pk_f16_f32 for the hi plane, and the scaled residuals
written half a register each by v_fma_mixlo_f16 / v_fma_mixhi_f16 with S = 2^11 from an SGPR — no vector multiply by S is left.
The pins of tests/test_f16_headline_static.py hold beside it (576 f16 MFMAs per layer call, no bf16 MFMA, scratch and AGPR-move
budgets, modelled ratio <= the r09 record + 0.02), and two figures of the one-wave unit are below the parent's and no worse than
recorded in profiles/r10_f16_issue_model.json: the modelled cycles of tools/mfma_gaps.py for a layer call, and the v_readlane_b32
inside the RK4 stage loop (the parameters are read per stage with scalar loads instead of being parked in vector lanes).
Cross-compiles; no GPU."""
import json
import os
import re

import pytest

from tests.test_f16_headline_static import (ACC_MOVE_BUDGET, KERNEL, MFMA_PER_LAYER_CALL, RATIO_SLACK, SCRATCH_BUDGET,
                                            acc_moves_in_mfma_blocks, mfma_gaps)
from tests.test_headline_resources import compile_unit, scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_PAIRS = 96          # per unit: 16 pairs of slab 0 in front of the first MFMA + 16 for each of the five slabs after it
SCALE_BITS = "0x45000000"  # 2^11 as an fp32 literal
SENS = "nn_inst_wt8_f16_sens"


def recorded(name):
    with open(os.path.join(ROOT, "profiles", name)) as fh:
        return json.load(fh)


@pytest.fixture(scope="module", params=sorted(KERNEL))
def unit(request, tmp_path_factory):
    asm, remarks = compile_unit(request.param, str(tmp_path_factory.mktemp(request.param)))
    return request.param, asm, remarks


def count(asm, mnemonic):
    return len(re.findall(r"^\s*%s\s" % re.escape(mnemonic), asm, re.M))


def loop_blocks(asm):
    """[(instructions, loops)] per basic block of the text: `loops` = the headers of the loops the block lies in, outermost
    first, read off the loop comments the compiler prints behind the block labels."""
    parents, blocks, cur = {}, [], None
    head = None  # label whose comment lines are being read
    for line in asm.split("\n"):
        s = line.strip()
        m = re.match(r"\.L(BB\d+_\d+):(.*)", s)
        if m or re.match(r"; %bb\.\d+:", s):
            cur = {"label": m.group(1) if m else None, "ins": [], "inner": None, "chain": []}
            blocks.append(cur)
            head = cur
            s = ";" + (m.group(2) if m else s.split(":", 1)[1])
        if cur is None:
            continue
        if s.startswith(";"):
            if head is None:
                continue
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", s)
            if h:
                head["inner"] = h.group(1)
            p = re.search(r"Parent Loop (BB\d+_\d+)", s)
            if p:
                head["chain"].append(p.group(1))
            if "Loop Header" in s and head["label"]:
                head["inner"] = head["label"]
                parents[head["label"]] = list(head["chain"])
            continue
        if not s or s[0] == "." or s.endswith(":"):
            continue
        head = None
        cur["ins"].append(s.split(";")[0].strip())
    return [(b["ins"], (parents.get(b["inner"], []) + [b["inner"]]) if b["inner"] else []) for b in blocks]


def stage_loop_readlanes(asm):
    """v_readlane_b32 inside the RK4 stage loop.  Every f16 MFMA of the kernel sits in the loop over the hidden layers (the
    compiler keeps the three layer_bf calls of forward() rolled), and that loop lies directly inside the stage loop — beside
    the primal aero, the edge layers and the dual rigid body of the stage."""
    blocks = loop_blocks(asm)
    chains = [loops for ins, loops in blocks if any(i.startswith(mfma_gaps.MFMA_F16) for i in ins)]
    assert chains and all(chains), "an f16 MFMA outside every loop"
    common = chains[0]
    for c in chains[1:]:
        k = 0
        while k < min(len(common), len(c)) and common[k] == c[k]:
            k += 1
        common = common[:k]
    assert len(common) >= 2, f"no loop around the hidden-layer loop: {common}"
    stage = common[-2]
    body = [ins for ins, loops in blocks if stage in loops]
    # the stage loop holds the whole evaluation: the edge layers' and the rigid body's packed FMAs as well as the MFMAs
    assert sum(i.startswith("v_pk_fma_f32") for ins in body for i in ins) >= 576, "not the stage loop"
    return sum(i.startswith("v_readlane_b32") for ins in body for i in ins)


def test_split_instructions(unit):
    name, asm, _ = unit
    cvt, lo, hi = count(asm, "v_cvt_pk_f16_f32"), count(asm, "v_fma_mixlo_f16"), count(asm, "v_fma_mixhi_f16")
    muls = re.findall(r"^\s*v_(?:pk_)?mul\S*\s[^\n;]*%s" % SCALE_BITS, asm, re.M | re.I)
    print(f"{name}: v_cvt_pk_f16_f32 {cvt}, v_fma_mixlo_f16 {lo}, v_fma_mixhi_f16 {hi}, multiplies by {SCALE_BITS}: {len(muls)}")
    assert not muls, muls[:3]
    assert (cvt, lo, hi) == (SPLIT_PAIRS, SPLIT_PAIRS, SPLIT_PAIRS)


def test_existing_pins_hold(unit):
    name, asm, remarks = unit
    r = mfma_gaps.analyse(asm, mfma_gaps.MFMA_F16)
    scratch, moves = scratch_bytes(remarks, KERNEL[name]), acc_moves_in_mfma_blocks(asm)
    ratio9 = recorded("r09_f16_issue_model.json")[name]["ratio"]
    print(f"{name}: f16 MFMAs {r['mfma']}; scratch {scratch} B/lane; AGPR<->VGPR moves {moves}; ratio {r['ratio']:.3f} (r09 {ratio9:.3f})")
    assert r["mfma"] == MFMA_PER_LAYER_CALL
    assert not re.search(r"^\s*v_mfma_f32_16x16x32_bf16", asm, re.M), "a bf16 MFMA in an f16 unit"
    assert scratch <= SCRATCH_BUDGET[name] and moves <= ACC_MOVE_BUDGET[name]
    assert r["ratio"] <= ratio9 + RATIO_SLACK


def test_modelled_cycles_and_stage_loop_readlanes_below_the_parent(unit):
    name, asm, _ = unit
    rec = recorded("r10_f16_issue_model.json")[name]
    r = mfma_gaps.analyse(asm, mfma_gaps.MFMA_F16)
    lanes = stage_loop_readlanes(asm) if name == SENS else None
    print(f"{name}: modelled {r['modelled']} (parent {rec['parent']['modelled']}, recorded {rec['modelled']}); filler {r['filler']} "
          f"(parent {rec['parent']['filler']}); v_readlane_b32 in the stage loop {lanes}")
    assert rec["parent"]["modelled"] == recorded("r09_f16_issue_model.json")[name]["modelled"]
    assert r["modelled"] < rec["parent"]["modelled"]
    # regression guards on the recorded figures, as the r09 ratio: the model's slack of 0.02 of the floor / no more lane reads
    assert r["modelled"] <= rec["modelled"] + RATIO_SLACK * r["floor"]
    if name == SENS:
        assert lanes < rec["parent"]["stage_loop_readlane"], (lanes, rec["parent"]["stage_loop_readlane"])
        assert lanes <= rec["stage_loop_readlane"], (lanes, rec["stage_loop_readlane"])
