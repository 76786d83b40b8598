"""The two units of the two-plane f16 hidden layers (nn_inst_wt8_f16_sens / _pair), compiled here with their product flags:
576 f16 MFMAs per layer call (three plane products where the bf16 form has six) and no bf16 MFMA; register-spill scratch and
AGPR<->VGPR moves in the MFMA blocks within the budgets of the bf16 units (tests/test_headline_resources.py: the f16 form has
fewer live registers and must not do worse); and the modelled issue ratio of tools/mfma_gaps.py no higher than the value
recorded in profiles/r09_f16_issue_model.json + 0.02 — a regression guard on the staged placement, not an acceptance figure
(a gap behind an f16 MFMA hides the same 8 cycles, but the form has half the gaps for well over half the vector work, so its
ratio to the MFMA floor is higher than the bf16 form's by construction).  Cross-compiles; no GPU."""
import importlib.util
import json
import os
import re

import pytest

from tests.test_headline_resources import compile_unit, scratch_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mfma_gaps", os.path.join(ROOT, "tools", "mfma_gaps.py"))
mfma_gaps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfma_gaps)

KERNEL = {"nn_inst_wt8_f16_sens": "k_nn_step_sens", "nn_inst_wt8_f16_pair": "k_nn_step_sens_pair"}
SCRATCH_BUDGET = {"nn_inst_wt8_f16_sens": 216, "nn_inst_wt8_f16_pair": 0}    # the bf16 units' budgets
ACC_MOVE_BUDGET = {"nn_inst_wt8_f16_sens": 200, "nn_inst_wt8_f16_pair": 50}
MFMA_PER_LAYER_CALL = 576
RATIO_SLACK = 0.02


def acc_moves_in_mfma_blocks(asm):
    moves = total = 0
    for blk in re.split(r"\n(?=\.LBB\d+_\d+:)", asm):
        ins = [l.strip() for l in blk.split("\n") if l.strip() and l.strip()[0] not in ";."]
        if any(i.startswith(mfma_gaps.MFMA_F16) for i in ins):
            moves += sum(i.startswith("v_accvgpr_") for i in ins)
            total += 1
    assert total > 0, "no f16 MFMA block found"
    return moves


@pytest.mark.parametrize("unit", sorted(KERNEL))
def test_f16_unit_static(unit, tmp_path):
    asm, remarks = compile_unit(unit, str(tmp_path))
    r = mfma_gaps.analyse(asm, mfma_gaps.MFMA_F16)
    scratch = scratch_bytes(remarks, KERNEL[unit])
    moves = acc_moves_in_mfma_blocks(asm)
    with open(os.path.join(ROOT, "profiles", "r09_f16_issue_model.json")) as fh:
        recorded = json.load(fh)[unit]["ratio"]
    print(f"{unit}: f16 MFMAs {r['mfma']}; scratch {scratch} B/lane; AGPR<->VGPR moves {moves}; modelled / floor "
          f"{r['modelled']} / {r['floor']} = {r['ratio']:.3f} (recorded {recorded:.3f})")
    assert r["mfma"] == MFMA_PER_LAYER_CALL
    assert not re.search(r"^\s*v_mfma_f32_16x16x32_bf16", asm, re.M), "a bf16 MFMA in an f16 unit"
    assert scratch <= SCRATCH_BUDGET[unit], f"{KERNEL[unit]}: scratch {scratch} B/lane"
    assert moves <= ACC_MOVE_BUDGET[unit], f"{KERNEL[unit]}: {moves} AGPR<->VGPR moves in the f16 MFMA blocks"
    assert r["ratio"] <= recorded + RATIO_SLACK, f"{unit}: modelled / floor {r['ratio']:.3f} against the recorded {recorded:.3f}"
