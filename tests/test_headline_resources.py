"""Register budget of the two headline units, compiled here with their product flags (aircraft_amd/build.py): the bf16
hidden layers keep the weight fragments in AGPRs and the accumulators in VGPRs, so the AGPR<->VGPR copies inside them
stay under budget, and the register-spill scratch does not grow back.  Cross-compiles; no GPU."""
import os
import re
import subprocess

import pytest

from aircraft_amd import build as B

# v_accvgpr_read/write/mov in the basic blocks that issue bf16 MFMAs (the hidden-layer body); before the AGPR fragments and
# the VGPR-form accumulators: 604 (k_nn_step_sens) and 384 (pair); after: 167 and 0 (profiles/r06_resources.txt).
ACC_MOVE_BUDGET = {"nn_inst_wt8_mfma_sens": 200, "nn_inst_wt8_mfma_pair": 50}
# bytes per lane; 256 before this budget was set (the spills sit in the dual RK4 code around forward())
SCRATCH_BUDGET = {"nn_inst_wt8_mfma_sens": 216, "nn_inst_wt8_mfma_pair": 0}
KERNEL = {"nn_inst_wt8_mfma_sens": "k_nn_step_sens", "nn_inst_wt8_mfma_pair": "k_nn_step_sens_pair"}


def compile_unit(unit, out_dir):
    src = os.path.join(B.CSRC, unit + ".hip")
    asm = os.path.join(out_dir, unit + ".s")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get(unit, []), "-S", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(asm).read(), r.stderr


def scratch_bytes(remarks, kernel):
    for block in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]:
        name = block.split("\n")[0].split(" ")[0]
        if re.match(r"_ZN2ac%d%s[IE]" % (len(kernel), kernel), name):
            return int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1))
    raise AssertionError(f"no resource remark for {kernel}")


def hidden_layer_acc_moves(asm):
    """accvgpr moves in the basic blocks that hold bf16 MFMAs (the unit instantiates one kernel)."""
    moves = total = 0
    for blk in re.split(r"\n(?=\.LBB\d+_\d+:)", asm):
        ins = [l.strip() for l in blk.split("\n") if l.strip() and l.strip()[0] not in ";."]
        if any(i.startswith("v_mfma_f32_16x16x32_bf16") for i in ins):
            moves += sum(i.startswith("v_accvgpr_") for i in ins)
            total += 1
    assert total > 0, "no bf16 MFMA block found"
    return moves


@pytest.mark.parametrize("unit", sorted(KERNEL))
def test_headline_unit_budget(unit, tmp_path):
    asm, remarks = compile_unit(unit, str(tmp_path))
    scratch = scratch_bytes(remarks, KERNEL[unit])
    moves = hidden_layer_acc_moves(asm)
    assert scratch <= SCRATCH_BUDGET[unit], f"{KERNEL[unit]}: scratch {scratch} B/lane"
    assert moves <= ACC_MOVE_BUDGET[unit], f"{KERNEL[unit]}: {moves} AGPR<->VGPR moves in the bf16 MFMA blocks"
