"""Issue placement of the bf16 hidden layers of the two headline units (MlpEngine::layer_bf), read off the emitted ISA with
tools/mfma_gaps.py: compiled here with the product flags, no GPU.

A bf16 16x16x32 MFMA holds the SIMD's vector issue for 8 of its 16 cycles, so the gap behind it hides 8 cycles of vector
issue and a gap runs max(16, 8 + filler).  The vector work of a layer call about equals that free capacity; it has to be
spread level to stay free.  Before the staged placement the model stood at 1.32 (k_nn_step_sens) and 1.24 (pair) of the
MFMA floor with 6.5 % / 3.6 % of the gaps above 32 cycles; a perfectly level placement of the same instructions is 1.05.
The bounds: modelled / floor <= 1.15 (room for the compiler, fails on any return of the clumps; ds_read_b128 priced at 4
although it is nearly free beside MFMAs — the stricter reading), at most 2 % of the gaps above 32 cycles (a third of the
better figure before: one clump of that size costs a whole block's free capacity), 1152 MFMAs per layer call."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mfma_gaps", os.path.join(ROOT, "tools", "mfma_gaps.py"))
mfma_gaps = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfma_gaps)

MAX_RATIO = 1.15
MAX_SHARE_ABOVE_32 = 0.02
MFMA_PER_LAYER_CALL = 1152


@pytest.mark.parametrize("unit", sorted(mfma_gaps.HEADLINE_UNITS))
def test_headline_issue_budget(unit, tmp_path):
    r = mfma_gaps.analyse(mfma_gaps.compile_unit(unit, str(tmp_path)))
    print(f"{unit}: modelled / floor {r['modelled']} / {r['floor']} = {r['ratio']:.3f}; gaps above 32 cycles {r['gt32']} of "
          f"{r['gaps'] - r['excluded']} ({100 * r['gt32_share']:.2f} %); gaps with a barrier or a branch left out: {r['excluded']}; "
          f"bf16 MFMAs {r['mfma']}")
    assert r["mfma"] == MFMA_PER_LAYER_CALL
    assert r["ratio"] <= MAX_RATIO, f"{unit}: modelled / floor {r['ratio']:.3f}"
    assert r["gt32_share"] <= MAX_SHARE_ABOVE_32, f"{unit}: {r['gt32']} gaps above 32 cycles of filler"
