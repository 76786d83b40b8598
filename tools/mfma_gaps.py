#!/usr/bin/env python3
"""Static issue model of the bf16 hidden layers (MlpEngine::layer_bf) from the emitted ISA.  No GPU.

Compiles a unit with its product flags (aircraft_amd/build.py) to assembly, cuts the instruction stream between the first and
the last v_mfma_f32_16x16x32_bf16 at every MFMA and prices what sits in each gap with the measured issue costs of gfx950
(one wave per SIMD): a bf16 16x16x32 MFMA holds the SIMD's vector issue for 8 of its 16 cycles, so a gap runs about
max(16, 8 + filler); plain v_* 4, v_exp/log/rcp/rsq/sqrt/sin/cos and v_pk_* 8, ds_* and memory ops 4, s_nop n 4 (n + 1),
scalar ops 0.  Gaps that hold a barrier or a branch (the mid-layer barrier, the wave-pair exchange, the seam between the two
role bodies of the pair kernel) are left out of the sums and counted.

    python tools/mfma_gaps.py                    # both headline units
    python tools/mfma_gaps.py UNIT [UNIT ...]    # named units
    python tools/mfma_gaps.py --asm FILE.s       # an assembly file made elsewhere
    python tools/mfma_gaps.py --f16              # the two units of the two-plane f16 form (v_mfma_f32_16x16x32_f16)
    python tools/mfma_gaps.py --mfma MNEMONIC UNIT [UNIT ...]

analyse() is what tests/test_headline_issue_budget.py asserts on."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA = "v_mfma_f32_16x16x32_bf16"
MFMA_F16 = "v_mfma_f32_16x16x32_f16"
HEADLINE_UNITS = ("nn_inst_wt8_mfma_sens", "nn_inst_wt8_mfma_pair")
F16_UNITS = ("nn_inst_wt8_f16_sens", "nn_inst_wt8_f16_pair")
TRANS = ("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")
MFMA_CYCLES = 16   # one v_mfma_f32_16x16x32_bf16 on the matrix pipe
MFMA_ISSUE = 8     # of which the SIMD's vector issue is held
BLOCK = 12         # MFMAs of one block of layer_bf (two output tiles x six plane products of one k-chunk)
SLAB = 192         # MFMAs of one slab (eight output tiles x four k-chunks x six)
# the f16 form: three plane products instead of six (same cycles per MFMA)
SHAPES = {MFMA: (BLOCK, SLAB), MFMA_F16: (BLOCK // 2, SLAB // 2)}


def cost(ins):
    """Issue cycles of one non-MFMA instruction beside the matrix stream."""
    if ins.startswith(TRANS) or ins.startswith("v_pk_"):
        return 8
    if ins.startswith(("v_", "ds_", "scratch_", "global_", "buffer_", "flat_")):
        return 4
    if ins.startswith("s_nop"):
        f = ins.split()
        return 4 * (int(f[1], 0) + 1) if len(f) > 1 else 4
    return 0


def compile_unit(unit, out_dir):
    from aircraft_amd import build as B

    asm = os.path.join(out_dir, unit + ".s")
    cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get(unit, []), "-S", "--cuda-device-only",
           os.path.join(B.CSRC, unit + ".hip"), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    with open(asm) as fh:
        return fh.read()


def basic_blocks(asm):
    """[label, innermost loop header or None, instructions] per basic block, in text order."""
    blocks = [[None, None, []]]
    for line in asm.split("\n"):
        line = line.strip()
        m = re.match(r"\.(LBB\d+_\d+):(.*)", line)
        if m:
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            blocks.append([m.group(1)[1:], h.group(1) if h else None, []])
            continue
        if line.startswith(";") and "This Loop Header" in line and not blocks[-1][2]:
            blocks[-1][1] = blocks[-1][0]  # a loop header: its own loop
            continue
        if not line or line[0] in ";." or line.endswith(":"):
            continue
        ins = line.split(";")[0].strip()
        if ins:
            blocks[-1][2].append(ins)
    return blocks


def instructions(asm, mfma=MFMA):
    """The instruction stream in the order one trip of each loop executes it: the block placement pass may rotate a loop
    (header in the middle of its text, e.g. the hidden-layer loop cut at the mid-layer barrier), which would put the
    seam between two layer calls inside the region and shift every block and slab sum."""
    blocks = basic_blocks(asm)
    # loops whose own blocks issue the MFMAs: first .. last block of the loop in the text (child loops lie inside)
    for h in sorted({b[1] for b in blocks if b[1] and any(i.startswith(mfma) for i in b[2])}):
        own = [k for k, b in enumerate(blocks) if b[1] == h]
        head = next((k for k in own if blocks[k][0] == h), own[0])
        blocks[own[0]:own[-1] + 1] = blocks[head:own[-1] + 1] + blocks[own[0]:head]
    return [i for b in blocks for i in b[2]]


def analyse(asm, mfma=MFMA):
    """Figures of the region between the first and the last MFMA (`mfma`: its mnemonic, the bf16 form by default) of an
    assembly text."""
    block, slab = SHAPES.get(mfma, (BLOCK, SLAB))
    ins = instructions(asm, mfma)
    idx = [k for k, i in enumerate(ins) if i.startswith(mfma)]
    if len(idx) < 2:
        raise ValueError(f"no {mfma} region")
    gaps, kinds = [], collections.Counter()
    for a, b in zip(idx, idx[1:]):
        seg = ins[a + 1:b]
        if any(x.startswith(("s_cbranch", "s_branch", "s_barrier")) for x in seg):
            gaps.append(None)
            continue
        gaps.append(sum(cost(x) for x in seg))
        for x in seg:
            if cost(x):
                kinds[x.split()[0]] += 1
    priced = [g for g in gaps if g is not None]
    filled = [g if g is not None else 0 for g in gaps]
    hist = collections.Counter(min(g // 8 * 8, 120) for g in priced)
    modelled = sum(max(MFMA_CYCLES, MFMA_ISSUE + g) for g in priced)
    floor = MFMA_CYCLES * len(priced)
    slabs = []
    for s in range(0, len(filled), slab):
        seg = filled[s:s + slab]
        slabs.append({"filler": sum(seg), "modelled": sum(max(MFMA_CYCLES, MFMA_ISSUE + g) for g in seg),
                      "floor": MFMA_CYCLES * len(seg)})
    return {
        "mfma": len(idx),
        "gaps": len(gaps),
        "excluded": len(gaps) - len(priced),
        "empty": sum(g == 0 for g in priced),
        "ge40": sum(g >= 40 for g in priced),
        "gt32": sum(g > 32 for g in priced),
        "gt32_share": sum(g > 32 for g in priced) / len(priced),
        "filler": sum(priced),
        "ds_read_b128": kinds.get("ds_read_b128", 0),
        "capacity": MFMA_ISSUE * len(priced),
        "above_budget": sum(max(0, g - MFMA_ISSUE) for g in priced),
        "modelled": modelled,
        "floor": floor,
        "ratio": modelled / floor,
        "hist": dict(sorted(hist.items())),
        "blocks": [sum(filled[k:k + block]) for k in range(0, len(filled), block)],
        "block": block,
        "slabs": slabs,
        "kinds": kinds.most_common(25),
        "acc_moves": sum(n for k, n in kinds.items() if k.startswith("v_accvgpr_")),
    }


def report(name, r):
    p = print
    p(f"== {name}")
    p(f"MFMAs {r['mfma']}; gaps {r['gaps']} ({r['excluded']} with a barrier or a branch left out)")
    p(f"gaps with no vector work {r['empty']}; carrying >= 40 cycles {r['ge40']}; above 32 cycles {r['gt32']} "
      f"({100 * r['gt32_share']:.1f} %)")
    p(f"filler {r['filler']} cycles ({4 * r['ds_read_b128']} of them ds_read_b128); free capacity (8 x gaps) {r['capacity']}; "
      f"above the 8-cycle budget {r['above_budget']}")
    p(f"modelled {r['modelled']} / floor {r['floor']} = {r['ratio']:.3f}")
    p("modelled per slab: " + " ".join(str(s["modelled"]) for s in r["slabs"])
      + "   (floor " + " ".join(str(s["floor"]) for s in r["slabs"]) + ")")
    p("filler per slab:   " + " ".join(str(s["filler"]) for s in r["slabs"]))
    p("histogram (filler cycles per gap, buckets of 8, last bucket open: gaps):")
    p("  " + "  ".join(f"{k}:{v}" for k, v in r["hist"].items()))
    p(f"filler per {r['block']}-MFMA block:")
    b = r["blocks"]
    for k in range(0, len(b), 16):
        p("  " + " ".join(f"{x:4d}" for x in b[k:k + 16]))
    p("instructions in the gaps: " + ", ".join(f"{k} {n}" for k, n in r["kinds"]))
    p(f"v_accvgpr_* in the gaps: {r['acc_moves']}")
    p("")


def main(argv):
    mfma, units = MFMA, HEADLINE_UNITS
    if argv and argv[0] == "--f16":
        mfma, units, argv = MFMA_F16, F16_UNITS, argv[1:]
    elif len(argv) > 1 and argv[0] == "--mfma":
        mfma, argv = argv[1], argv[2:]
    if argv and argv[0] == "--asm":
        for f in argv[1:]:
            with open(f) as fh:
                report(f, analyse(fh.read(), mfma))
        return
    with tempfile.TemporaryDirectory() as tmp:
        for unit in argv or units:
            report(unit, analyse(compile_unit(unit, tmp), mfma))


if __name__ == "__main__":
    main(sys.argv[1:])
