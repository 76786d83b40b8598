"""The block-by-block reference of the width-128 plane routes (tests/sens_blocks_ref.py) checked on the CPU: the fp32
restatement of the MLP step with tangents (tests/host_dyn/dyn_host.cpp::host_nn_sens) against the float64 oracle, the cap on
e_ref for every case of the matrix that tests/test_gpu_plane_routes.py runs on the card, and the power of the metric: changes
a kernel could plausibly make (a lost plane product, a stale ring region, a wrong half) made on the float64 side and held
against each case's bar.  No GPU.

Measured here (x86-64, g++ -O1 -ffp-contract=off; the figures travel to parity_report.jsonl as plane_blocks_cpu[...]
and are tabulated in DESIGN.md section 5):
  e_ref over the 32 cases with a host entry (the four sub-stepped ones have none): worst block 7.6e-6 (A[w,w], per-unit dt on
  4 x 128), every case under the 1.25e-5 cap at dt = 2^-4 (at dt = 0.01: 2e-5 .. 7.5e-5 on the diagonal blocks, see
  sens_blocks_ref.DT); the route's own arithmetic never exceeds 4 x the plain-fp32 chain on any block (worst 2.04, B[v,ae] on
  its own scale at the gate edge; <= 1.75 elsewhere).  No deep net needed a scale to pass the gate; the gate-edge shift is 12.
  Flagged on every one of the 346 sampled units, against the bars of k4-bf16 / k4-f16 / k7-bf16 / k3-f16 (worst block of the
  LEAST affected unit / its bar): (a) hidden weights rounded to f16 58 / 71 / 71 / 61, (b) bf16(w) alone 490 / 490 / 344 / 691,
  (c) a layer on its successor's weights >= 1.6e5, (d) a back half from the successor >= 1.2e5.  Their whole-unit A figures in
  the old metric (least .. most affected unit, k4): (a) 4.1e-4 .. 1.3e-3, (b) 3.3e-3 .. 8.1e-3, (c) 0.62 .. 1.9, (d) 0.75 .. 2.0.
  Measured only: the third bf16 weight plane missing (bf16(w) + bf16(w - w1)) is 0.37 .. 0.83 x the bar in the least affected
  unit, 16 / 16 / 306 / 334 of 346 units flagged (old metric: A 2.2e-6 .. 8.9e-6 per unit); single dropped products of the bf16
  route: w1.x1, w1.x2, w2.x1 flag every unit, w2.x2, w1.x3, w3.x1 flag 11 %, 5 %, 1 %; of the f16 route: all three flag every unit."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import MlpData
from tests import sens_blocks_ref as R
from tests.helpers import block_rel_err, f32_exact, make_aircraft, make_oracle, parity_report, synthetic_units, unit_max_rel

CASES = {c.name: c for c in R.all_cases()}


def test_plane_roundings_are_numpy_s():
    rng = np.random.default_rng(11)
    x = (10.0 ** rng.uniform(-9, 4.5, 200_000) * rng.choice([-1.0, 1.0], 200_000)).astype(np.float32)
    x[:4] = [0.0, -0.0, 65504.0, 2.0 ** -25]
    out = np.empty_like(x)
    fp = C.POINTER(C.c_float)
    R.dyn_lib().host_plane_round(1, x.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp))
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).astype(np.float32)  # RNE, gradual underflow, overflow to infinity
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    R.dyn_lib().host_plane_round(2, x.ctypes.data_as(fp), x.size, out.ctypes.data_as(fp))
    u = x.view(np.uint32).astype(np.uint64)
    want = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)
    assert np.array_equal(out.view(np.uint32), want)


@pytest.mark.parametrize("normalise", [True, False])
def test_plain_fp32_restatement_against_the_oracle(normalise):
    """host_nn_sens in mode 0 to the conventions of host_dyn_sens (tests/test_host_dyn.py): exact structure, every unit within
    1e-5 of the oracle in the max norm, on a 3 x 64 net at the suite's dt."""
    ac = make_aircraft("nn", hidden=(64, 64, 64), normalise=normalise)
    X, U = synthetic_units(300, seed=21)
    X, U = f32_exact(X), f32_exact(U)
    Xn, A, B, c = R.host_nn_sens(ac, X, U, 0.01, 0)
    Xr, Ar, Br, cr = make_oracle(ac).step_sens(X, U, 0.01)
    assert block_rel_err(Xn, Xr) < 1e-5
    for got, want in ((A, Ar), (B, Br), (c, cr)):
        assert unit_max_rel(got, want).max() < 1e-5
    R.assert_exact_structure(A, B)
    # per-unit dt is the scalar one, unit by unit
    dts = f32_exact(np.random.default_rng(2).uniform(0.005, 0.02, 40))
    per = R.host_nn_sens(ac, X[:, :40], U[:, :40], dts, 0)
    for k in (0, 17, 39):
        one = R.host_nn_sens(ac, X[:, k:k + 1], U[:, k:k + 1], float(dts[k]), 0)
        assert all(np.array_equal(a[..., k], b[..., 0]) for a, b in zip(per, one))


def test_the_routes_modes_are_the_numpy_emulations():
    """One hidden layer of mode 1 / mode 2 is layer_f16("keep") of tests/test_mlp_f16_planes.py / the product order of
    tests/test_mlp_bf16_planes.py: through the step they differ from mode 0 by the planes' truncation (2^-22 of a term), not more."""
    c = CASES["k4-f16"]
    X, U, dt, idx = R.case_units(c)
    Xs, Us = X[:, idx[:64]], U[:, idx[:64]]
    ac = R.case_aircraft(c)
    h0 = R.host_nn_sens(ac, Xs, Us, dt, 0)
    for mode in (1, 2):
        hm = R.host_nn_sens(ac, Xs, Us, dt, mode)
        assert not all(np.array_equal(a, b) for a, b in zip(h0, hm))
        assert max(R.worst(R.block_errors(hm[1:], h0[1:])).values()) < 2e-5


@pytest.mark.parametrize("name", list(CASES))
def test_e_ref_is_under_the_cap(name):
    case = CASES[name]
    ref, e_ref, e0, em, eF = R.case_reference(case)
    net, scale = R.case_net(case)
    if case.substeps > 1:  # no host entry for sub-steps: held to the suite's existing lines on the card
        assert e_ref is None
        return
    worst_block = max(e_ref, key=e_ref.get)
    ratio = {k: em[k] / max(e0[k], 1e-300) for k in em}
    print(f"{name}: units {ref[0].shape[1]} hidden scale {scale} e_ref worst {worst_block} {e_ref[worst_block]:.2e} x+ {eF:.2e}; "
          f"route / fp32 worst {max(ratio.values()):.2f} ({max(ratio, key=ratio.get)})")
    parity_report(f"plane_blocks_cpu[{name}]", units=int(ref[0].shape[1]), hidden_scale=scale, e_ref=e_ref, e_fp32=e0, e_route=em,
                  state=eF, route_over_fp32=max(ratio.values()))
    assert all(v <= R.E_REF_CAP for v in e_ref.values()), {k: v for k, v in e_ref.items() if v > R.E_REF_CAP}
    assert eF < 1e-5
    # blocks the net reaches are populated on the sampled units (nothing is checked only through the floor)
    sc = R.block_scales(ref[1:])
    fam_max = np.max(np.stack([sc[k] for k in sc if k.startswith("A[")]), axis=0)
    for k in ("A[w,q]", "A[w,v]", "A[v,w]"):
        assert np.median(sc[k] / fam_max) > R.FLOOR, (k, float(np.median(sc[k] / fam_max)))
    # a route whose own arithmetic is more than 4 x worse than the plain fp32 chain on a block is a finding about the route
    assert max(ratio.values()) <= 4.0, {k: v for k, v in ratio.items() if v > 4.0}


def test_gate_edge_net_sits_at_the_floor():
    k = R.gate_edge_shift()
    syn = MlpData.synthetic((128,) * 4, seed=42)
    ok = R.with_weights(syn, [syn.weights[0] * np.float32(2.0 ** -k)] + syn.weights[1:])
    out = R.with_weights(syn, [syn.weights[0] * np.float32(2.0 ** -(k + 1))] + syn.weights[1:])
    assert R.host_f16_gate(ok)[0] == 0 and R.host_f16_gate(out)[0] == 3
    # its largest tangent entering the first hidden product is within a factor 2 of 2^-14: the hi plane of most is subnormal
    t1 = np.abs(ok.weights[0]).max()
    assert 2.0 ** -14 <= t1 < 2.0 ** -12, t1
    print(f"gate edge: W0 2^-{k}, max|W0| = {t1:.3e} = {t1 * 2 ** 14:.2f} x 2^-14")


# ---- the metric can fail ------------------------------------------------------------------------------------------------
def f16_w(w):
    return w.astype(np.float16).astype(np.float32)


def bf16_w(w):
    u = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def mutations(net):
    """name -> MlpData: the float64 side of a change a kernel could make to the hidden layers"""
    W, b = net.weights, net.biases
    hid = range(1, len(W) - 1)

    def swap(f):
        return R.with_weights(net, [f(w) if l in hid else w for l, w in enumerate(W)])

    stale = [w.copy() for w in W]; stale_b = [v.copy() for v in b]
    stale[1], stale_b[1] = W[2].copy(), b[2].copy()      # layer 1 runs on layer 2's region (weights and bias: the front half holds both)
    half = [w.copy() for w in W]
    half[1][64:] = W[2][64:]                             # output tiles 4 .. 7 of layer 1 from layer 2's back half
    return {"a_f16_weights": swap(f16_w), "b_bf16_one_plane": swap(bf16_w),
            "c_stale_region": MlpData(stale, stale_b, net.act, net.input_mean, net.input_std, net.output_mean, net.output_std),
            "d_wrong_back_half": R.with_weights(net, half),
            "bf16_two_planes": swap(lambda w: (bf16_w(w) + bf16_w(w - bf16_w(w))).astype(np.float32))}


ASSERTED = ("a_f16_weights", "b_bf16_one_plane", "c_stale_region", "d_wrong_back_half")


@pytest.mark.parametrize("name", ["k4-bf16", "k4-f16", "k7-bf16", "k3-f16"])
def test_changes_a_kernel_could_make_exceed_the_bar_on_every_unit(name):
    case = CASES[name]
    X, U, dt, idx = R.case_units(case)
    ref, e_ref, *_ = R.case_reference(case)
    net, _ = R.case_net(case)
    Xs, Us = X[:, idx], U[:, idx]
    for mname, mnet in mutations(net).items():
        mut = R.case_oracle(case, mnet).step_sens(Xs, Us, dt)
        err = R.block_errors(mut[1:], ref[1:])
        over = np.stack([err[k] / (R.BAR_FACTOR * e_ref[k]) for k in err])    # (blocks, units): error / bar
        per_unit = over.max(axis=0)
        least = int(per_unit.argmin())
        which = list(err)[int(over[:, least].argmax())]
        old = {k: unit_max_rel(g, w) for k, g, w in (("A", mut[1], ref[1]), ("B", mut[2], ref[2]), ("c", mut[3], ref[3]))}
        print(f"{name} {mname}: least affected unit {per_unit.min():.3g} x its bar ({which}), median {np.median(per_unit):.3g}; "
              f"whole-unit A {old['A'].min():.1e} .. {old['A'].max():.1e} B {old['B'].max():.1e} c {old['c'].max():.1e}; "
              f"units flagged {int((per_unit > 1).sum())} / {per_unit.size}")
        parity_report(f"plane_blocks_cpu[{name}/{mname}]", least_over_bar=float(per_unit.min()), block=which,
                      median_over_bar=float(np.median(per_unit)), flagged=int((per_unit > 1).sum()), units=int(per_unit.size),
                      whole_unit_A=[float(old["A"].min()), float(old["A"].max())], whole_unit_B=float(old["B"].max()),
                      whole_unit_c=float(old["c"].max()),
                      blocks_median_over_bar={k: float(np.median(over[i])) for i, k in enumerate(err)})
        if mname in ASSERTED:
            assert (per_unit > 1.0).all(), (name, mname, int((per_unit <= 1).sum()), float(per_unit.min()))


@pytest.mark.parametrize("name,mode,nprod", [("k4-bf16", 2, 6), ("k4-f16", 1, 3)])
def test_single_dropped_products_next_to_the_bar(name, mode, nprod):
    """Measured, not required: the host route with one product left out, block by block against 8 x e_ref — which single
    products the bar can see.  (The large ones must show; the smallest are below any fp32 comparison.)"""
    case = CASES[name]
    X, U, dt, idx = R.case_units(case)
    ref, e_ref, *_ = R.case_reference(case)
    sub = idx[:96]
    Xs, Us = X[:, sub], U[:, sub]
    refs = tuple(a[..., :96] for a in ref)
    ac = R.case_aircraft(case)
    seen = {}
    for drop in range(nprod):
        h = R.host_nn_sens(ac, Xs, Us, dt, mode, drop)
        err = R.block_errors(h[1:], refs[1:])
        over = np.stack([err[k] / (R.BAR_FACTOR * e_ref[k]) for k in err])
        per_unit = over.max(axis=0)
        blk = list(err)[int(np.median(over, axis=1).argmax())]
        seen[drop] = float((per_unit > 1).mean())
        print(f"{name} drop {drop}: flagged {seen[drop] * 100:.0f} % of units, median unit {np.median(per_unit):.3g} x bar, "
              f"least {per_unit.min():.3g}; block {blk}: " + " ".join(f"{k} {np.median(over[i]):.2g}" for i, k in enumerate(err) if np.median(over[i]) > 0.5))
        parity_report(f"plane_blocks_cpu[{name}/drop{drop}]", flagged_fraction=seen[drop], median_over_bar=float(np.median(per_unit)),
                      least_over_bar=float(per_unit.min()))
    # the leading product carries the whole result: without it every unit is far outside
    lead = 0 if mode == 2 else 2
    assert seen[lead] == 1.0
