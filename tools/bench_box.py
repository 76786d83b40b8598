#!/usr/bin/env python3
"""Times what the control box in the backward pass costs: each of the eight box kernels (ac_ilqr_backward_box_f32,
ac_ilqr_backward_rate_box_f32) beside the unboxed kernel of the same <NODE, NEWTON> (ac_ilqr_backward_newton_f32 / _goal_f32 /
_rate_f32 — instantiations this option does not touch), in two regimes:

    inactive   bounds +-1e6: every QP ends after one Newton iteration, nothing is clamped
    clamped    U clipped into a symmetric box of --half-width: roughly a third of the rows clamped (the fraction is reported)

    python tools/bench_box.py                      # B = 4096, H = 50
    python tools/bench_box.py --out profiles/box_bench.json

Inputs are random, in the shape of tests/riccati_ref.synthetic_riccati.  Every part is warmed up on its real shapes, then timed with
device events around a window of repeated launches at least --window seconds long; the variants alternate over --rounds rounds,
the median round is reported with the spread.  One JSON line."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.bench_mppi import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--half-width", type=float, default=0.5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_box.py needs the GPU: there is nothing to time without it")
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts
    from aircraft_amd.build import source_sha
    from aircraft_amd.control import ILQR, QuadraticCost
    from aircraft_amd.synthetic import GLIDER

    dev = torch.device("cuda", 0)
    B, H = args.batch, args.nodes
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(s, device=dev, generator=g)  # noqa: E731
    out = {"B": B, "H": H, "half_width": args.half_width, "source_sha": source_sha(), "ms": {}, "spread_over_rounds": {}, "ratio": {},
           "clamped_fraction": {}, "qp_iterations_max": {}, "qp_capped_nodes": {}}

    poly = os.path.join(ROOT, "tests", "golden", "poly_coef.npz")
    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=poly, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    base = QuadraticCost(q=[1.0] * 13, qf=[2.0] * 13, r=[0.5] * 7, reg=0.25)
    wide, tight = copy.deepcopy(base), copy.deepcopy(base)
    wide.u_min, wide.u_max = [-1e6] * 7, [1e6] * 7
    tight.u_min, tight.u_max = [-args.half_width] * 7, [args.half_width] * 7
    il = {"inactive": ILQR(system=ac, dt=0.01, num_nodes=H, cost=wide, box="qp"),
          "clamped": ILQR(system=ac, dt=0.01, num_nodes=H, cost=tight, box="qp")}
    A = torch.eye(13, device=dev)[None, :, :, None] + 0.05 * rn(H, 13, 13, B)
    Bm = 0.1 * rn(H, 13, 7, B)
    X, Ufree = rn(H + 1, 13, B), rn(H, 7, B)
    Us = {"inactive": Ufree, "clamped": Ufree.clamp(-args.half_width, args.half_width).contiguous()}
    node = (ru(0.2, 2.0, H + 1, 13, B), rn(H + 1, 13, B), 0.5 * rn(H + 1, 13, B))
    S = 0.03 * rn(H, 21, 21, B)
    Hz = (S + S.transpose(1, 2)).contiguous()
    ug, rg, rh = 0.5 * rn(H, 7, B), 0.5 * rn(H, 7, B), ru(0.2, 2.0, H, 7, B)
    o3 = (torch.empty((H, 7, 13, B), device=dev), torch.empty((H, 7, B), device=dev), torch.empty((2, B), device=dev))
    o4 = o3 + (torch.empty((H, 7, 7, B), device=dev),)
    ex = (torch.empty((H, 7, B), device=dev, dtype=torch.int8), torch.empty((2, B), device=dev, dtype=torch.int32))
    variants = {   # name -> keyword arguments of ILQR.backward
        "gn": dict(node=None), "node": dict(node=node), "newton": dict(node=None, Hz=Hz), "goal": dict(node=node, Hz=Hz, uglin=ug),
        "rate_gn": dict(node=None, rate=(rg, rh)), "rate_node": dict(node=node, rate=(rg, rh)),
        "rate_newton": dict(node=None, Hz=Hz, rate=(rg, rh)), "rate_node_newton": dict(node=node, Hz=Hz, rate=(rg, rh)),
    }
    for name, kw in variants.items():
        o = o4 if "rate" in kw else o3
        parts = {f"{name}/unboxed": lambda: il["inactive"].backward(X, Ufree, A, Bm, out=o, **kw)}
        for regime in il:
            parts[f"{name}/box_{regime}"] = (lambda r: lambda: il[r].backward(X, Us[r], A, Bm, out=o + ex, box=True, **kw))(regime)
        rounds = {k: [] for k in parts}
        for _ in range(args.rounds):          # the variants alternate within a round
            for k, fn in parts.items():
                rounds[k].append(timed(torch, fn, args.window))
        for k, v in rounds.items():
            out["ms"][k] = float(np.median(v))
            out["spread_over_rounds"][k] = float((max(v) - min(v)) / np.median(v))
        for regime in il:
            parts[f"{name}/box_{regime}"]()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(o[0]).all())
            k = f"{name}/box_{regime}"
            out["ratio"][k] = out["ms"][k] / out["ms"][f"{name}/unboxed"]
            out["clamped_fraction"][k] = float((ex[0] != 0).float().mean())
            out["qp_iterations_max"][k] = int(ex[1][0].max())
            out["qp_capped_nodes"][k] = int(ex[1][1].sum())
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
