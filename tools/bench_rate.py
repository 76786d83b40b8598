#!/usr/bin/env python3
"""Times what the exact control-rate treatment costs: the Riccati pass that carries u_{k-1} (ac_ilqr_backward_rate_f32) beside
the pass it stands in for (ac_ilqr_backward_goal_f32: node arrays, Hz, control gradient), and the closed-loop rollout with and
without the gains on the previous control (ac_rollout_policy_rate_f32 / ac_rollout_policy_f32).

    python tools/bench_rate.py                      # B = 4096, H = 50; rollouts through the cubic fits and the 4x128 net
    python tools/bench_rate.py --batch 256 --models poly

Inputs are random (the kernels' work does not depend on the values).  Every part is warmed up on its real shapes, then timed
with device events around a window of repeated launches at least --window seconds long; the variants alternate over --rounds
rounds, the median round is reported with the spread.  One JSON line."""
import argparse
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
    ap.add_argument("--alphas", type=int, default=5)
    ap.add_argument("--models", type=str, default="poly,nn")
    ap.add_argument("--hidden", type=str, default="128,128,128,128")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rate.py needs the GPU: there is nothing to time without it")
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
    from aircraft_amd.control import ILQR, QuadraticCost
    from aircraft_amd.synthetic import GLIDER, TRIM_STATE

    dev = torch.device("cuda", 0)
    B, H, na = args.batch, args.nodes, args.alphas
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
    ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(s, device=dev, generator=g)  # noqa: E731
    out = {"B": B, "H": H, "n_alpha": na, "ms": {}, "spread_over_rounds": {}}

    def run(parts):
        rounds = {k: [] for k in parts}
        for _ in range(args.rounds):
            for k, fn in parts.items():
                rounds[k].append(timed(torch, fn, args.window))
        for k, v in rounds.items():
            out["ms"][k] = float(np.median(v))
            out["spread_over_rounds"][k] = float((max(v) - min(v)) / np.median(v))

    # ---- backward passes on the same synthetic linearisation -------------------------------------------------------------------
    poly = os.path.join(ROOT, "tests", "golden", "poly_coef.npz")
    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=poly, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    cost = QuadraticCost(q=[1.0] * 13, qf=[2.0] * 13, r=[0.5] * 7, reg=0.25)
    il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost)
    A = torch.eye(13, device=dev)[None, :, :, None] + 0.05 * rn(H, 13, 13, B)
    Bm = 0.1 * rn(H, 13, 7, B)
    X, U = rn(H + 1, 13, B), rn(H, 7, B)
    node = (ru(0.2, 2.0, H + 1, 13, B), rn(H + 1, 13, B), 0.5 * rn(H + 1, 13, B))
    S = 0.03 * rn(H, 21, 21, B)
    Hz = (S + S.transpose(1, 2)).contiguous()
    ug, rg, rh = 0.5 * rn(H, 7, B), 0.5 * rn(H, 7, B), ru(0.2, 2.0, H, 7, B)
    o3 = (torch.empty((H, 7, 13, B), device=dev), torch.empty((H, 7, B), device=dev), torch.empty((2, B), device=dev))
    o4 = o3 + (torch.empty((H, 7, 7, B), device=dev),)
    run({
        "backward_goal": lambda: il.backward(X, U, A, Bm, out=o3, Hz=Hz, node=node, uglin=ug),
        "backward_rate_node_newton": lambda: il.backward(X, U, A, Bm, out=o4, Hz=Hz, node=node, rate=(rg, rh)),
        "backward_node": lambda: il.backward(X, U, A, Bm, out=o3, node=node),
        "backward_rate_node": lambda: il.backward(X, U, A, Bm, out=o4, node=node, rate=(rg, rh)),
    })
    assert bool(torch.isfinite(o4[0]).all()) and bool(torch.isfinite(o4[3]).all())
    out["backward_rate_over_goal"] = out["ms"]["backward_rate_node_newton"] / out["ms"]["backward_goal"]
    out["backward_rate_node_over_goal"] = out["ms"]["backward_rate_node"] / out["ms"]["backward_goal"]
    out["backward_rate_node_over_node"] = out["ms"]["backward_rate_node"] / out["ms"]["backward_node"]

    # ---- closed-loop rollouts ---------------------------------------------------------------------------------------------------
    for model in args.models.split(","):
        if model == "nn":
            path = MlpData.synthetic(tuple(int(h) for h in args.hidden.split(",")), seed=42)
        else:
            path = poly
        acm = Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=path, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                                    physical_integration_substeps=1))
        ilm = ILQR(system=acm, dt=0.01, num_nodes=H, cost=QuadraticCost())
        x0 = torch.from_numpy(np.repeat(TRIM_STATE[:, None], B, axis=1).astype(np.float32)).to(dev)
        Un = torch.zeros((H, 7, B), device=dev)
        Xn = ilm.rollout(x0, Un)
        K, Kp, kff = 0.01 * rn(H, 7, 13, B), 0.1 * rn(H, 7, 7, B), 0.1 * rn(H, 7, B)
        al = [1.0, 0.5, 0.25, 0.1, 0.03, 0.01, 0.003, 0.001][:na]
        oc = (torch.empty((H + 1, 13, na * B), device=dev), torch.empty((H, 7, na * B), device=dev))
        run({
            f"policy_{model}": lambda: ilm.forward(x0, Xn, Un, K, kff, alphas=al, out=oc),
            f"policy_rate_{model}": lambda: ilm.forward(x0, Xn, Un, K, kff, alphas=al, out=oc, Kp=Kp),
        })
        out[f"kernel_{model}"] = acm.last_launch()[0]
        out[f"policy_rate_over_plain_{model}"] = out["ms"][f"policy_rate_{model}"] / out["ms"][f"policy_{model}"]
        assert bool(torch.isfinite(oc[0]).all())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
