#!/usr/bin/env python3
"""The goal problem of examples/random_restart_mpc.py solved by sampling: batched MPPI on the plain rollout engine.

    python examples/mppi_goal.py --model poly --batch 64 --samples 1024 --horizon 50

Every instance starts from the same trimmed glider with zero controls (the actuation weight is 1e-2 here, not the 0.5 of
random_restart_mpc.py: white control noise is scored by it, and at 0.5 no perturbed candidate beats zero controls); each iteration draws `--samples` perturbed control
sequences per instance in the kernel, rolls all of them out in one launch, and blends them by exp(-cost / temperature).
Prints one JSON line: per-iteration mean cost, mean effective sample size, and milliseconds per iteration.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--temperature", type=float, default=0.2, help="of the order of the candidates' cost spread")
    ap.add_argument("--sigma", type=float, default=0.5, help="std of the noise on aileron, elevator and rudder (deg)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--hidden", type=str, default="128,128,128,128")
    ap.add_argument("--model", type=str, default="poly", choices=["default", "poly", "nn"])
    ap.add_argument("--poly-path", type=str, default=os.path.join(ROOT, "tests", "golden", "poly_coef.npz"))
    args = ap.parse_args()

    import torch

    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
    from aircraft_amd.control import ILQR, MPPI, QuadraticCost
    from aircraft_amd.synthetic import GLIDER, TRIM_STATE

    dev = torch.device("cuda", 0)
    if args.model == "nn":
        path = MlpData.synthetic(tuple(int(h) for h in args.hidden.split(",")), seed=42)
    else:
        path = args.poly_path if args.model == "poly" else ""
    ac = Aircraft(AircraftOpts(coeff_model_type=args.model, coeff_model_path=path,
                               aircraft_config=AircraftConfiguration(dict(GLIDER)), physical_integration_substeps=1))
    H, B = args.horizon, args.batch
    T = H * 0.01
    cost = QuadraticCost.goal((50.0 * T, 2.0), w_goal=1.0, height=-200.0, w_height=1.0, w_lateral_speed=0.5, r=1e-2, reg=1.0)
    problem = ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost)
    mppi = MPPI(problem, samples=args.samples, sigma=(args.sigma,) * 3 + (0.0,) * 4, temperature=args.temperature, seed=args.seed)

    x0 = torch.from_numpy(np.repeat(TRIM_STATE[:, None], B, axis=1).astype(np.float32)).to(dev)
    U = torch.zeros((H, 7, B), device=dev)
    X = problem.rollout(x0, U)
    mppi.iterate(x0, X.clone(), U.clone())  # untimed warm-up on the real shapes: workspaces are allocated on first use
    mppi.set_iteration(0)
    J0 = mppi.nominal_cost(X, U, torch.empty((B,), device=dev))
    costs, ess, ms = [float(J0.mean())], [], []
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        J, _ = mppi.iterate(x0, X, U)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        costs.append(float(J.mean()))
        ess.append(float(mppi.last_stats[1].mean()))
    print(json.dumps({"model": args.model, "batch": B, "samples": args.samples, "horizon": H, "iters": args.iters,
                      "temperature": args.temperature, "sigma": args.sigma, "mean_cost": costs, "effective_sample_size": ess,
                      "ms_per_iteration": ms, "rollouts_per_s": B * args.samples / (min(ms) * 1e-3)}))


if __name__ == "__main__":
    main()
