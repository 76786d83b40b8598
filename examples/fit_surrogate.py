#!/usr/bin/env python3
"""Fit the MLP surrogate to flight trajectories through the simulator (needs an MI355X).

Short rollouts of B glider instances are generated with the shipped 5-16-32-6 coefficient net (the "true" net); the weights
are then perturbed and recovered with torch.optim.Adam on the trajectory loss

    loss = mean ((X(theta) - X_true) / s)^2        s: per-row scale of the true trajectories' step increments

written in plain torch over the differentiable rollout.  `autodiff.rollout(..., params=params)` makes the loss reach the
network: the backward pass is ac_rollout_wgrad_f32 (the reverse recurrence of the rollout, then the weight-gradient kernel
over the B H steps), and MlpParameters re-installs the changed weights before the next forward pass.

Prints the loss per iteration.

    python examples/fit_surrogate.py [--batch 256] [--horizon 20] [--iters 200]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--perturb", type=float, default=0.05, help="relative size of the weight perturbation")
    args = ap.parse_args(argv)
    import torch
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData, autodiff
    from aircraft_amd.synthetic import GLIDER, near_trim_problem

    w = np.load(os.path.join(ROOT, "tests", "golden", "scaledmodel_weights.npz"))  # the reference checkpoint, decoded
    data = MlpData([w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0], w["input_mean"], w["input_std"],
                   w["output_mean"], w["output_std"])
    ac = Aircraft(AircraftOpts(coeff_model_type="nn", coeff_model_path=data, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    ac.normalise = True
    dev = torch.device("cuda", 0)
    B, H = args.batch, args.horizon
    X0, _ = near_trim_problem(B, H, seed=0)
    x0 = torch.tensor(X0, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    U = np.zeros((H, 7, B), dtype=np.float32)
    U[:, :3] = rng.uniform(-3.0, 3.0, (1, 3, B)) + rng.uniform(-1.0, 1.0, (H, 3, B))  # aileron, elevator, rudder [deg]
    U = torch.from_numpy(U).to(dev)
    with torch.no_grad():
        X_true = ac.rollout(x0, U, args.dt).clone()
    scale = (X_true[1:] - X_true[:-1]).pow(2).mean(dim=(0, 2)).sqrt().clamp_min(1e-6)[None, :, None]

    params = autodiff.MlpParameters(ac)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in params.parameters():
            p.mul_(1.0 + args.perturb * torch.randn(p.shape, generator=gen))
    opt = torch.optim.Adam(params.parameters(), lr=args.lr)
    losses = []
    for it in range(args.iters):
        opt.zero_grad()
        X = autodiff.rollout(ac, x0, U, args.dt, params=params)   # installs the current weights first
        loss = (((X - X_true) / scale) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
        print(f"it={it:3d} loss={losses[-1]:.6e}", flush=True)
    return losses


if __name__ == "__main__":
    main()
