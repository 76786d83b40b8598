#!/usr/bin/env python3
"""Recover the coefficients of the cubic-fit model from flight trajectories through the simulator (needs an MI355X).

A flight of B glider instances is generated with the golden coefficients at dt = 0.1 s and 10 RK4 sub-steps (the recording
convention of the reference's simulation.h5).  The coefficients are then perturbed and recovered with torch.optim.Adam on
the trajectory loss

    loss = mean ((X(theta) - X_true) / s)^2        s: per-row scale of the true trajectories' step increments

written in plain torch over the differentiable rollout.  `autodiff.rollout(..., params=params)` makes the loss reach the
coefficients: the backward pass is ONE fused reverse sweep (ac_rollout_cgrad_f32) through all 10 sub-steps of every node, and
CoefficientParameters re-installs the changed coefficients before the next forward pass.  The fits span five orders of
magnitude and many entries are exactly zero, so Adam runs in relative coordinates theta = theta_start (1 + s): structural
zeros stay zero, and every coefficient moves by the same fraction per step.

Prints the loss and the relative coefficient error |theta - theta_true| / |theta_true| per epoch.

    python examples/fit_polynomial.py [--batch 256] [--horizon 20] [--epochs 200]
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
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--substeps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--perturb", type=float, default=0.05, help="relative size of the coefficient perturbation")
    args = ap.parse_args(argv)
    import torch
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, autodiff
    from aircraft_amd.synthetic import GLIDER, near_trim_problem

    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=os.path.join(ROOT, "tests", "golden", "poly_coef.npz"),
                               aircraft_config=AircraftConfiguration(dict(GLIDER)), physical_integration_substeps=args.substeps))
    ac.normalise = True
    dev = torch.device("cuda", 0)
    B, H = args.batch, args.horizon
    X0, U = near_trim_problem(B, H, seed=0)
    x0 = torch.tensor(X0, dtype=torch.float32, device=dev)
    U = torch.tensor(U, dtype=torch.float32, device=dev)
    with torch.no_grad():
        X_true = ac.rollout(x0, U, args.dt).clone()
    scale = (X_true[1:] - X_true[:-1]).pow(2).mean(dim=(0, 2)).sqrt().clamp_min(1e-6)[None, :, None]

    params = autodiff.CoefficientParameters(ac)
    true = [p.detach().clone() for p in params.parameters()]
    true_norm = torch.sqrt(sum((t ** 2).sum() for t in true))
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in params.parameters():
            p.mul_(1.0 + args.perturb * torch.randn(p.shape, generator=gen))
    start = [p.detach().clone() for p in params.parameters()]
    rel = [torch.zeros_like(p, requires_grad=True) for p in start]  # theta = start (1 + rel)
    opt = torch.optim.Adam(rel, lr=args.lr)
    losses, errors = [], []
    for epoch in range(args.epochs):
        X = autodiff.rollout(ac, x0, U, args.dt, params=params)   # installs the current coefficients first
        loss = (((X - X_true) / scale) ** 2).mean()
        params.zero_grad()
        loss.backward()
        err = torch.sqrt(sum(((p.detach() - t) ** 2).sum() for p, t in zip(params.parameters(), true))) / true_norm
        with torch.no_grad():
            for s, p, p0 in zip(rel, params.parameters(), start):
                s.grad = p.grad * p0
            opt.step()
            for s, p, p0 in zip(rel, params.parameters(), start):
                p.copy_(p0 * (1.0 + s))
        losses.append(loss.item())
        errors.append(err.item())
        print(f"epoch={epoch:3d} loss={losses[-1]:.6e} coefficient_error={errors[-1]:.6e}", flush=True)
    return losses, errors


if __name__ == "__main__":
    main()
