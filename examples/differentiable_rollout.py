#!/usr/bin/env python3
"""Single shooting with torch.optim through the simulator (needs an MI355X).

B glider instances (the cubic-fit coefficient model every reference driver uses) start near trim with their goals spread
around where the uncontrolled glide ends; the control sequences U (H, 7, B) are optimised with torch.optim.Adam on a loss written
in plain torch over the differentiable rollout (aircraft_amd.autodiff.rollout: the forward pass is ac_rollout_f32, the backward
pass the reverse-mode kernel ac_rollout_vjp_f32):

    loss = mean_b |p_H - goal_b|^2 / scale  +  w_rate * mean (U[k+1] - U[k])^2

Prints the loss per iteration.

    python examples/differentiable_rollout.py [--batch 256] [--horizon 100] [--iters 60]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--w-rate", type=float, default=1e-3)
    args = ap.parse_args()
    import torch
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, autodiff
    from aircraft_amd.synthetic import GLIDER, near_trim_problem

    poly = os.path.join(ROOT, "tests", "golden", "poly_coef.npz")  # the reference's fitted_models_casadi.pkl, decoded
    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=poly, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    ac.com = np.array([0.0131991, -1.78875e-08, 0.00313384])       # the reference driver's centre-of-mass override
    dev = torch.device("cuda", 0)
    B, H = args.batch, args.horizon
    X0, _ = near_trim_problem(B, H, seed=0)  # near-trim glides (RK4 at dt <= 0.01 stays inside its stability region)
    x0 = torch.tensor(X0, dtype=torch.float32, device=dev)
    with torch.no_grad():  # where the uncontrolled glide ends: the goals are offsets from it
        p_free = ac.rollout(x0, torch.zeros((H, 7, B), device=dev), args.dt)[-1, :3]
    rng = np.random.default_rng(0)
    offset = torch.tensor(np.stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-3, 3, B)]),
                          dtype=torch.float32, device=dev)
    goal = p_free + offset
    scale = float((offset ** 2).sum(0).mean())
    # aileron, elevator, rudder (deg) are optimised; thrust rows (no effect on the glider) and flaps stay at zero
    mask = torch.tensor([1, 1, 1, 0, 0, 0, 0], dtype=torch.float32, device=dev)[None, :, None]
    U = torch.zeros((H, 7, B), device=dev, requires_grad=True)
    opt = torch.optim.Adam([U], lr=args.lr)
    for it in range(args.iters):
        opt.zero_grad()
        Um = U.clamp(-10.0, 10.0) * mask  # (deg: keep the surfaces inside the range the fits were made on)
        X = autodiff.rollout(ac, x0, Um, args.dt)
        miss = ((X[-1, :3] - goal) ** 2).sum(0).mean() / scale
        rate = ((Um[1:] - Um[:-1]) ** 2).mean()
        loss = miss + args.w_rate * rate
        loss.backward()
        opt.step()
        print(f"it={it:3d} loss={loss.item():.6e} miss={miss.item():.4e} rate={rate.item():.3e}", flush=True)


if __name__ == "__main__":
    main()
