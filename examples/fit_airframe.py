#!/usr/bin/env python3
"""Recover mass, inertia and centre of mass of the glider from flight trajectories through the simulator (needs an MI355X).

A flight of B glider instances is generated with the cubic-fit model at dt = 0.1 s and 10 RK4 sub-steps (the recording
convention of the reference's simulation.h5).  Mass, (Ixx, Iyy, Izz, Ixz) and the three com numbers are then perturbed by 10 % and
recovered with torch.optim.Adam on the trajectory loss

    loss = mean ((X(phi) - X_true) / s)^2          s: per-row scale of the true trajectories' step increments

written in plain torch over the differentiable rollout.  `autodiff.rollout(..., params=frame)` makes the loss reach the eight
numbers: the backward pass is ONE fused reverse sweep (ac_rollout_agrad_f32) through all 10 sub-steps of every node, autograd
carries its 22 raw gradients through I = I0 + m K(com) and the inverse, and AirframeParameters re-installs the changed
constants before the next forward pass.  The eight numbers span four orders of magnitude, so Adam runs in relative
coordinates phi = phi_start (1 + s) (cf. fit_polynomial.py); com_1 of the glider is -1.8e-8, practically zero: its error is
printed in metres, relative to |com|.

Prints the loss and the relative error of each number every 50 iterations.

    python examples/fit_airframe.py [--batch 256] [--horizon 20] [--iters 400]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("mass", "Ixx", "Iyy", "Izz", "Ixz", "com0", "com1", "com2")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.1)
    ap.add_argument("--substeps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--perturb", type=float, default=0.10, help="relative size of the perturbation of each number")
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
    frame = autodiff.AirframeParameters(ac)
    frame.sync()  # the flight is recorded on the float32 numbers the parameters hold
    with torch.no_grad():
        X_true = ac.rollout(x0, U, args.dt).clone()
    scale = (X_true[1:] - X_true[:-1]).pow(2).mean(dim=(0, 2)).sqrt().clamp_min(1e-6)[None, :, None]

    pars = [frame.mass, frame.inertia, frame.com]
    true = [p.detach().clone() for p in pars]
    # the scale of each number's error: itself, and |com| for the three com numbers
    ref = torch.cat([true[0].abs().reshape(1), true[1].abs(), true[2].norm().expand(3)])
    signs = [torch.tensor(1.0), torch.tensor([1.0, -1.0, 1.0, -1.0]), torch.tensor([-1.0, 1.0, 1.0])]
    with torch.no_grad():
        for p, s in zip(pars, signs):
            p.mul_(1.0 + args.perturb * s)
    start = [p.detach().clone() for p in pars]
    rel = [torch.zeros_like(p, requires_grad=True) for p in start]  # phi = start (1 + rel)
    opt = torch.optim.Adam(rel, lr=args.lr)
    losses, errors = [], []
    for it in range(args.iters):
        X = autodiff.rollout(ac, x0, U, args.dt, params=frame)   # installs the current constants first
        loss = (((X - X_true) / scale) ** 2).mean()
        frame.zero_grad()
        loss.backward()
        err = (torch.cat([(p.detach() - t).reshape(-1) for p, t in zip(pars, true)]).abs() / ref).tolist()
        with torch.no_grad():
            for s, p, p0 in zip(rel, pars, start):
                s.grad = p.grad * p0
            opt.step()
            for s, p, p0 in zip(rel, pars, start):
                p.copy_(p0 * (1.0 + s))
        losses.append(loss.item())
        errors.append(err)
        if it % 50 == 0 or it == args.iters - 1:
            print(f"iter={it:4d} loss={losses[-1]:.6e} " + " ".join(f"{k}={e:.3e}" for k, e in zip(NAMES, err)), flush=True)
    return losses, errors


if __name__ == "__main__":
    main()
