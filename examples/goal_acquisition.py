#!/usr/bin/env python3
"""The reference's goal-acquisition problem on the batched sweep (needs an MI355X).

What /root/reference/main/control/control.py:157-213 sets up — glider from data/glider/problem_definition.json, the
polynomial coefficient model every reference driver uses (:166), the driver's centre-of-mass override (:172), trim state at
80 m/s and 200 m, N = 400 nodes of dt = 0.01 s, goal (150, 0), vel_param = +1, Controller.loss (:44-68) with the final
velocity constraint v_x(N) < -2 — solved here for B random restarts at once (perturbed initial controls) by the iLQR sweep
on the exact loss, where the reference hands ONE instance to IPOPT.  Prints the loss history (mean / best over the batch).

    python examples/goal_acquisition.py [--batch 64] [--iters 12] [--time variable] [--rate exact] [--box qp]
    python examples/goal_acquisition.py --shooting multiple [--guess rollout|line]

--rate: how the backward pass models the control-rate term — frozen neighbours (the default) or exactly, with u_{k-1} carried
through the Riccati pass.  The loss that is printed is the exact one either way.
--reg: the Levenberg term on Q_uu; default 1 with --rate frozen, 100 with --rate exact.  The frozen model's 4e4 on the diagonal
of Q_uu damps every step by itself; the exact model has no curvature along smooth control changes, and with reg = 1 its steps
are too long for the line search on most restarts (profiles/goal_acquisition_rate_*.txt).
--box: where the control box acts — clip (the default: in the closed-loop rollout only) or qp (in the backward pass too: a QP per
node, control-limited DDP).
--shooting multiple: Gauss-Newton multiple shooting — the states are decision variables too, the line search evaluates every
candidate as independent nodes and runs on the merit  loss + mu sum |defect|; the loss and the largest defect are printed.
--guess (with it): the state guess — rollout (of the initial controls: no gaps) or line (positions interpolated from the initial
state to the goal at the initial height, every other row held at the initial state).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--nodes", type=int, default=400)
    ap.add_argument("--time", choices=("fixed", "variable"), default="fixed")
    ap.add_argument("--rate", choices=("frozen", "exact"), default="frozen")
    ap.add_argument("--reg", type=float, default=None)
    ap.add_argument("--box", choices=("clip", "qp"), default="clip")
    ap.add_argument("--shooting", choices=("single", "multiple"), default="single")
    ap.add_argument("--guess", choices=("rollout", "line"), default="rollout")
    args = ap.parse_args()
    reg = args.reg if args.reg is not None else (100.0 if args.rate == "exact" else 1.0)
    import torch
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts
    from aircraft_amd.control import GoalAcquisition
    from aircraft_amd.synthetic import GLIDER

    poly = os.path.join(ROOT, "tests", "golden", "poly_coef.npz")  # the reference's fitted_models_casadi.pkl, decoded
    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=poly, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    ac.com = np.array([0.0131991, -1.78875e-08, 0.00313384])       # control.py:169-172
    dev = torch.device("cuda", 0)
    B, H = args.batch, args.nodes
    x0 = torch.tensor([0, 0, -200, 80, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=dev)[:, None].expand(13, B).contiguous()
    rng = np.random.default_rng(0)
    U0 = np.zeros((H, 7, B), dtype=np.float32)
    U0[:, :3] = rng.normal(0, 0.3, (1, 3, B))                      # random restarts: a constant offset on the three surfaces
    il = GoalAcquisition(system=ac, goal=(150.0, 0.0), dt=0.01, num_nodes=H, vel_param=1.0, time=args.time,
                         alphas=(1.0, 0.5, 0.25, 0.1, 0.03), reg=reg, rate=args.rate, box=args.box, shooting=args.shooting)
    kw = {}
    if args.guess == "line":
        assert args.shooting == "multiple", "--guess line needs --shooting multiple: single shooting takes no state guess"
        s = torch.linspace(0.0, 1.0, H + 1, device=dev)[:, None]
        X0 = x0[None].expand(H + 1, 13, B).clone()
        X0[:, 0] = x0[0][None] + s * (150.0 - x0[0][None])
        X0[:, 1] = x0[1][None] + s * (0.0 - x0[1][None])
        kw["X0"] = X0
    X, U, hist = il.solve(x0, torch.from_numpy(U0).to(dev), iters=args.iters, al_every=4, **kw)
    h = hist.cpu().numpy()
    dh = il.defect_history.cpu().numpy() if args.shooting == "multiple" else None
    for i, row in enumerate(h):
        gap = f"  defect max {dh[i].max():10.3e}" if dh is not None else ""
        print(f"[rate={args.rate} reg={reg:g} box={args.box} shooting={args.shooting}] sweep {i:2d}  loss mean {row.mean():14.1f}  best {row.min():14.1f}{gap}")
    xN = X[-1].cpu().numpy()
    b = int(h[-1].argmin())
    print(f"best instance {b}: final p = ({xN[0, b]:.1f}, {xN[1, b]:.1f}, {xN[2, b]:.1f}) m, v = ({xN[3, b]:.1f}, {xN[4, b]:.1f}, {xN[5, b]:.1f}) m/s, "
          f"goal (150, 0); v_x(N) < -2 violated by {float(il.update_goal_multiplier(X)[b]):.2f} m/s")
    if args.box == "qp":
        act, stat = il.last_active.cpu().numpy(), il.qp_stat.cpu().numpy()
        print(f"last backward pass: {((act == 1) | (act == -1))[:, :3].mean():.1%} of the surface entries clamped, "
              f"most QP iterations {int(stat[0].max())}, nodes at a cap {int(stat[1].sum())}")


if __name__ == "__main__":
    main()
