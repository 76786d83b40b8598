#!/usr/bin/env python3
"""The maximum-a-posteriori trajectory of a recorded flight when the initial estimate is badly wrong: fly a noisy truth from a
range of trims, read the simulated sensors along every flight (Aircraft.sense with a SensorModel: GPS every 10th step, the
others every step), start the estimators from a prior mean several sigma off, and compare, per block of the error state, the
RMS error against the truth of
  - the bank of extended Kalman filters (causal),
  - the filters plus the RTS smoother (one linearisation per step, about the filter's own running estimate),
  - EKF.map_smooth: Gauss-Newton on the MAP cost of the whole log (the iterated extended Kalman smoother), and
  - a sliding window of N steps of it (moving-horizon estimation): the arrival prior of a window is the bank's (x, P) from N
    steps back, the bank being advanced with filter() as the window slides; the window's last node is the estimate of that step.

    python examples/map_smooth.py --model poly --speeds 4 --draws 64
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from aircraft_amd import SensorModel  # noqa: E402
from examples.ekf_track import BLOCKS, SIG_P0, SIG_Q, SIG_R, boxminus, boxplus  # noqa: E402
from examples.glide_polar import make  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=4)
    ap.add_argument("--vmin", type=float, default=30.0)
    ap.add_argument("--vmax", type=float, default=50.0)
    ap.add_argument("--draws", type=int, default=64, help="noise draws per flight")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--window", type=int, default=20, help="N of the sliding-window variant")
    ap.add_argument("--stride", type=int, default=10, help="steps between two windows")
    ap.add_argument("--wide", type=float, default=10.0, help="the prior is this many times SIG_P0 wide")
    ap.add_argument("--off", type=float, default=2.0, help="sigmas of that prior the initial estimate is off by")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    ac = make(args.model)
    trim = ac.trim(np.linspace(args.vmin, args.vmax, args.speeds))
    ok = trim.converged
    if not ok.any():
        raise SystemExit("no instance trimmed")
    m, T, dt, N = int(ok.sum()), args.steps, args.dt, args.window
    n = m * args.draws
    rng = np.random.default_rng(args.seed)
    u = np.repeat(trim.u[:, ok], args.draws, axis=1)
    U = np.repeat(u[None], T, axis=0)
    X = [np.repeat(trim.x[:, ok], args.draws, axis=1)]
    for _ in range(T):
        X.append(boxplus(ac.state_update(X[-1], u, dt), SIG_Q[:, None] * rng.standard_normal((12, n))))
    X = np.stack(X)
    sensors = SensorModel(sigma=SIG_R, period=(10, 10, 1, 1, 1), phase=(9, 9, 0, 0, 0), seed=args.seed)
    Z, mask = (np.stack(a) for a in zip(*(ac.sense(X[k + 1], sensors, k) for k in range(T))))
    sp = args.wide * SIG_P0
    P0 = np.repeat(np.diag(sp ** 2)[:, :, None], n, axis=2)
    d0 = rng.standard_normal((12, n))
    x0 = boxplus(X[0], args.off * sp[:, None] * d0 / np.sqrt((d0 ** 2).sum(0)))  # `off` sigma along a random direction
    bank = ac.ekf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2)
    res = bank.map_smooth(U, dt, Z, mask, iters=args.iters)  # (the bank is not advanced)
    tr = bank.filter(U, dt, Z, mask, record=True)
    sm = bank.smooth(tr)
    bad = (tr.status != 0).any(axis=0) | (sm.status != 0).any(axis=0) | ((res.status & 3) != 0)
    # the sliding window: a second bank runs N steps behind the window's end and supplies the arrival prior
    tail, ends, est = ac.ekf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2), [], []
    for end in range(N, T + 1, args.stride):
        start = end - N
        if ends:
            tail.filter(U[ends[-1] - N:start], dt, Z[ends[-1] - N:start], mask[ends[-1] - N:start])
        w = tail.map_smooth(U[start:end], dt, Z[start:end], mask[start:end], iters=args.iters)
        ends.append(end)
        est.append(w.X[-1])
    print(f"model={args.model}  {m} flights x {args.draws} draws = {n} logs, {T} steps of {dt} s, seed {args.seed}; prior {args.wide:g} x SIG_P0, "
          f"initial estimate {args.off:g} sigma off; {int(bad.sum())} instances reported a status")
    print(f"MAP cost, median over the logs: {np.median(res.cost[:, ~bad], axis=1)}")
    print(f"accepted step lengths per iteration (share of logs): "
          + "; ".join(", ".join(f"{a:g}: {np.mean(al == a):.2f}" for a in np.unique(al)) for al in res.alpha[:, ~bad]))
    err = lambda est, k0=0: np.stack([boxminus(X[k0 + k + 1], est[k]) for k in range(est.shape[0])])[:, :, ~bad]  # noqa: E731
    rms = lambda e, sl: np.sqrt((e[..., sl, :] ** 2).mean())  # noqa: E731
    rows = [("EKF, all steps", err(tr.X)), ("EKF + RTS, all steps", err(sm.X)), ("MAP, all steps", err(res.X)),
            ("EKF + RTS, initial", boxminus(X[0], sm.X0)[:, ~bad]), ("MAP, initial", boxminus(X[0], res.X0)[:, ~bad]),
            ("EKF at window ends", np.stack([boxminus(X[e], tr.X[e - 1]) for e in ends])[:, :, ~bad]),
            (f"MAP window N={N}, ends", np.stack([boxminus(X[e], x) for e, x in zip(ends, est)])[:, :, ~bad])]
    print(f"  {'RMS error':>24s}  " + "  ".join(f"{name:>16s}" for name, _ in BLOCKS))
    for label, a in rows:
        print(f"  {label:>24s}  " + "  ".join(f"{rms(a, sl):16.4f}" for _, sl in BLOCKS))


if __name__ == "__main__":
    main()
