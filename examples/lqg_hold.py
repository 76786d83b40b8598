#!/usr/bin/env python3
"""examples/lqr_hold.py's scenario flown on the ESTIMATE: the LQR about each steady flight sees only what a filter bank gives
it.  The truth is driven by process noise, the sensors (GPS every 10th step, the others at every step) are simulated on the
device, and the EKF and the UKF bank fly the same flights, noise draws and starting estimates side by side
(Aircraft.rollout_lqg).  Prints the RMS steady-flight error of both against the loop that is handed the true state under the
same process noise, the mean NIS per used row and the mean NEES / 12 (1 for a consistent filter).

    python examples/lqg_hold.py --model poly --speeds 4 --draws 256
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.ekf_track import SIG_P0, SIG_Q, SIG_R, boxplus  # noqa: E402
from examples.glide_polar import make  # noqa: E402
from examples.lqr_hold import start_state  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=4)
    ap.add_argument("--vmin", type=float, default=30.0)
    ap.add_argument("--vmax", type=float, default=50.0)
    ap.add_argument("--draws", type=int, default=256, help="noise draws per flight")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--kappa", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from aircraft_amd import SensorModel

    ac = make(args.model)
    trim = ac.trim(np.linspace(args.vmin, args.vmax, args.speeds))
    ok = trim.converged
    if not ok.any():
        raise SystemExit("no instance trimmed")
    xb, ub = np.repeat(trim.x[:, ok], args.draws, axis=1), np.repeat(trim.u[:, ok], args.draws, axis=1)
    n, T, dt = xb.shape[1], args.steps, args.dt
    res = ac.lqr((xb, ub), dt, q=[0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    xi0 = np.zeros((12, n))
    xi0[1], xi0[2], xi0[3], xi0[6] = 2.0, 2.0, -1.0, np.deg2rad(3.0)
    x0 = start_state(xi0, xb)
    rng = np.random.default_rng(args.seed)
    xh0 = boxplus(x0, SIG_P0[:, None] * rng.standard_normal((12, n)))
    P0 = np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2)
    sensors = SensorModel(sigma=SIG_R, period=(10, 10, 1, 1, 1), seed=args.seed)
    kw = dict(q=SIG_Q ** 2, r=SIG_R ** 2)
    banks = {"EKF": ac.ekf(xh0, P0, **kw), "UKF": ac.ukf(xh0, P0, kappa=args.kappa, **kw)}
    runs = {k: ac.rollout_lqg(res, b, x0, T, sensors, process_sigma=SIG_Q) for k, b in banks.items()}
    runs["true state"] = ac.rollout_lqg(res, ac.ekf(xh0, P0, **kw), x0, T, sensors, process_sigma=SIG_Q, feedback="truth")
    print(f"model={args.model}  {int(ok.sum())} flights x {args.draws} draws = {n} loops, {T} steps of {dt} s")
    print(f"  {'t [s]':>6s}  " + "  ".join(f"{k:>30s}" for k in runs) + "      (RMS cross-track, down [m] | airspeed rows [m/s])")
    for k in sorted({0, 9, T // 4 - 1, T // 2 - 1, T - 1}):
        cols = []
        for r in runs.values():
            xi = ac.steady_error(r.X[k + 1], r.Xnom[k + 1])
            cols.append(f"{np.sqrt((xi[1:3] ** 2).mean()):14.4f} | {np.sqrt((xi[3:6] ** 2).mean()):13.4f}")
        print(f"  {(k + 1) * dt:6.2f}  " + "  ".join(cols))
    for name in ("EKF", "UKF"):
        r = runs[name]
        good = (r.status == 0).all(axis=0) & np.isfinite(r.nees).all(axis=0)
        rows = np.array([bin(int(v)).count("1") for v in r.used.ravel()]).reshape(r.used.shape)
        print(f"{name}: {int((~good).sum())} loops reported a status; mean NIS per used row "
              f"{r.nis[:, good].sum() / rows[:, good].sum():.3f}, mean NEES / 12 {r.nees[:, good].mean() / 12:.3f} "
              f"(first step {r.nees[0, good].mean() / 12:.3f})")


if __name__ == "__main__":
    main()
