#!/usr/bin/env python3
"""The scenario of examples/ekf_track.py run with both filter banks: the flights, sensors, noise draws and starting estimates
are the same, Aircraft.ekf linearises once per step, Aircraft.ukf carries 25 sigma points through the step and the sensors.
Prints the RMS estimation error and the mean normalised innovation squared per used row of both, side by side (1 for a
consistent filter; the first step, with the full initial spread, is where the two differ).

    python examples/ukf_track.py --model poly --speeds 4 --draws 256
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.ekf_track import ALL, BLOCKS, GPS, SIG_P0, SIG_Q, SIG_R, boxminus, boxplus  # noqa: E402
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
    ac = make(args.model)
    trim = ac.trim(np.linspace(args.vmin, args.vmax, args.speeds))
    ok = trim.converged
    if not ok.any():
        raise SystemExit("no instance trimmed")
    xb, ub = trim.x[:, ok], trim.u[:, ok]
    m, T, dt = xb.shape[1], args.steps, args.dt
    res = ac.lqr((xb, ub), dt, q=[0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    xi0 = np.zeros((12, m))
    xi0[1], xi0[2], xi0[3], xi0[6] = 2.0, 2.0, -1.0, np.deg2rad(3.0)
    X, U, _ = ac.rollout_lqr(res, start_state(xi0, xb), T)
    n = m * args.draws
    rng = np.random.default_rng(args.seed)
    Xn, Un = np.repeat(X, args.draws, axis=2), np.repeat(U, args.draws, axis=2)
    Z = np.stack([ac.measure(Xn[k + 1]) for k in range(T)]) + SIG_R[None, :, None] * rng.standard_normal((T, 15, n))
    mask = np.full((T, n), ALL & ~GPS, dtype=np.int32)
    mask[9::10] = ALL
    P0 = np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2)
    x0 = boxplus(Xn[0], SIG_P0[:, None] * rng.standard_normal((12, n)))
    banks = {"EKF": ac.ekf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2), "UKF": ac.ukf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2, kappa=args.kappa)}
    tr = {k: b.filter(Un, dt, Z, mask) for k, b in banks.items()}
    bad = np.any([(t.status != 0).any(axis=0) for t in tr.values()], axis=0)
    print(f"model={args.model}  {m} flights x {args.draws} draws = {n} filters, {T} steps of {dt} s; "
          f"{int(bad.sum())} filters reported a status")
    print(f"  {'t [s]':>6s}  " + "  ".join(f"{name:>22s}" for name, _ in BLOCKS) + "      (RMS error EKF | UKF)")
    for k in sorted({0, 9, T // 4 - 1, T // 2 - 1, T - 1}):
        d = {name: boxminus(Xn[k + 1], t.X[k])[:, ~bad] for name, t in tr.items()}
        cols = [f"{np.sqrt((d['EKF'][sl] ** 2).mean()):10.4f} | {np.sqrt((d['UKF'][sl] ** 2).mean()):9.4f}" for _, sl in BLOCKS]
        print(f"  {(k + 1) * dt:6.2f}  " + "  ".join(cols))
    for name, t in tr.items():
        rows = np.array([bin(int(v)).count("1") for v in t.used.ravel()]).reshape(t.used.shape)
        print(f"{name}: mean NIS per used row {t.nis[:, ~bad].sum() / rows[:, ~bad].sum():.3f} over {int(rows[:, ~bad].sum())} rows "
              f"(first step {t.nis[0, ~bad].sum() / rows[0, ~bad].sum():.3f}); mean log-likelihood per filter {t.ll[~bad].mean():.1f}")


if __name__ == "__main__":
    main()
