#!/usr/bin/env python3
"""Track a glider with a bank of extended Kalman filters: trim a range of airspeeds, hold each trim with the LQR
(Aircraft.rollout_lqr) from a disturbed start, read the sensors along every flight (Aircraft.measure plus seeded noise: GPS
every 10th step, gyro, air data and magnetometer every step), and filter `--draws` noise draws of every flight in one batch
(Aircraft.ekf(...).filter).  Prints the RMS estimation error beside the filter's own posterior sigma, and the mean
normalised innovation squared per used row (1 for a consistent filter; these flights carry no process noise, so a filter that
allows for Qd is conservative and prints less).

    python examples/ekf_track.py --model poly --speeds 4 --draws 256
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.glide_polar import make  # noqa: E402
from examples.lqr_hold import start_state  # noqa: E402

SIG_P0 = np.array([2, 2, 2, 0.5, 0.5, 0.5, 0.03, 0.03, 0.05, 0.05, 0.05, 0.05])        # m, m/s, rad, rad/s
SIG_Q = np.array([0.01] * 3 + [0.05] * 3 + [0.002] * 3 + [0.02] * 3)                  # per step
SIG_R = np.array([1.5, 1.5, 3, 0.2, 0.2, 0.3, 0.01, 0.01, 0.01, 0.5, 0.01, 0.01, 0.02, 0.02, 0.02])
GPS, ALL = 0x3F, 0x7FFF
BLOCKS = (("position [m]", slice(0, 3)), ("velocity [m/s]", slice(3, 6)), ("attitude [rad]", slice(6, 9)), ("rates [rad/s]", slice(9, 12)))


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.stack([aw * bx + bw * ax + ay * bz - az * by, aw * by + bw * ay + az * bx - ax * bz,
                     aw * bz + bw * az + ax * by - ay * bx, aw * bw - (ax * bx + ay * by + az * bz)])


def boxplus(x, d):
    """x [+] d: the filter's error coordinates (dp, dv, body-frame rotation vector, dw) applied to a state"""
    q = qmul(x[6:10], np.concatenate([0.5 * d[6:9], np.ones((1, d.shape[1]))]))
    return np.concatenate([x[0:3] + d[0:3], x[3:6] + d[3:6], q / np.sqrt((q * q).sum(0)), x[10:13] + d[9:12]])


def boxminus(x, xb):
    """the d with xb [+] d = x"""
    e = qmul(np.stack([-xb[6], -xb[7], -xb[8], xb[9]]), x[6:10])
    return np.concatenate([x[0:3] - xb[0:3], x[3:6] - xb[3:6], 2 * e[:3] / e[3], x[10:13] - xb[10:13]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=4)
    ap.add_argument("--vmin", type=float, default=30.0)
    ap.add_argument("--vmax", type=float, default=50.0)
    ap.add_argument("--draws", type=int, default=256, help="noise draws per flight")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    ac = make(args.model)
    trim = ac.trim(np.linspace(args.vmin, args.vmax, args.speeds))
    ok = trim.converged
    if not ok.any():
        raise SystemExit("no instance trimmed")
    xb, ub = trim.x[:, ok], trim.u[:, ok]
    m, T, dt = xb.shape[1], args.steps, args.dt
    # the flights: each trim held by the LQR from 2 m off the path, 1 m/s slow, 3 degrees of bank
    res = ac.lqr((xb, ub), dt, q=[0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1])
    xi0 = np.zeros((12, m))
    xi0[1], xi0[2], xi0[3], xi0[6] = 2.0, 2.0, -1.0, np.deg2rad(3.0)
    X, U, _ = ac.rollout_lqr(res, start_state(xi0, xb), T)
    # the sensors: n = m * draws filters, `draws` noise draws of every flight
    n = m * args.draws
    rng = np.random.default_rng(args.seed)
    Xn, Un = np.repeat(X, args.draws, axis=2), np.repeat(U, args.draws, axis=2)
    Z = np.stack([ac.measure(Xn[k + 1]) for k in range(T)]) + SIG_R[None, :, None] * rng.standard_normal((T, 15, n))
    mask = np.full((T, n), ALL & ~GPS, dtype=np.int32)
    mask[9::10] = ALL
    # the filters start from a draw of N(truth, P0)
    P0 = np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2)
    x0 = boxplus(Xn[0], SIG_P0[:, None] * rng.standard_normal((12, n)))
    filt = ac.ekf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2)
    tr = filt.filter(Un, dt, Z, mask)
    bad = (tr.status != 0).any(axis=0)
    print(f"model={args.model}  {m} flights x {args.draws} draws = {n} filters, {T} steps of {dt} s; "
          f"{int(bad.sum())} filters reported a status")
    print(f"  {'t [s]':>6s}  " + "  ".join(f"{name:>24s}" for name, _ in BLOCKS) + "      (RMS error | posterior sigma)")
    for k in sorted({0, 9, T // 4 - 1, T // 2 - 1, T - 1}):
        d = boxminus(Xn[k + 1], tr.X[k])[:, ~bad]
        sig = np.sqrt(np.diagonal(tr.P[k]).T[:, ~bad])  # (12, n)
        cols = [f"{np.sqrt((d[sl] ** 2).mean()):11.4f} | {np.sqrt((sig[sl] ** 2).mean()):10.4f}" for _, sl in BLOCKS]
        print(f"  {(k + 1) * dt:6.2f}  " + "  ".join(cols))
    rows = np.array([bin(int(v)).count("1") for v in tr.used.ravel()]).reshape(tr.used.shape)
    print(f"mean NIS per used row: {tr.nis[:, ~bad].sum() / rows[:, ~bad].sum():.3f} over {int(rows[:, ~bad].sum())} rows "
          f"(first step {tr.nis[0, ~bad].sum() / rows[0, ~bad].sum():.3f}); mean log-likelihood per filter {tr.ll[~bad].mean():.1f}")


if __name__ == "__main__":
    main()
