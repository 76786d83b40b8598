#!/usr/bin/env python3
"""Smooth recorded flights: fly a noisy truth from a range of trims (x_{t+1} = F(x_t, u) [+] N(0, Qd), constant trim
controls), read the sensors along every flight (GPS every 10th step, gyro, air data and magnetometer every step), run the bank
of extended Kalman filters with the records kept (Aircraft.ekf(...).filter(..., record=True)) and the Rauch-Tung-Striebel
smoother over them in one backward sweep (EKF.smooth).  Prints the RMS estimation error per block (position, velocity,
attitude, rates), the filtered estimate (causal: the data up to each step) against the smoothed one (the whole log), which is
what a system-identification fit to recorded flights wants.  The smoother's gains (gains=True) give the lag-one covariances
P^s_k C_k' an EM estimate of Q and R would need; that loop is not part of this example.

    python examples/rts_smooth.py --model poly --speeds 4 --draws 256
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.ekf_track import ALL, BLOCKS, GPS, SIG_P0, SIG_Q, SIG_R, boxminus, boxplus  # noqa: E402
from examples.glide_polar import make  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=4)
    ap.add_argument("--vmin", type=float, default=30.0)
    ap.add_argument("--vmax", type=float, default=50.0)
    ap.add_argument("--draws", type=int, default=256, help="noise draws per flight")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    ac = make(args.model)
    trim = ac.trim(np.linspace(args.vmin, args.vmax, args.speeds))
    ok = trim.converged
    if not ok.any():
        raise SystemExit("no instance trimmed")
    m, T, dt = int(ok.sum()), args.steps, args.dt
    n = m * args.draws
    rng = np.random.default_rng(args.seed)
    u = np.repeat(trim.u[:, ok], args.draws, axis=1)
    # the noisy truth and its sensors
    X = [np.repeat(trim.x[:, ok], args.draws, axis=1)]
    for _ in range(T):
        X.append(boxplus(ac.state_update(X[-1], u, dt), SIG_Q[:, None] * rng.standard_normal((12, n))))
    X = np.stack(X)
    Z = np.stack([ac.measure(X[k + 1]) for k in range(T)]) + SIG_R[None, :, None] * rng.standard_normal((T, 15, n))
    mask = np.full((T, n), ALL & ~GPS, dtype=np.int32)
    mask[9::10] = ALL
    # the filters start from a draw of N(truth, P0)
    P0 = np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2)
    x0 = boxplus(X[0], SIG_P0[:, None] * rng.standard_normal((12, n)))
    filt = ac.ekf(x0, P0, q=SIG_Q ** 2, r=SIG_R ** 2)
    tr = filt.filter(np.repeat(u[None], T, axis=0), dt, Z, mask, record=True)
    sm = filt.smooth(tr)
    bad = (tr.status != 0).any(axis=0) | (sm.status != 0).any(axis=0)
    print(f"model={args.model}  {m} flights x {args.draws} draws = {n} filters, {T} steps of {dt} s; "
          f"{int(bad.sum())} instances reported a status")
    ef = np.stack([boxminus(X[k + 1], tr.X[k]) for k in range(T)])[:, :, ~bad]
    es = np.stack([boxminus(X[k + 1], sm.X[k]) for k in range(T)])[:, :, ~bad]
    e0f, e0s = boxminus(X[0], x0)[:, ~bad], boxminus(X[0], sm.X0)[:, ~bad]
    rms = lambda e, sl: np.sqrt((e[..., sl, :] ** 2).mean())  # noqa: E731
    print(f"  {'RMS error':>22s}  " + "  ".join(f"{name:>16s}" for name, _ in BLOCKS))
    for label, a in (("filtered, all steps", ef), ("smoothed, all steps", es), ("initial estimate", e0f), ("smoothed initial", e0s),
                     (f"filtered, step {T // 2}", ef[T // 2]), (f"smoothed, step {T // 2}", es[T // 2])):
        print(f"  {label:>22s}  " + "  ".join(f"{rms(a, sl):16.4f}" for _, sl in BLOCKS))
    k = T // 2
    ratio = np.trace(sm.P[k]) / np.trace(tr.P[k])
    print(f"trace P^s / trace P at step {k}: {ratio[~bad].mean():.3f}")


if __name__ == "__main__":
    main()
