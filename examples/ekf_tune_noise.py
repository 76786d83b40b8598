#!/usr/bin/env python3
"""Tune the filter's noise variances from recorded flights: fly a noisy truth from a range of trims (x_{t+1} = F(x_t, u) [+]
N(0, Qd), constant trim controls), read the sensors along every flight (GPS every 10th step, the others every step), and start
a bank of extended Kalman filters from process and sensor variances that are WRONG by 16 x either way (sigma by 4 x).
EKF.fit_noise then runs EM over the logs: filter, smooth, re-estimate q and r, repeat (share=True: one airframe, many logs,
so the sums are pooled over the logs).  Prints the summed log-likelihood per iteration, the fitted sigma against the true
ones, and the RMS error of the smoothed states before and after.

    python examples/ekf_tune_noise.py --model poly --speeds 4 --draws 64 --iters 10
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
    ap.add_argument("--draws", type=int, default=64, help="noise draws per flight")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--per-log", action="store_true", help="fit every log on its own instead of pooling them")
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
    X = [np.repeat(trim.x[:, ok], args.draws, axis=1)]
    for _ in range(T):
        X.append(boxplus(ac.state_update(X[-1], u, dt), SIG_Q[:, None] * rng.standard_normal((12, n))))
    X = np.stack(X)
    Z = np.stack([ac.measure(X[k + 1]) for k in range(T)]) + SIG_R[None, :, None] * rng.standard_normal((T, 15, n))
    mask = np.full((T, n), ALL & ~GPS, dtype=np.int32)
    mask[9::10] = ALL
    U = np.repeat(u[None], T, axis=0)
    P0 = np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2)
    x0 = boxplus(X[0], SIG_P0[:, None] * rng.standard_normal((12, n)))
    # the wrong start: every other variance 16 x too large, the others 16 x too small
    q0 = SIG_Q ** 2 * np.where(np.arange(12) % 2 == 0, 16.0, 1 / 16.0)
    r0 = SIG_R ** 2 * np.where(np.arange(15) % 2 == 0, 1 / 16.0, 16.0)

    def smoothed_rms(q, r):
        bank = ac.ekf(x0, P0, q=q, r=r)
        sm = bank.smooth(bank.filter(U, dt, Z, mask, record=True), initial=False)
        e = np.stack([boxminus(X[k + 1], sm.X[k]) for k in range(T)])
        return [float(np.sqrt((e[:, sl] ** 2).mean())) for _, sl in BLOCKS]

    bank = ac.ekf(x0, P0, q=q0, r=r0)
    fit = bank.fit_noise(U, dt, Z, mask, iters=args.iters, share=not args.per_log)
    print(f"model={args.model}  {m} flights x {args.draws} draws = {n} logs, {T} steps of {dt} s; "
          f"{'per log' if args.per_log else 'pooled over the logs'}; {int((fit.status != 0).any(axis=0).sum())} logs reported a status")
    for it, ll in enumerate(fit.ll.sum(axis=1)):
        print(f"  iteration {it:2d}: summed log-likelihood {ll:14.1f}")
    sq, sr = np.sqrt(np.median(fit.q, axis=1)), np.sqrt(np.median(fit.r, axis=1))
    print("  sigma_q  start / true: " + " ".join(f"{v:5.2f}" for v in np.sqrt(q0) / SIG_Q))
    print("  sigma_q fitted / true: " + " ".join(f"{v:5.2f}" for v in sq / SIG_Q))
    print("  sigma_r  start / true: " + " ".join(f"{v:5.2f}" for v in np.sqrt(r0) / SIG_R))
    print("  sigma_r fitted / true: " + " ".join(f"{v:5.2f}" for v in sr / SIG_R))
    print(f"  {'RMS error, smoothed':>26s}  " + "  ".join(f"{name:>16s}" for name, _ in BLOCKS))
    for label, (q, r) in (("wrong start", (q0, r0)), ("fitted", (fit.q, fit.r)), ("true variances", (SIG_Q ** 2, SIG_R ** 2))):
        print(f"  {label:>26s}  " + "  ".join(f"{v:16.4f}" for v in smoothed_rms(q, r)))


if __name__ == "__main__":
    main()
