#!/usr/bin/env python3
"""Stability studies of the discrete step, each as ONE batched call of Aircraft.modes (the reference's main/stability study
evaluates the step Jacobian and numpy eigvals point by point):

  1. the eigenvalues of the step at a cloud of perturbed states about a trim, against the unit circle;
  2. max |lambda| against dt (logspace 1e-4 .. 1; one call per dt over the whole batch of trims);
  3. the 20 x 20 aileron / elevator map of max |lambda| at a trim state;
  4. per trim of an airspeed sweep, the flight modes as (omega_n, zeta, time to half or double amplitude), open loop and with
     the LQR of Aircraft.lqr, side by side.

    python examples/stability_map.py --model poly
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.glide_polar import make  # noqa: E402


def describe(s):
    """one mode s = sigma + i omega -> text: omega_n [rad/s], zeta, time to half (-) or double (+) amplitude [s]"""
    wn = abs(s)
    if wn == 0 or not np.isfinite(wn):
        return "      (s = 0)      " if wn == 0 else "       (nan)       "
    t = np.log(2.0) / abs(s.real) if s.real != 0 else np.inf
    return f"{wn:7.3f} {-s.real / wn:+6.3f} {'T2' if s.real > 0 else 'T½'}={min(t, 9999.0):7.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--speed", type=float, default=35.0)
    args = ap.parse_args()
    ac = make(args.model)
    dt = args.dt
    trim = ac.trim(np.array([args.speed]))
    if not trim.converged.all():
        print("the nominal speed does not trim")
        return 1
    x0, u0 = trim.x[:, 0], trim.u[:, 0]

    # 1. a cloud of perturbed states: body velocity, attitude and rates disturbed about the trim
    rng = np.random.default_rng(0)
    n = 512
    x = np.repeat(x0[:, None], n, axis=1)
    x[3:6] += rng.normal(0, 2.0, (3, n))
    x[6:10] += rng.normal(0, 0.05, (4, n))
    x[6:10] /= np.linalg.norm(x[6:10], axis=0)
    x[10:13] += rng.normal(0, 0.2, (3, n))
    cloud = ac.modes((x, np.repeat(u0[:, None], n, axis=1)), dt)
    print(f"1. cloud of {n} perturbed states, dt = {dt}: {int((cloud.unstable > 0).sum())} have an eigenvalue outside the unit circle; "
          f"max |lambda| {cloud.rho.min():.6f} .. {cloud.rho.max():.6f}; QR iterations per eigenvalue {cloud.iterations.mean() / 8:.2f}")
    print("   Re lambda %.4f .. %.4f, |Im lambda| <= %.4f" % (cloud.lam.real.min(), cloud.lam.real.max(), np.abs(cloud.lam.imag).max()))

    # 2. max |lambda| against dt over a batch of trims
    V = np.linspace(25.0, 70.0, 64)
    sweep = ac.trim(V)
    ok = sweep.converged
    print(f"2. max |lambda| against dt over {int(ok.sum())} trims, {V[0]:.0f} .. {V[-1]:.0f} m/s (the explicit step leaves the unit circle where dt grows)")
    print("        dt   min rho   max rho  stable trims")
    for d in np.logspace(-4, 0, 17):
        r = ac.modes((sweep.x[:, ok], sweep.u[:, ok]), float(d))
        rho = np.where(r.converged, r.rho, np.inf)
        print(f"   {d:8.2e}  {rho.min():8.5f}  {min(rho.max(), 9.9e9):8.3g}  {int((rho <= 1 + 1e-6).sum()):4d}")

    # 3. the aileron / elevator map at the trim state
    g = 20
    ail, ele = np.meshgrid(np.linspace(-10, 10, g), np.linspace(-10, 10, g), indexing="ij")
    u = np.repeat(u0[:, None], g * g, axis=1)
    u[0], u[1] = u0[0] + ail.ravel(), u0[1] + ele.ravel()
    m = ac.modes((np.repeat(x0[:, None], g * g, axis=1), u), dt)
    rho = m.rho.reshape(g, g)
    print(f"3. {g} x {g} aileron / elevator map (deflections +-10 deg about the trim) of (max |lambda| - 1) x 1e4; rows: aileron, columns: elevator")
    for i in range(0, g, 2):
        print("   " + " ".join(f"{(rho[i, j] - 1) * 1e4:6.1f}" for j in range(0, g, 2)))

    # 4. the modes per trim, open loop and with the LQR
    V4 = np.linspace(25.0, 60.0, 8)
    t4 = ac.trim(V4)
    design = ac.lqr(t4, dt)
    op, cl = ac.modes(t4, dt), ac.modes(t4, dt, gains=design)
    print("4. flight modes per trim: omega_n [rad/s], zeta, time to half (T½) or double (T2) amplitude [s]; one line per mode with Im s >= 0")
    for i, v in enumerate(V4):
        if not (t4.converged[i] and op.converged[i] and cl.converged[i]):
            print(f"   V = {v:5.1f}: not trimmed or not converged")
            continue
        print(f"   V = {v:5.1f} m/s: rho open {op.rho[i]:.6f} ({int(op.unstable[i])} unstable), closed {cl.rho[i]:.6f}")
        so, sc = (sorted(r.s[:, i][r.s[:, i].imag >= 0], key=abs) for r in (op, cl))
        for k in range(max(len(so), len(sc))):
            a = describe(so[k]) if k < len(so) else " " * 26
            b = describe(sc[k]) if k < len(sc) else ""
            print(f"      open  {a}    |  closed  {b}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
