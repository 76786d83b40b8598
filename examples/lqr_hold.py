#!/usr/bin/env python3
"""Path-holding LQR about a sweep of trims: trim a range of airspeeds (straight or turning) in one batched call, design a
constant-gain LQR about each trim in the steady-flight error coordinates (Aircraft.lqr), disturb the start, fly the closed
loop (Aircraft.rollout_lqr) and print how the error xi decays.

    python examples/lqr_hold.py --model poly --speeds 8 --turn-rate 0.1
    python examples/lqr_hold.py --model default --hold attitude --vmax 50
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from examples.glide_polar import make  # noqa: E402

XI_NAMES = ("along", "cross", "down", "vx", "vy", "vz", "tilt_x", "tilt_y", "heading", "p", "q", "r")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=8)
    ap.add_argument("--vmin", type=float, default=30.0)
    ap.add_argument("--vmax", type=float, default=60.0)
    ap.add_argument("--turn-rate", type=float, default=0.0, help="rad/s about NED down")
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--scale", type=float, default=1.0, help="size of the disturbance (1: 2 m, 1 m/s, 3 degrees)")
    ap.add_argument("--hold", default="path", choices=["path", "attitude"],
                    help="path: cross-track, height and heading are held too; attitude: the eight-state stability augmentation")
    args = ap.parse_args()
    ac = make(args.model)
    V = np.linspace(args.vmin, args.vmax, args.speeds)
    kw = dict(rudder=0.0) if args.model == "linear" and args.turn_rate else {}
    trim = ac.trim(V, turn_rate=args.turn_rate, **kw)
    ok = trim.converged
    print(f"model={args.model}  {int(ok.sum())}/{len(V)} trimmed")
    if not ok.any():
        raise SystemExit("no instance trimmed")
    x, u = trim.x[:, ok], trim.u[:, ok]
    q = None if args.hold == "attitude" else [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    res = ac.lqr((x, u), args.dt, q=q)
    print(f"LQR: status {res.status.tolist()}, doubling steps {res.iterations.tolist()}, worst residual {res.residual.max():.1e}")
    n = x.shape[1]
    # the start: 2 m off the path sideways and below, 1 m/s slow, 3 degrees of bank and heading
    xi0 = np.zeros((12, n))
    xi0[1], xi0[2], xi0[3], xi0[6], xi0[8] = 2.0, 2.0, -1.0, np.deg2rad(3.0), np.deg2rad(3.0)
    xi0 *= args.scale
    x0 = start_state(xi0, x)
    X, U, Xnom = ac.rollout_lqr(res, x0, args.steps)
    fin = np.isfinite(X).all(axis=(0, 1))
    if not fin.all():
        print(f"{int((~fin).sum())} of {n} closed loops left the model's range (explicit step, dt = {args.dt}): "
              f"V = {V[ok][~fin].round(1).tolist()} m/s; the rest:")
    if not fin.any():
        raise SystemExit("no closed loop stayed finite")
    shown = [i for i in range(12) if res.q[i] > 0]
    print("  t [s]  " + "  ".join(f"{XI_NAMES[i]:>8s}" for i in shown) + "   (worst instance per coordinate)")
    for k in sorted({0, args.steps // 8, args.steps // 4, args.steps // 2, args.steps}):
        xi = ac.steady_error(X[k][:, fin], Xnom[k][:, fin])
        print(f"  {k * args.dt:5.2f}  " + "  ".join(f"{np.abs(xi[i]).max():8.4f}" for i in shown))
    first, last = ac.steady_error(X[0][:, fin], Xnom[0][:, fin]), ac.steady_error(X[-1][:, fin], Xnom[-1][:, fin])
    v0 = np.einsum("in,ijn,jn->n", first, res.P[:, :, fin], first)
    v1 = np.einsum("in,ijn,jn->n", last, res.P[:, :, fin], last)
    print(f"cost-to-go xi'P xi fell by a factor of {np.min(v0 / v1):.1f} .. {np.max(v0 / v1):.1f} over {args.steps * args.dt:.1f} s")
    dU = np.abs(U - u[None])[:, :, fin].max(axis=(0, 2))
    print(f"largest control excursion from trim: {dU[[0, 1, 2]].round(3).tolist()} deg (aileron, elevator, rudder)")


def start_state(xi, xb):
    """the state whose steady-flight error about xb is xi (small attitude errors): heading-frame offsets added to the trim"""
    qx, qy, qz, qw = xb[6:10] / np.linalg.norm(xb[6:10], axis=0)
    psi = np.arctan2(2 * (qw * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz))
    c, s = np.cos(psi), np.sin(psi)

    def to_ned(v):
        return np.stack([c * v[0] - s * v[1], s * v[0] + c * v[1], v[2]])

    def qmul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return np.stack([aw * bx + bw * ax + ay * bz - az * by, aw * by + bw * ay + az * bx - ax * bz,
                         aw * bz + bw * az + ax * by - ay * bx, aw * bw - (ax * bx + ay * by + az * bz)])

    def rotate(q, v):
        qc = np.stack([-q[0], -q[1], -q[2], q[3]])
        return qmul(qmul(q, np.concatenate([v, np.zeros((1, v.shape[1]))])), qc)[:3]

    qb = np.stack([qx, qy, qz, qw])
    qbc = np.stack([-qx, -qy, -qz, qw])
    half = 0.5 * to_ned(xi[6:9])
    d = np.concatenate([half, np.sqrt(1 - (half * half).sum(0))[None]])
    q = qmul(d, qb)
    v_body = rotate(qbc, xb[3:6]) + xi[3:6]
    return np.concatenate([xb[0:3] + to_ned(xi[0:3]), rotate(q, v_body), q, xb[10:13] + xi[9:12]])


if __name__ == "__main__":
    main()
