#!/usr/bin/env python3
"""Glide polar of a coefficient model: trim a sweep of airspeeds (straight, wings level, beta = 0) in one batched call,
print alpha, theta, flight-path angle, elevator, sink rate and L/D per speed, pick the best-glide speed, and list the
eigenvalues of the step Jacobian A (dt = 0.01) at each trim that are not 1 (the position integrators), as the reference's
stability analysis does (main/stability/stability.py:74-81).

    python examples/glide_polar.py --model poly --speeds 12
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData  # noqa: E402
from aircraft_amd.synthetic import GLIDER  # noqa: E402


def make(model):
    cfg = AircraftConfiguration(dict(GLIDER))
    golden = os.path.join(ROOT, "tests", "golden")
    if model == "nn":
        w = np.load(os.path.join(golden, "scaledmodel_weights.npz"))
        path = MlpData([w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0], w["input_mean"], w["input_std"],
                       w["output_mean"], w["output_std"])
    elif model == "poly":
        path = os.path.join(golden, "poly_coef.npz")
    elif model == "linear":
        path = os.path.join(golden, "linearised.npz")
    else:
        path = ""
    return Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=path, aircraft_config=cfg,
                                 physical_integration_substeps=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="poly", choices=["default", "linear", "poly", "nn"])
    ap.add_argument("--speeds", type=int, default=12)
    ap.add_argument("--vmin", type=float, default=25.0)
    ap.add_argument("--vmax", type=float, default=70.0)
    args = ap.parse_args()
    ac = make(args.model)
    V = np.linspace(args.vmin, args.vmax, args.speeds)
    res = ac.trim(V)  # one batched call: every speed is one instance
    print(f"model={args.model}  {int(res.converged.sum())}/{len(V)} trimmed")
    print("  V [m/s]  alpha [deg]  theta [deg]  gamma [deg]  elevator [deg]  sink [m/s]    L/D  status")
    best = None
    for i, v in enumerate(V):
        al, th = np.rad2deg(res.z[0, i]), np.rad2deg(res.z[1, i])
        vn = res.x[3:6, i]
        sink = vn[2]  # NED: positive down
        gamma = -np.rad2deg(np.arctan2(sink, np.hypot(vn[0], vn[1])))
        ld = np.hypot(vn[0], vn[1]) / sink if sink > 0 else np.inf
        print(f"  {v:7.2f}  {al:11.3f}  {th:11.3f}  {gamma:11.3f}  {res.z[4, i]:14.3f}  {sink:10.3f}  {ld:5.2f}  {res.status[i]}")
        if res.converged[i] and np.isfinite(ld) and (best is None or ld > best[1]):
            best = (v, ld, sink)
    if best is None:
        print("best glide: none of the speeds trimmed")
        return 1
    print(f"best glide: V = {best[0]:.2f} m/s, L/D = {best[1]:.2f}, sink = {best[2]:.3f} m/s")
    ok = np.where(res.converged)[0]
    _, A, _, _ = ac.step_sens(res.x[:, ok], res.u[:, ok], 0.01)
    for k, i in enumerate(ok):
        ev = np.linalg.eigvals(A[:, :, k])  # host numpy: example code, not the product
        ev = ev[np.abs(ev - 1.0) > 1e-6]
        ev = ev[np.argsort(-np.abs(ev))]
        print(f"  V = {V[i]:6.2f}: |lambda|max = {np.abs(ev).max():.6f}; " + " ".join(f"{e.real:+.5f}{e.imag:+.5f}j" for e in ev))
    return 0


if __name__ == "__main__":
    sys.exit(main())
