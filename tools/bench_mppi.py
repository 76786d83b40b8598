#!/usr/bin/env python3
"""Times the parts of one MPPI iteration separately — sample, candidate rollout, candidate cost, update — and the same sample
and update arithmetic written in torch on the same buffers (randn, clamp, softmax, a weighted sum).

    python tools/bench_mppi.py                       # B=64 x K=1024 x H=50 and B=4096 x K=16 x H=50; cubic fits and the 4x128 net
    python tools/bench_mppi.py --sizes 64x1024x50 --models poly

Every part is warmed up on its real shapes, then timed with device events around a window of repeated launches that is at
least --window seconds long; HIP and torch variants alternate over --rounds rounds and the median round is reported, with the
spread.  Algorithmic bytes: the sampler writes 28 H K B (+ 52 K B for the tiled initial state), the update reads the same
28 H K B plus J and writes the weights once and reads them seven times per node from cache.  One JSON line per size and model.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(torch, fn, window):
    """Milliseconds per call of fn: warm-up, a probe to size the window, then one window between two device events."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        fn()
    b.record()
    torch.cuda.synchronize()
    per = max(a.elapsed_time(b) / 5, 1e-3)
    reps = int(min(max(window * 1e3 / per, 10), 20000))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="64x1024x50,4096x16x50", help="BxKxH, comma separated")
    ap.add_argument("--models", type=str, default="poly,nn")
    ap.add_argument("--hidden", type=str, default="128,128,128,128")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=0.05)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi.py needs the GPU: there is nothing to time without it")
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
    from aircraft_amd.control import ILQR, MPPI, QuadraticCost
    from aircraft_amd.synthetic import GLIDER, TRIM_STATE

    dev = torch.device("cuda", 0)
    for model in args.models.split(","):
        if model == "nn":
            path = MlpData.synthetic(tuple(int(h) for h in args.hidden.split(",")), seed=42)
        else:
            path = os.path.join(ROOT, "tests", "golden", "poly_coef.npz") if model == "poly" else ""
        ac = Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=path,
                                   aircraft_config=AircraftConfiguration(dict(GLIDER)), physical_integration_substeps=1))
        for size in args.sizes.split(","):
            B, K, H = (int(v) for v in size.split("x"))
            cost = QuadraticCost.goal((50.0 * H * 0.01, 2.0), w_goal=1.0, height=-200.0, w_height=1.0, w_lateral_speed=0.5, r=1e-2, reg=1.0)
            prob = ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost)
            sigma = (0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0)
            m = MPPI(prob, samples=K, sigma=sigma, temperature=args.temperature, seed=1, accept=False)
            x0 = torch.from_numpy(np.repeat(TRIM_STATE[:, None], B, axis=1).astype(np.float32)).to(dev)
            U = torch.zeros((H, 7, B), device=dev)
            X = prob.rollout(x0, U)
            ws = m._workspace(B, dev)
            m.iterate(x0, X.clone(), U.clone())  # fills every buffer once
            Uc, X0c, Xc, Jc, Un, stats = ws["Uc"], ws["X0c"], ws["Xc"], ws["Jc"], ws["Un"], ws["stats"]
            sg = torch.tensor(sigma, device=dev)[None, :, None, None]
            lo = torch.tensor(cost.u_min, device=dev)[None, :, None, None]
            hi = torch.tensor(cost.u_max, device=dev)[None, :, None, None]
            Uc4 = Uc.view(H, 7, K, B)
            noise = torch.empty((H, 7, K, B), device=dev)
            wt = torch.empty((K, B), device=dev)

            def torch_sample():
                torch.randn((H, 7, K, B), out=noise)
                torch.addcmul(U[:, :, None, :], noise, sg, out=Uc4)
                torch.maximum(Uc4, lo, out=Uc4)
                torch.minimum(Uc4, hi, out=Uc4)
                X0c.view(13, K, B).copy_(x0[:, None, :])

            def torch_update():
                torch.softmax(Jc.view(K, B) * (-1.0 / args.temperature), dim=0, out=wt)
                Un.copy_(torch.einsum("hrkb,kb->hrb", Uc4, wt))
                torch.maximum(Un, lo[:, :, 0], out=Un)
                torch.minimum(Un, hi[:, :, 0], out=Un)

            parts = {
                "sample_hip": lambda: m.sample(U, x0, out=(Uc, X0c)),
                "sample_torch": torch_sample,
                "update_hip": lambda: m.update(Jc, Uc, U, out=(Un, stats)),
                "update_torch": torch_update,
                "candidate_rollout": lambda: prob.rollout(X0c, Uc, out=Xc),
                "candidate_cost": lambda: prob.trajectory_cost(Xc, Uc, out=Jc),
                "nominal_rollout_and_cost": lambda: (prob.rollout(x0, Un, out=ws["Xn"]), prob.trajectory_cost(ws["Xn"], Un, out=ws["Jn"])),
                "iteration": lambda: m.iterate(x0, X, U),
            }
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    if k == "update_hip" or k == "update_torch":
                        m.sample(U, x0, out=(Uc, X0c)); prob.rollout(X0c, Uc, out=Xc); prob.trajectory_cost(Xc, Uc, out=Jc)
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            sample_bytes = 28.0 * H * K * B + 52.0 * K * B
            update_bytes = 28.0 * H * K * B + 4.0 * K * B * 2 + 28.0 * H * B * 2
            it_ms = ms["iteration"]
            print(json.dumps({
                "model": model, "B": B, "K": K, "H": H, "ms": ms, "spread_over_rounds": spread,
                "sample_algorithmic_bytes": sample_bytes, "update_algorithmic_bytes": update_bytes,
                "sample_hip_TBps": sample_bytes / (ms["sample_hip"] * 1e-3) / 1e12,
                "update_hip_TBps": update_bytes / (ms["update_hip"] * 1e-3) / 1e12,
                "sample_torch_over_hip": ms["sample_torch"] / ms["sample_hip"],
                "update_torch_over_hip": ms["update_torch"] / ms["update_hip"],
                "share_of_iteration": {"sample": ms["sample_hip"] / it_ms, "update": ms["update_hip"] / it_ms,
                                       "candidate_rollout": ms["candidate_rollout"] / it_ms, "candidate_cost": ms["candidate_cost"] / it_ms},
                "rollouts_per_s": K * B / (it_ms * 1e-3)}), flush=True)
            del m, ws, noise, wt, Uc4
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
