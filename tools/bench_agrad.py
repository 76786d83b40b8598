#!/usr/bin/env python3
"""Time of the airframe gradients next to the plain VJP on the same inputs, poly and default:
  rollout   B = 4096 instances x H = 50 nodes:  ac_rollout_agrad_f32 (k_rollout_agrad + k_wgrad_reduce; x0, U, dt and the 22
            airframe gradients)  against  ac_rollout_vjp_f32 (k_rollout_vjp; x0, U, dt gradients)
  step      the 204 800 nodes of those trajectories as units:  ac_step_agrad_f32  against  ac_step_vjp_f32
The VJP kernels are the baseline, timed in the same run.  Each figure: 3 warm-ups, then 20 repeats timed one by one with HIP
events; median, min and max in ms.  One JSON line on stdout and in --out (default profiles/agrad_bench.json).  `--profile` runs
every call a few times only (for a rocprofv3 --kernel-trace --stats run).
Both models are timed on the nodes of the cubic-fit model's trajectories: the kernels' arithmetic does not depend on which model
produced the states."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts  # noqa: E402
from aircraft_amd.synthetic import GLIDER, near_trim_problem  # noqa: E402


def make(model, substeps=1):
    path = os.path.join(ROOT, "tests", "golden", "poly_coef.npz") if model == "poly" else ""
    ac = Aircraft(AircraftOpts(coeff_model_type=model, coeff_model_path=path, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=substeps))
    ac.normalise = True
    return ac


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="poly,default")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agrad_bench.json"))
    args = ap.parse_args()
    if args.profile:
        args.reps, args.warmup = 3, 1
    dev = torch.device("cuda", 0)
    B, H, dt = args.batch, args.horizon, 0.01
    X0, U = near_trim_problem(B, H, seed=0)
    X0 = torch.from_numpy(np.ascontiguousarray(X0, dtype=np.float32)).to(dev)
    U = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(dev)
    G = torch.randn(H + 1, 13, B, device=dev) * 1e-2
    Xtraj = make("poly").rollout(X0, U, dt).clone()
    n = B * H
    Xu = Xtraj[:H].permute(1, 0, 2).reshape(13, n).contiguous()
    Uu = U.permute(1, 0, 2).reshape(7, n).contiguous()
    Lu = G[1:].permute(1, 0, 2).reshape(13, n).contiguous()
    res = {"B": B, "H": H, "units": n, "dt": dt, "device": torch.cuda.get_device_name(0),
           "finite_trajectory_frac": float(torch.isfinite(Xtraj).all(0).all(0).float().mean()), "models": {}}
    for model in args.models.split(","):
        ac = make(model)
        ac.vjp_route = "fused"
        out = {}
        out["rollout_vjp"] = timed(lambda: ac.rollout_vjp(Xtraj, U, dt, G), args.warmup, args.reps)
        out["step_vjp"] = timed(lambda: ac.step_vjp(Xu, Uu, dt, Lu), args.warmup, args.reps)
        phi = torch.empty(22, device=dev)
        ws = ac.airframe_grad_workspace("rollout", B, H)
        out["rollout_agrad"] = timed(lambda: ac.rollout_airframe_grad(Xtraj, U, dt, G, ws=ws, out=phi), args.warmup, args.reps)
        out["rollout_agrad"].update(zip(("kernel", "grid", "block", "lds_bytes"), ac.last_launch()))
        ws = ac.airframe_grad_workspace("step", n)
        out["step_agrad"] = timed(lambda: ac.step_airframe_grad(Xu, Uu, dt, Lu, ws=ws, out=phi), args.warmup, args.reps)
        out["step_agrad"].update(zip(("kernel", "grid", "block", "lds_bytes"), ac.last_launch()))
        out["phi_bar_finite"] = bool(torch.isfinite(phi).all())
        for what in ("rollout", "step"):
            out[what + "_agrad_over_vjp"] = out[what + "_agrad"]["median_ms"] / out[what + "_vjp"]["median_ms"]
        res["models"][model] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
