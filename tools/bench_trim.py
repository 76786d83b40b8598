#!/usr/bin/env python3
"""Time of one batched trim (Aircraft.trim -> ac_trim_f32, iters = 30) at n = 4096 and n = 65536 for the
cubic fits, the default model and the shipped 5-16-32-6 net: straight and turning flight at 25-70 m/s.  Each figure: warm-up,
then 25 repeats timed one by one with HIP events around the whole call (3 x iters launches); median, min and max in ms, and
the fraction of instances that converged.  One JSON line on stdout (and --out FILE).  `--profile` runs each case a few
times only, for a separate `rocprofv3 --kernel-trace --stats` run that splits the time into k_trim_assemble, the
derivative-sensitivity kernel and k_trim_update."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData  # noqa: E402
from aircraft_amd.synthetic import GLIDER  # noqa: E402


def make(model):
    cfg = AircraftConfiguration(dict(GLIDER))
    if model == "real_net":
        w = np.load(os.path.join(ROOT, "tests", "golden", "scaledmodel_weights.npz"))
        path = MlpData([w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0], w["input_mean"], w["input_std"],
                       w["output_mean"], w["output_std"])
        kind = "nn"
    elif model == "poly":
        path, kind = os.path.join(ROOT, "tests", "golden", "poly_coef.npz"), "poly"
    else:
        path, kind = "", "default"
    return Aircraft(AircraftOpts(coeff_model_type=kind, coeff_model_path=path, aircraft_config=cfg, physical_integration_substeps=1))


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
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--models", default="poly,default,real_net")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.profile:
        args.reps, args.warmup = 3, 1
    dev = torch.device("cuda", 0)
    res = {"iters": args.iters, "device": torch.cuda.get_device_name(0), "models": {}}
    for model in args.models.split(","):
        ac = make(model)
        out = {}
        for n in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(0)
            V = torch.tensor(rng.uniform(25, 70, n), dtype=torch.float32, device=dev)
            psid = torch.tensor(rng.choice([0.0, 0.15, -0.15], n), dtype=torch.float32, device=dev)
            psi = torch.tensor(rng.uniform(-np.pi, np.pi, n), dtype=torch.float32, device=dev)
            ws = ac.trim_workspace(n)
            r = timed(lambda: ac.trim(V, turn_rate=psid, psi=psi, iters=args.iters, ws=ws), args.warmup, args.reps)
            t = ac.trim(V, turn_rate=psid, psi=psi, iters=args.iters, ws=ws)
            r["converged_frac"] = float(t.converged.float().mean())
            r["status_counts"] = torch.bincount(t.status.long(), minlength=4).tolist()
            out[str(n)] = r
            del ws
            torch.cuda.empty_cache()
        res["models"][model] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
