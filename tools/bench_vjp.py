#!/usr/bin/env python3
"""Time of one rollout GRADIENT at B = 4096, H = 50, per model, by three routes:
  fused     ac_rollout_vjp_f32 on the fused kernel (k_rollout_vjp; analytic models only)
  composed  ac_rollout_vjp_f32 on the composed route (ac_shoot_sens_f32 into the workspace + k_vjp_recur)
  bmm       what a caller could do before: ac_shoot_sens_f32 (A, B, c of every node) + the reverse recurrence in torch
            (one bmm per node and matrix)
Each figure: warm-up, then >= 20 repeats timed one by one with HIP events; median, min and max in ms.  One JSON line on
stdout (and --out FILE).  `--profile` runs every route a few times only (for a rocprofv3 --kernel-trace --stats run)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData  # noqa: E402
from aircraft_amd.synthetic import GLIDER, near_trim_problem  # noqa: E402


def make(model):
    cfg = AircraftConfiguration(dict(GLIDER))
    if model == "real_net":
        w = np.load(os.path.join(ROOT, "tests", "golden", "scaledmodel_weights.npz"))
        path = MlpData([w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0], w["input_mean"], w["input_std"],
                       w["output_mean"], w["output_std"])
        kind = "nn"
    elif model == "net_4x128":
        path, kind = MlpData.synthetic((128, 128, 128, 128), seed=42), "nn"
    elif model == "poly":
        path, kind = os.path.join(ROOT, "tests", "golden", "poly_coef.npz"), "poly"
    else:
        path, kind = "", "default"
    ac = Aircraft(AircraftOpts(coeff_model_type=kind, coeff_model_path=path, aircraft_config=cfg, physical_integration_substeps=1))
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
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="poly,default,real_net,net_4x128")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.profile:
        args.reps, args.warmup = 3, 1
    dev = torch.device("cuda", 0)
    B, H = args.batch, args.horizon
    X0, U = near_trim_problem(B, H, seed=0)
    X0 = torch.from_numpy(np.ascontiguousarray(X0, dtype=np.float32)).to(dev)
    U = torch.from_numpy(np.ascontiguousarray(U, dtype=np.float32)).to(dev)
    G = torch.randn(H + 1, 13, B, device=dev) * 1e-2
    res = {"B": B, "H": H, "device": torch.cuda.get_device_name(0), "models": {}}
    for model in args.models.split(","):
        ac = make(model)
        dt = 0.002 if model == "default" else 0.01  # (the default model's fit leaves RK4's stability region at 0.01 near trim)
        Xtraj = ac.rollout(X0, U, dt)
        out = {}
        routes = (["fused"] if model in ("poly", "default") else []) + ["composed"]
        for route in routes:
            ac.vjp_route = route
            ws = ac.vjp_workspace("rollout", B, H)
            out[route] = timed(lambda: ac.rollout_vjp(Xtraj, U, dt, G, ws=ws), args.warmup, args.reps)
            out[route]["kernel"] = ac.last_launch()[0]
        # the route of a user without the reverse-mode entry points: dense A, B, c of every node, recurrence in torch
        Xn = torch.empty(H, 13, B, device=dev)
        A = torch.empty(H, 13, 13, B, device=dev)
        Bm = torch.empty(H, 13, 7, B, device=dev)
        c = torch.empty(H, 13, B, device=dev)

        def bmm_route():
            from aircraft_amd import _lib
            import ctypes as C

            _lib.check(_lib.load().ac_shoot_sens_f32(ac._handle, Xtraj.data_ptr(), U.data_ptr(), C.c_float(dt), None, B, H,
                                                     Xn.data_ptr(), A.data_ptr(), Bm.data_ptr(), c.data_ptr(), ac._stream()))
            At = A.permute(0, 3, 2, 1)   # (H, B, 13 in, 13 out): A_k' per instance
            Bt = Bm.permute(0, 3, 2, 1)
            lam = G[H].t().unsqueeze(-1)  # (B, 13, 1)
            ub = torch.empty(H, B, 7, 1, device=dev)
            dtb = torch.zeros(B, device=dev)
            for k in range(H - 1, -1, -1):
                ub[k] = torch.bmm(Bt[k], lam)
                dtb += (c[k].t() * lam[..., 0]).sum(1)
                lam = G[k].t().unsqueeze(-1) + torch.bmm(At[k], lam)
            return lam, ub, dtb

        ac._sync()
        out["bmm"] = timed(bmm_route, args.warmup, args.reps)
        # the three agree (fp32 roundings apart)
        ref = ac.rollout_vjp(Xtraj, U, dt, G)[0]
        alt = bmm_route()[0][..., 0].t()
        out["bmm_vs_composed_max_rel"] = float((ref - alt).abs().max() / ref.abs().max())
        out["dt"] = dt
        out["finite_trajectory_frac"] = float(torch.isfinite(Xtraj).all(0).all(0).float().mean())
        res["models"][model] = out
        del Xn, A, Bm, c
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
