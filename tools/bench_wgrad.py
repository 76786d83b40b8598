#!/usr/bin/env python3
"""Time of one rollout WEIGHT gradient of the MLP surrogate at B = 4096, H = 50, per net:
  rollout_wgrad  ac_rollout_wgrad_f32: sensitivities + reverse recurrence (the composed VJP route, lambda kept), the stage
                 table, the recording reverse sweep, k_mlp_wgrad, the reduction
  rollout_vjp    ac_rollout_vjp_f32 on the composed route in the same run: the lambda recurrence the call above reuses
  step_wgrad     ac_step_wgrad_f32 over the same B H units (no recurrence); seeds: ac_step_wgrad_seeds_f32 alone; their
                 difference is k_mlp_wgrad + reduction
  torch_f32      the same weight gradient by torch float32 autograd (forward + backward of the folded net) over the EXPORTED
                 seeds — what a caller could do without k_mlp_wgrad (the seeds' own time is not in it)
and the fp32-MFMA floor of the weight gradient: 6 P flop per sample (forward, backward-data, weights: 2 P each), P = sum of
n_i n_{i+1} over the folded net, four samples per unit, at the measured 155 TFLOP/s of v_mfma_f32_16x16x4_f32.
Each figure: warm-up, then repeats timed one by one with HIP events; median, min and max in ms.  One JSON line on stdout
(and --out FILE, default profiles/wgrad_bench.json).  `--profile` runs every route a few times only: for the kernel table run
    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/wgrad_trace -- python tools/bench_wgrad.py --profile --out ""
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from aircraft_amd import autodiff  # noqa: E402
from aircraft_amd.synthetic import near_trim_problem  # noqa: E402
from tools.bench_vjp import make, timed  # noqa: E402

MFMA_F32_TFLOPS = 155.0  # measured peak of v_mfma_f32_16x16x4_f32 on an MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default="real_net,net_4x128")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_bench.json"))
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
        dt = 0.01
        Xtraj = ac.rollout(X0, U, dt)
        out = {}
        ws = ac.wgrad_workspace("rollout", B, H)
        wbar = torch.empty(ac.mlp_grad_floats(), device=dev)
        out["rollout_wgrad"] = timed(lambda: ac.rollout_wgrad(Xtraj, U, dt, G, ws=ws, out=wbar), args.warmup, args.reps)
        ac.vjp_route = "composed"
        wsv = ac.vjp_workspace("rollout", B, H)
        out["rollout_vjp"] = timed(lambda: ac.rollout_vjp(Xtraj, U, dt, G, ws=wsv), args.warmup, args.reps)
        del wsv
        # the B H steps as flat units (X_k, U_k) with some cotangent: the step gradient and its seeds on their own
        n = B * H
        Xu = Xtraj[:H].permute(1, 0, 2).reshape(13, n).contiguous()
        Uu = U.permute(1, 0, 2).reshape(7, n).contiguous()
        Lu = G[1:].permute(1, 0, 2).reshape(13, n).contiguous()
        out["step_wgrad"] = timed(lambda: ac.step_wgrad(Xu, Uu, dt, Lu, ws=ws, out=wbar), args.warmup, args.reps)
        out["seeds"] = timed(lambda: ac.step_wgrad_seeds(Xu, Uu, dt, Lu, ws=ws), args.warmup, args.reps)
        out["wgrad_kernel_and_reduce_ms"] = out["step_wgrad"]["median_ms"] - out["seeds"]["median_ms"]
        Z, Yb = ac.step_wgrad_seeds(Xu, Uu, dt, Lu, ws=ws)
        ref = ac.step_wgrad(Xu, Uu, dt, Lu, ws=ws).clone()
        params = autodiff.MlpParameters(ac)
        layers = [(W.detach().to(dev).requires_grad_(True), b.detach().to(dev).requires_grad_(True)) for W, b in params.folded()]
        z = Z.permute(0, 2, 1).reshape(-1, 5).contiguous()
        yb = Yb.permute(0, 2, 1).reshape(-1, 6).contiguous()

        def torch_route():
            h = z
            for l, (W, b) in enumerate(layers):
                h = torch.addmm(b, h, W.t())
                if l < len(layers) - 1:
                    h = torch.tanh(h)
            return torch.autograd.grad((h * yb).sum(), [t for Wb in layers for t in Wb])

        out["torch_f32"] = timed(torch_route, args.warmup, args.reps)
        alt = torch.cat([t.reshape(-1) for t in torch_route()])
        out["torch_vs_kernel_max_rel"] = float((ref - alt).abs().max() / ref.abs().max())
        widths = ac.mlp_folded_shape()
        P = sum(a * b for a, b in zip(widths[:-1], widths[1:]))
        floor_ms = 6.0 * P * 4 * n / (MFMA_F32_TFLOPS * 1e12) * 1e3
        out.update(folded_widths=widths, flop_per_unit=6 * P * 4, mfma_floor_ms=floor_ms,
                   fraction_of_floor=floor_ms / max(out["wgrad_kernel_and_reduce_ms"], 1e-9), kernel=ac.last_launch()[0])
        res["models"][model] = out
        del ws, Z, Yb, z, yb
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
