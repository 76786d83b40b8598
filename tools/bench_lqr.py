#!/usr/bin/env python3
"""Times ac_lqr_f32 — the whole call and its three launches (the handle's step-sensitivity launch, the projection, the
Riccati solve) — and the gain expansion and the chart, per model and batch size.

    python tools/bench_lqr.py                         # n = 4096 and 65 536; cubic fits, default model, the shipped net
    python tools/bench_lqr.py --sizes 4096 --models poly

Each part is warmed up, then timed with device events around a window of repeated launches at least --window seconds long;
the median of --rounds rounds is reported with the spread.  The projection and the Riccati kernel are not callable alone
through the ABI: their times are differences (whole call with iters = 1 and with the default iters; whole call minus the
step-sensitivity launch).  One JSON line per model and size.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.bench_mppi import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default,nn")
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--horizon", type=int, default=50, help="nodes of the gain expansion")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_lqr.py needs the GPU: there is nothing to time without it")
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    for model in args.models.split(","):
        ac = make(model)
        for n in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(0)
            V = torch.tensor(rng.uniform(30, 60, n), dtype=torch.float32, device=dev)
            psid = torch.tensor(rng.uniform(-0.1, 0.1, n), dtype=torch.float32, device=dev)
            kw = dict(rudder=torch.zeros(n, device=dev)) if model == "linear" else {}
            trim = ac.trim(V, turn_rate=psid, **kw)
            x, u = trim.x.contiguous(), trim.u.contiguous()
            ws = ac.lqr_workspace(n)
            q11 = [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
            res = ac.lqr((x, u), 0.01, q=q11, iters=args.iters, ws=ws)
            H = args.horizon
            Xnom = ac.rollout(x, u.unsqueeze(0).expand(H, -1, -1).contiguous(), 0.01)
            sens_out = tuple(torch.empty(s, device=dev) for s in ((13, n), (13, 13, n), (13, 7, n))) + (None,)
            parts = {
                "lqr": lambda: ac.lqr((x, u), 0.01, q=q11, iters=args.iters, ws=ws),
                "lqr_iters1": lambda: ac.lqr((x, u), 0.01, q=q11, iters=1, ws=ws),
                "step_sens": lambda: ac.step_sens(x, u, 0.01, want_c=False, out=sens_out),
                "gains": lambda: res.gains(Xnom),
                "steady_error": lambda: ac.steady_error(x, x),
            }
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            per_iter = (ms["lqr"] - ms["lqr_iters1"]) / max(args.iters - 1, 1)
            print(json.dumps({
                "model": model, "n": n, "iters": args.iters, "horizon": H, "ms": ms, "spread_over_rounds": spread,
                "trimmed": int(trim.converged.sum().item()), "converged": int(res.converged.sum().item()),
                "doubling_steps_max": int(res.iterations.max().item()),
                "riccati_ms_per_doubling_step": per_iter,
                "riccati_ms": per_iter * args.iters,
                "projection_and_gain_ms": ms["lqr_iters1"] - ms["step_sens"] - per_iter,
                "lqr_over_step_sens": ms["lqr"] / ms["step_sens"],
                "designs_per_s": n / (ms["lqr"] * 1e-3)}), flush=True)
            del ws, res, Xnom, sens_out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
