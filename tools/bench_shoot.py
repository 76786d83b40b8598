#!/usr/bin/env python3
"""Times the multiple-shooting mode beside single shooting, built from the same tree, at two shapes
(B = 64 x H = 400, the goal-acquisition example's; B = 4096 x H = 50):

    iterate    one ILQR.iterate of shooting="multiple" (backward pass with the defects, direction, candidates as independent nodes
               in ONE step launch, merit, acceptance) against one of shooting="single" (backward pass, closed-loop rollouts of every
               alpha, cost, acceptance), each from the same restored iterate, with the parts of the multiple-shooting line search
    backward   k_ilqr_backward_shoot (ac_ilqr_backward_shoot_f32, with and without the Vx / Vxx output) against the unswitched
               kernel of the same <NODE, NEWTON> (ac_ilqr_backward_newton_f32 / _goal_f32), on random inputs in the shape of
               tests/riccati_ref.synthetic_riccati

    python tools/bench_shoot.py --out profiles/shoot_bench.json

Every part is warmed up on its real shapes, then timed with device events around a window of repeated launches at least --window
seconds long; the variants alternate over --rounds rounds, the median round is reported with the spread.  One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.bench_mppi import timed  # noqa: E402


def rounds_of(torch, parts, rounds, window):
    """the parts alternate within a round -> ({name: median ms}, {name: (max - min) / median})"""
    t = {k: [] for k in parts}
    for _ in range(rounds):
        for k, fn in parts.items():
            t[k].append(timed(torch, fn, window))
    return ({k: float(np.median(v)) for k, v in t.items()}, {k: float((max(v) - min(v)) / np.median(v)) for k, v in t.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="64x400,4096x50")
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_shoot.py needs the GPU: there is nothing to time without it")
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts
    from aircraft_amd.build import source_sha
    from aircraft_amd.control import ILQR, QuadraticCost
    from aircraft_amd.synthetic import GLIDER

    dev = torch.device("cuda", 0)
    poly = os.path.join(ROOT, "tests", "golden", "poly_coef.npz")
    ac = Aircraft(AircraftOpts(coeff_model_type="poly", coeff_model_path=poly, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                               physical_integration_substeps=1))
    out = {"source_sha": source_sha(), "window_s": args.window, "rounds": args.rounds, "shapes": {}}
    for shape in args.shapes.split(","):
        B, H = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(1)
        rn = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
        ru = lambda lo, hi, *s: lo + (hi - lo) * torch.rand(s, device=dev, generator=g)  # noqa: E731
        res = {"ms": {}, "spread_over_rounds": {}, "ratio": {}}

        # ---- one iteration of each mode, from the same iterate -------------------------------------------------------------------
        cost = QuadraticCost.goal((0.01 * H * 80.0, 2.0), reg=1.0)
        prob = {m: ILQR(system=ac, dt=0.01, num_nodes=H, cost=cost, shooting=m) for m in ("single", "multiple")}
        x0 = torch.tensor([0, 0, -200, 80, 0, 0, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=dev)[:, None].expand(13, B).contiguous()
        x0 = x0 + 0.05 * rn(13, B) * torch.tensor([0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1], device=dev)[:, None]
        Us = torch.zeros(H, 7, B, device=dev)
        Xs = prob["single"].rollout(x0, Us)
        X, U = Xs.clone(), Us.clone()

        def iterate(m):
            def fn():
                X.copy_(Xs); U.copy_(Us)
                prob[m].iterate(x0, X, U)
            return fn

        p = prob["multiple"]
        ws = p._workspace(B, dev)
        iterate("multiple")()   # fills the workspace the parts below read
        na = len(p.alphas)
        parts = {"iterate/single": iterate("single"), "iterate/multiple": iterate("multiple"),
                 "part/restore_iterate": lambda: (X.copy_(Xs), U.copy_(Us)),
                 "part/linearise": lambda: p.linearise(X, U, want_c=False, out=(ws["F"], ws["A"], ws["Bm"], None)),
                 "part/backward_shoot": lambda: p.backward(X, U, ws["A"], ws["Bm"], out=(ws["K"], ws["kff"], ws["dV"], ws["Vx"], ws["Vxx"]),
                                                           node=None, shoot=ws["F"]),
                 "part/direction": lambda: p.direction(X, ws["F"], ws["A"], ws["Bm"], ws["K"], ws["kff"], ws["Vx"], ws["Vxx"],
                                                       out=(ws["dX"], ws["dU"], ws["Lam"])),
                 "part/candidate_defects": lambda: p.defects(ws["Xc"], ws["Uc"]),
                 "part/candidate_cost": lambda: p.trajectory_cost(ws["Xc"], ws["Uc"], out=ws["Jc"]),
                 "part/candidate_merit": lambda: p._merit(ws["Jc"], ws["mu"], ws["phic"], ws["dinfc"], R=ws["Rc"]),
                 "part/single_forward": lambda: prob["single"].forward(x0, Xs, Us, ws["K"], ws["kff"], out=(ws["Xc"], ws["Uc"]))}
        ms, sp = rounds_of(torch, parts, args.rounds, args.window)
        res["ms"].update(ms); res["spread_over_rounds"].update(sp)
        res["ratio"]["iterate multiple/single"] = ms["iterate/multiple"] / ms["iterate/single"]
        res["candidate_nodes_per_launch"] = na * B * H

        # ---- the backward kernel beside its unswitched twin ----------------------------------------------------------------------
        base = QuadraticCost(q=[1.0] * 13, qf=[2.0] * 13, r=[0.5] * 7, reg=0.25)
        il = ILQR(system=ac, dt=0.01, num_nodes=H, cost=base)
        A = torch.eye(13, device=dev)[None, :, :, None] + 0.05 * rn(H, 13, 13, B)
        Bm = 0.1 * rn(H, 13, 7, B)
        Xr, Ur = rn(H + 1, 13, B), rn(H, 7, B)
        F = (Xr[1:] + 0.3 * rn(H, 13, B)).contiguous()
        node = (ru(0.2, 2.0, H + 1, 13, B), rn(H + 1, 13, B), 0.5 * rn(H + 1, 13, B))
        S = 0.03 * rn(H, 21, 21, B)
        Hz = (S + S.transpose(1, 2)).contiguous()
        ug = 0.5 * rn(H, 7, B)
        o3 = (torch.empty((H, 7, 13, B), device=dev), torch.empty((H, 7, B), device=dev), torch.empty((2, B), device=dev))
        ov = (torch.empty((H, 13, B), device=dev), torch.empty((H, 13, 13, B), device=dev))
        variants = {"gn": dict(node=None), "node": dict(node=node), "newton": dict(node=None, Hz=Hz), "goal": dict(node=node, Hz=Hz, uglin=ug)}
        for name, kw in variants.items():
            parts = {f"backward/{name}/unswitched": (lambda kw: lambda: il.backward(Xr, Ur, A, Bm, out=o3, **kw))(kw),
                     f"backward/{name}/shoot": (lambda kw: lambda: il.backward(Xr, Ur, A, Bm, out=o3 + ov, shoot=F, **kw))(kw),
                     f"backward/{name}/shoot_no_V": (lambda kw: lambda: il.backward(Xr, Ur, A, Bm, out=o3 + (None, None), shoot=F, **kw))(kw)}
            ms, sp = rounds_of(torch, parts, args.rounds, args.window)
            res["ms"].update(ms); res["spread_over_rounds"].update(sp)
            for k in ("shoot", "shoot_no_V"):
                res["ratio"][f"backward/{name}/{k}"] = ms[f"backward/{name}/{k}"] / ms[f"backward/{name}/unswitched"]
            assert bool(torch.isfinite(o3[0]).all())
        out["shapes"][shape] = res
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
