#!/usr/bin/env python3
"""Times ac_ukf_step_f32 — the whole step and its three launches (k_ukf_sigma, the handle's forward step over the 25 n sigma
points, k_ukf_update) — beside ac_ekf_step_f32 and its step-sensitivity launch in the same run, per model and batch size.

    python tools/bench_ukf.py                         # n = 4096 and 65 536; cubic fits, default model, shipped net, 4x128 net
    python tools/bench_ukf.py --sizes 4096 --models poly --out ""

tools/bench_ekf.py's protocol: each part is warmed up, then timed with device events around a window of repeated launches at
least --window seconds long; the median of --rounds rounds is reported with the spread.  The calls go to the C ABI on
preallocated buffers.  Neither UKF kernel is callable alone through the ABI: the forward step is timed alone on the workspace's
own 25 n points, the two kernels together are the whole step minus that, and k_ukf_update<false> is the measurement update
alone (predict = 0).  One JSON line per model and size, written to --out.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from aircraft_amd import _lib  # noqa: E402
from tools.bench_ekf import SIG_P0, SIG_Q, SIG_R  # noqa: E402
from tools.bench_mppi import timed  # noqa: E402


def make(model):
    from examples.glide_polar import make as make_glider

    if model != "net4":
        return make_glider(model)
    from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
    from aircraft_amd.synthetic import GLIDER

    return Aircraft(AircraftOpts(coeff_model_type="nn", coeff_model_path=MlpData.synthetic((128,) * 4, seed=42),
                                 aircraft_config=AircraftConfiguration(dict(GLIDER)), physical_integration_substeps=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default,nn,net4")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ukf_bench.jsonl"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_ukf.py needs the GPU: there is nothing to time without it")
    from aircraft_amd.synthetic import TRIM_STATE

    dev = torch.device("cuda", 0)
    lines = []
    for model in args.models.split(","):
        ac = make(model)
        for n in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(0)
            f32 = dict(device=dev, dtype=torch.float32)
            t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
            if model == "net4":  # (the synthetic net has no trims of its own)
                x, u = t(np.repeat(TRIM_STATE[:, None], n, axis=1)), torch.zeros((7, n), **f32)
            else:
                V = torch.tensor(rng.uniform(30, 60, n), **f32)
                trim = ac.trim(V, turn_rate=torch.tensor(rng.uniform(-0.1, 0.1, n), **f32))
                x, u = trim.x.contiguous(), trim.u.contiguous()
            P = t(np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2))
            Qd, Rd = t(np.repeat((SIG_Q ** 2)[:, None], n, axis=1)), t(np.repeat((SIG_R ** 2)[:, None], n, axis=1))
            z = ac.measure(ac.state_update(x, u, 0.01)) + torch.sqrt(Rd) * torch.randn((15, n), generator=torch.Generator(dev).manual_seed(0), **f32)
            ws = {"ekf": ac.ekf_workspace(n), "ukf": ac.ukf_workspace(n)}
            Xo, Po = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)
            nu, S, nis, ll = torch.empty((15, n), **f32), torch.empty((15, n), **f32), torch.empty(n, **f32), torch.empty(n, **f32)
            used, st = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
            sens_out = tuple(torch.empty(s, device=dev) for s in ((13, n), (13, 13, n), (13, 7, n))) + (None,)
            lib = ac._sync()

            def step(kind, predict):
                o = _lib.UkfOpts() if kind == "ukf" else _lib.EkfOpts()
                o.mag_ned[:] = ac.EKF_MAG_NED
                o.predict = predict
                fn = getattr(lib, f"ac_{kind}_step_f32")
                w = ws[kind]
                return lambda: _lib.check(fn(ac._handle, C.byref(o), x.data_ptr(), P.data_ptr(), u.data_ptr(), C.c_float(0.01),
                                             z.data_ptr(), None, Qd.data_ptr(), Rd.data_ptr(), n, Xo.data_ptr(), Po.data_ptr(),
                                             nu.data_ptr(), S.data_ptr(), nis.data_ptr(), ll.data_ptr(), used.data_ptr(), st.data_ptr(),
                                             None, None, None, w.data_ptr(), w.numel(), ac._stream()), f"ac_{kind}_step_f32")

            step("ukf", 1)()  # the workspace now holds the 25 n points and the replicated controls
            torch.cuda.synchronize()
            ukf_status_ok = int((st == 0).sum().item())
            base = (ws["ukf"].data_ptr() + 255) & ~255
            pts = torch.empty((13, 25 * n), **f32)
            u25 = u.repeat(1, 25).contiguous()
            off = (base - ws["ukf"].data_ptr()) // 4
            pts.copy_(ws["ukf"][off:off + 13 * 25 * n].view(13, 25 * n))
            img = torch.empty_like(pts)
            forward = lambda: _lib.check(lib.ac_step_f32(ac._handle, pts.data_ptr(), u25.data_ptr(), C.c_float(0.01), None, 25 * n,  # noqa: E731
                                                         img.data_ptr(), ac._stream()), "ac_step_f32")
            parts = {
                "ukf_step": step("ukf", 1), "ukf_forward_25n": forward, "ukf_update_only": step("ukf", 0),
                "ekf_step": step("ekf", 1), "ekf_step_sens": lambda: ac.step_sens(x, u, 0.01, want_c=False, out=sens_out),
                "ekf_update_only": step("ekf", 0),
            }
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            kernels = ms["ukf_step"] - ms["ukf_forward_25n"]  # k_ukf_sigma + k_ukf_update<1>
            line = {"model": model, "n": n, "ms": ms, "spread_over_rounds": spread, "ukf_status_ok": ukf_status_ok,
                    "ukf_kernels_ms": kernels, "k_ekf_step_ms": ms["ekf_step"] - ms["ekf_step_sens"],
                    "ukf_over_ekf": ms["ukf_step"] / ms["ekf_step"],
                    "ukf_kernels_over_k_ekf_step": kernels / (ms["ekf_step"] - ms["ekf_step_sens"]),
                    "ukf_update_only_over_ekf_update_only": ms["ukf_update_only"] / ms["ekf_update_only"],
                    "ukf_filter_steps_per_s": n / (ms["ukf_step"] * 1e-3), "ekf_filter_steps_per_s": n / (ms["ekf_step"] * 1e-3)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del ws, sens_out, pts, img, u25
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
