#!/usr/bin/env python3
"""Times ac_ekf_step_f32 — the whole step and its two launches (the handle's step-sensitivity launch, k_ekf_step) — the
measurement update alone and ac_ekf_measure_f32, per model and batch size.

    python tools/bench_ekf.py                         # n = 4096 and 65 536; cubic fits, default model, the shipped net
    python tools/bench_ekf.py --sizes 4096 --models poly

Each part is warmed up, then timed with device events around a window of repeated launches at least --window seconds long;
the median of --rounds rounds is reported with the spread.  The calls go to the C ABI on preallocated buffers (no
allocation inside the window).  k_ekf_step with the time update is not callable alone: its time is the whole step minus
the step-sensitivity launch, which is timed on the same inputs in the same run.  One JSON line per model and size.
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
from tools.bench_mppi import timed  # noqa: E402

SIG_P0 = np.array([2, 2, 2, 0.5, 0.5, 0.5, 0.03, 0.03, 0.05, 0.05, 0.05, 0.05])
SIG_Q = np.array([0.01] * 3 + [0.05] * 3 + [0.002] * 3 + [0.02] * 3)
SIG_R = np.array([1.5, 1.5, 3, 0.2, 0.2, 0.3, 0.01, 0.01, 0.01, 0.5, 0.01, 0.01, 0.02, 0.02, 0.02])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default,nn")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_ekf.py needs the GPU: there is nothing to time without it")
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
            f32 = dict(device=dev, dtype=torch.float32)
            t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
            P = t(np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2))
            Qd, Rd = t(np.repeat((SIG_Q ** 2)[:, None], n, axis=1)), t(np.repeat((SIG_R ** 2)[:, None], n, axis=1))
            z = ac.measure(ac.state_update(x, u, 0.01)) + torch.sqrt(Rd) * torch.randn((15, n), generator=torch.Generator(dev).manual_seed(0), **f32)
            ws = ac.ekf_workspace(n)
            Xo, Po = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)
            nu, S, nis, ll = torch.empty((15, n), **f32), torch.empty((15, n), **f32), torch.empty(n, **f32), torch.empty(n, **f32)
            used, st = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
            sens_out = tuple(torch.empty(s, device=dev) for s in ((13, n), (13, 13, n), (13, 7, n))) + (None,)
            lib = ac._sync()
            opts = {}
            for predict in (0, 1):
                o = _lib.EkfOpts()
                o.mag_ned[:] = ac.EKF_MAG_NED
                o.predict = predict
                opts[predict] = o

            def step(predict):
                _lib.check(lib.ac_ekf_step_f32(ac._handle, C.byref(opts[predict]), x.data_ptr(), P.data_ptr(), u.data_ptr(), C.c_float(0.01),
                                               z.data_ptr(), None, Qd.data_ptr(), Rd.data_ptr(), n, Xo.data_ptr(), Po.data_ptr(),
                                               nu.data_ptr(), S.data_ptr(), nis.data_ptr(), ll.data_ptr(), used.data_ptr(), st.data_ptr(),
                                               None, None, None, ws.data_ptr(), ws.numel(), ac._stream()), "ac_ekf_step_f32")

            parts = {
                "ekf_step": lambda: step(1),
                "step_sens": lambda: ac.step_sens(x, u, 0.01, want_c=False, out=sens_out),
                "update_only": lambda: step(0),
                "measure": lambda: ac.measure(x),
            }
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            step(1)
            torch.cuda.synchronize()
            k_ms = ms["ekf_step"] - ms["step_sens"]
            print(json.dumps({
                "model": model, "n": n, "ms": ms, "spread_over_rounds": spread, "trimmed": int(trim.converged.sum().item()),
                "status_ok": int((st == 0).sum().item()),
                "k_ekf_step_ms": k_ms, "k_ekf_step_over_step_sens": k_ms / ms["step_sens"],
                "filter_steps_per_s": n / (ms["ekf_step"] * 1e-3),
                "k_ekf_step_GBps": n * 2300 / (k_ms * 1e-3) / 1e9}), flush=True)
            del ws, sens_out
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
