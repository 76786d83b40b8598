#!/usr/bin/env python3
"""Times one step of the loop closed through the estimator (ac_lqg_rollout_f32 with T = 1: control law, forward step, process
noise, sensors, the estimator's step, score) beside its parts in the same run, per model and batch size.

    python tools/bench_lqg.py                         # n = 4096 and 65 536; cubic fits, default model, shipped net
    python tools/bench_lqg.py --sizes 4096 --models poly --out ""

tools/bench_ekf.py's protocol: each part is warmed up, then timed with device events around a window of repeated launches at
least --window seconds long; the median of --rounds rounds is reported with the spread.  The calls go to the C ABI on
preallocated buffers.  The forward step and the EKF / UKF step are the code the loop calls; the new kernels' time is the loop's
minus theirs, and each new kernel is also timed alone through its own entry point.  k_ekf_step alone is the EKF step minus its
sensitivity launch.  One JSON line per model and size, written to --out.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default,nn")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "lqg_bench.jsonl"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_lqg.py needs the GPU: there is nothing to time without it")
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    lines = []
    for model in args.models.split(","):
        ac = make(model)
        for n in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(0)
            f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
            t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
            V = torch.tensor(rng.uniform(30, 60, n), **f32)
            trim = ac.trim(V, turn_rate=torch.tensor(rng.uniform(-0.1, 0.1, n), **f32))
            x, u = trim.x.contiguous(), trim.u.contiguous()
            res = ac.lqr((x, u), 0.01)
            Xnom = torch.stack([x, ac.state_update(x, u, 0.01)]).contiguous()
            Kx = res.gains(Xnom).contiguous()
            Unom = u.unsqueeze(0).contiguous()
            P = t(np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2))
            Qd, Rd = t(np.repeat((SIG_Q ** 2)[:, None], n, axis=1)), t(np.repeat((SIG_R ** 2)[:, None], n, axis=1))
            sq, sr = torch.sqrt(Qd), torch.sqrt(Rd)
            xh = x + 0.0
            xh[0:3] += 1.0
            ws = {k: ac.lqg_workspace(k, n) for k in ("ekf", "ukf")}
            Xo, Po, xn, U = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32), torch.empty((13, n), **f32), torch.empty((7, n), **f32)
            Z, M = torch.empty((15, n), **f32), torch.empty(n, **i32)
            nu, S, nis, ll, nees, err = (torch.empty(s, **f32) for s in ((15, n), (15, n), (n,), (n,), (n,), (12, n)))
            used, st, sst = (torch.empty(n, **i32) for _ in range(3))
            sens_out = tuple(torch.empty(s, device=dev) for s in ((13, n), (13, 13, n), (13, 7, n))) + (None,)
            lib = ac._sync()
            so = _lib.SenseOpts()
            so.mag_ned[:] = ac.EKF_MAG_NED
            so.seed_lo, so.period[:] = 1, (10, 10, 1, 1, 1)
            lim = _lib.IlqrCost()
            lim.u_min[:], lim.u_max[:] = [-25.0] * 7, [25.0] * 7
            h, stream = ac._handle, ac._stream()

            def loop(kind):
                o = _lib.LqgOpts()
                o.estimator, o.feedback, o.kappa, o.step0 = _lib.LQG_ESTIMATORS[kind], 0, 0.0, 9  # (step 10: every sensor reports)
                w = ws[kind]
                return lambda: _lib.check(lib.ac_lqg_rollout_f32(
                    h, C.byref(o), C.byref(so), C.byref(lim), x.data_ptr(), xh.data_ptr(), P.data_ptr(), Xnom.data_ptr(), Unom.data_ptr(),
                    Kx.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), sq.data_ptr(), sr.data_ptr(), C.c_float(0.01), n, 1, Xo.data_ptr(),
                    Po.data_ptr(), None, None, U.data_ptr(), None, Z.data_ptr(), M.data_ptr(), nis.data_ptr(), nees.data_ptr(),
                    used.data_ptr(), st.data_ptr(), sst.data_ptr(), err.data_ptr(), w.data_ptr(), w.numel(), stream), "ac_lqg_rollout_f32")

            def est(kind):
                o = _lib.UkfOpts() if kind == "ukf" else _lib.EkfOpts()
                o.mag_ned[:] = ac.EKF_MAG_NED
                o.predict = 1
                fn = getattr(lib, f"ac_{kind}_step_f32")
                w = ws[kind]
                return lambda: _lib.check(fn(h, C.byref(o), xh.data_ptr(), P.data_ptr(), U.data_ptr(), C.c_float(0.01), Z.data_ptr(),
                                             M.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), n, Xo.data_ptr(), Po.data_ptr(), nu.data_ptr(),
                                             S.data_ptr(), nis.data_ptr(), ll.data_ptr(), used.data_ptr(), st.data_ptr(), None, None, None,
                                             w.data_ptr(), w.numel(), stream), f"ac_{kind}_step_f32")

            loop("ekf")()  # U, Z, M, Xo, Po now hold a real step's values for the parts timed alone
            torch.cuda.synchronize()
            xn.copy_(ac.state_update(x, U, 0.01))
            parts = {
                "loop_ekf": loop("ekf"), "loop_ukf": loop("ukf"), "ekf_step": est("ekf"), "ukf_step": est("ukf"),
                "forward_step": lambda: _lib.check(lib.ac_step_f32(h, x.data_ptr(), U.data_ptr(), C.c_float(0.01), None, n, xn.data_ptr(),
                                                                   stream), "ac_step_f32"),
                "ekf_step_sens": lambda: ac.step_sens(xh, U, 0.01, want_c=False, out=sens_out),
                "policy": lambda: _lib.check(lib.ac_policy_f32(h, C.byref(lim), xh.data_ptr(), Xnom.data_ptr(), Unom.data_ptr(), Kx.data_ptr(),
                                                               n, U.data_ptr(), stream), "ac_policy_f32"),
                "disturb": lambda: _lib.check(lib.ac_disturb_f32(h, C.byref(so), 9, None, xn.data_ptr(), sq.data_ptr(), n, xn.data_ptr(),
                                                                 stream), "ac_disturb_f32"),
                "sense": lambda: _lib.check(lib.ac_sense_f32(h, C.byref(so), 10, None, xn.data_ptr(), sr.data_ptr(), n, Z.data_ptr(),
                                                             M.data_ptr(), stream), "ac_sense_f32"),
                "score": lambda: _lib.check(lib.ac_estimate_score_f32(h, xn.data_ptr(), Xo.data_ptr(), Po.data_ptr(), n, err.data_ptr(),
                                                                      nees.data_ptr(), sst.data_ptr(), stream), "ac_estimate_score_f32"),
            }
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            new = {k: ms[f"loop_{k}"] - ms["forward_step"] - ms[f"{k}_step"] for k in ("ekf", "ukf")}
            alone = ms["policy"] + ms["disturb"] + ms["sense"] + ms["score"]
            k_ekf = ms["ekf_step"] - ms["ekf_step_sens"]
            line = {"model": model, "n": n, "ms": ms, "spread_over_rounds": spread, "new_kernels_ms": new,
                    "new_kernels_share_of_loop": {k: new[k] / ms[f"loop_{k}"] for k in new}, "new_kernels_alone_ms": alone,
                    "k_ekf_step_ms": k_ekf, "new_kernels_alone_over_k_ekf_step": alone / k_ekf,
                    "loop_steps_per_s": {k: n / (ms[f"loop_{k}"] * 1e-3) for k in new}}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del ws, sens_out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
