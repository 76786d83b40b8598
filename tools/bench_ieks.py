#!/usr/bin/env python3
"""Times one linearised pass of the iterated Kalman smoother (ac_ieks_pass_f32: one sensitivity launch over the T n units and
k_ieks_filter) plus the RTS sweep, and one full Gauss-Newton iteration (pass, sweep, candidates, one step launch and the cost
over the ladder's candidates, accept), beside ac_ekf_filter_rec_f32 + ac_ekf_smooth_f32 on the same n and T in the same run.

    python tools/bench_ieks.py                                   # n = 65 536 x T = 50 and n = 16 x T = 16 384; cubic fits
    python tools/bench_ieks.py --shapes 4096x50 --models poly,default

The log is a trim flown under noisy measurements (GPS rows every tenth step); the nominal is the filter's own smoothed trace.
Each part is warmed up, then timed with device events around a window of repeated calls at least --window seconds long; the
median of --rounds rounds is reported with the spread.  The calls go to the C ABI on preallocated buffers (no allocation inside
the window).  One JSON line per model and shape.
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

LADDER = (1.0, 0.5, 0.25, 0.125)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="65536x50,16x16384", help="n x T, comma separated")
    ap.add_argument("--models", type=str, default="poly")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of repeated calls per timing")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_ieks.py needs the GPU: there is nothing to time without it")
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    Cn = len(LADDER)
    lad = (C.c_float * Cn)(*LADDER)
    for model in args.models.split(","):
        ac = make(model)
        for n, T in ((int(a) for a in s.split("x")) for s in args.shapes.split(",")):
            rng = np.random.default_rng(0)
            V = torch.tensor(rng.uniform(30, 60, n), dtype=torch.float32, device=dev)
            psid = torch.tensor(rng.uniform(-0.1, 0.1, n), dtype=torch.float32, device=dev)
            trim = ac.trim(V, turn_rate=psid)
            x, u = trim.x.contiguous(), trim.u.contiguous()
            f32, i32 = dict(device=dev, dtype=torch.float32), dict(device=dev, dtype=torch.int32)
            t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)  # noqa: E731
            P = t(np.repeat(np.diag(SIG_P0 ** 2)[:, :, None], n, axis=2))
            Qd, Rd = t(np.repeat((SIG_Q ** 2)[:, None], n, axis=1)), t(np.repeat((SIG_R ** 2)[:, None], n, axis=1))
            gen = torch.Generator(dev).manual_seed(0)
            U = u.unsqueeze(0).expand(T, 7, n).contiguous()
            truth = ac.rollout(x, U, 0.01)
            Z = torch.stack([ac.measure(truth[k + 1]) + torch.sqrt(Rd) * torch.randn((15, n), generator=gen, **f32) for k in range(T)])
            mask = torch.full((T, n), 0x7FFF & ~0x3F, **i32)
            mask[9::10] = 0x7FFF
            ws, iws = ac.ekf_workspace(n), ac.ieks_workspace(n, T, Cn)
            e = lambda *s: torch.empty(s, **f32)  # noqa: E731
            Xo, Po, ll = e(13, n), e(12, 12, n), e(n)
            Xf, Xp, Xs = (e(T, 13, n) for _ in range(3))
            Pf, Pp, Ab, Ps = (e(T, 12, 12, n) for _ in range(4))
            Xs0, Ps0, Xb = e(13, n), e(12, 12, n), e(T + 1, 13, n)
            Xc, Uc, Jc, J0, J1, al = e(T + 1, 13, Cn * n), e(T, 7, Cn * n), e(Cn * n), e(n), e(n), e(n)
            fst, sst = torch.empty((T, n), **i32), torch.empty((T, n), **i32)
            stc, st = torch.empty((Cn * n,), **i32), torch.zeros((n,), **i32)
            lib = ac._sync()
            o = _lib.EkfOpts()
            o.mag_ned[:] = ac.EKF_MAG_NED
            o.predict = 1
            s = ac._stream()
            data = (C.c_float(0.01), Z.data_ptr(), mask.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), n)
            prior = (ac._handle, C.byref(o), x.data_ptr(), P.data_ptr())

            def filt():
                _lib.check(lib.ac_ekf_filter_rec_f32(*prior, U.data_ptr(), *data, T, Xo.data_ptr(), Po.data_ptr(), ll.data_ptr(), Xf.data_ptr(),
                                                     Pf.data_ptr(), None, None, None, None, fst.data_ptr(), Xp.data_ptr(), Pp.data_ptr(),
                                                     Ab.data_ptr(), ws.data_ptr(), ws.numel(), s), "ac_ekf_filter_rec_f32")

            def smooth():
                _lib.check(lib.ac_ekf_smooth_f32(ac._handle, x.data_ptr(), P.data_ptr(), Xf.data_ptr(), Pf.data_ptr(), Xp.data_ptr(),
                                                 Pp.data_ptr(), Ab.data_ptr(), n, T, Xs.data_ptr(), Ps.data_ptr(), Xs0.data_ptr(), Ps0.data_ptr(),
                                                 None, sst.data_ptr(), s), "ac_ekf_smooth_f32")

            def ipass():
                _lib.check(lib.ac_ieks_pass_f32(*prior, Xb.data_ptr(), U.data_ptr(), *data, T, Xf.data_ptr(), Pf.data_ptr(), ll.data_ptr(), None,
                                                None, None, None, fst.data_ptr(), Xp.data_ptr(), Pp.data_ptr(), Ab.data_ptr(), iws.data_ptr(),
                                                iws.numel(), s), "ac_ieks_pass_f32")

            def cost(Xt, Ut, reps, J, stat):
                _lib.check(lib.ac_ieks_cost_f32(*prior, Xt.data_ptr(), Ut.data_ptr(), *data, reps, T, J.data_ptr(), None, None, None,
                                                stat.data_ptr(), iws.data_ptr(), iws.numel(), s), "ac_ieks_cost_f32")

            def line_search():
                _lib.check(lib.ac_ieks_candidates_f32(ac._handle, Xb.data_ptr(), Xs0.data_ptr(), Xs.data_ptr(), U.data_ptr(), lad, Cn, n, T,
                                                      Xc.data_ptr(), Uc.data_ptr(), s), "ac_ieks_candidates_f32")
                cost(Xc, Uc, Cn, Jc, stc)
                _lib.check(lib.ac_ieks_accept_f32(ac._handle, J0.data_ptr(), Jc.data_ptr(), stc.data_ptr(), Xc.data_ptr(), lad, Cn, n, T,
                                                  Xb.data_ptr(), al.data_ptr(), J1.data_ptr(), st.data_ptr(), s), "ac_ieks_accept_f32")

            filt()
            smooth()
            Xb[0].copy_(Xs0)
            Xb[1:].copy_(Xs)
            cost(Xb, U, 1, J0, st)
            torch.cuda.synchronize()
            nominal = Xb.clone()

            def iteration():
                ipass()
                smooth()
                line_search()

            parts = {"filter_rec": filt, "smooth": smooth, "pass": ipass, "pass_smooth": lambda: (ipass(), smooth()), "iteration": iteration}
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    Xb.copy_(nominal)
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            print(json.dumps({
                "model": model, "n": n, "T": T, "ms": ms, "spread_over_rounds": spread, "trimmed": int(trim.converged.sum().item()),
                "pass_status_ok": int((fst == 0).all(dim=0).sum().item()), "smooth_status_ok": int((sst == 0).all(dim=0).sum().item()),
                "pass_over_filter_rec": ms["pass"] / ms["filter_rec"],
                "pass_smooth_over_filter_smooth": ms["pass_smooth"] / (ms["filter_rec"] + ms["smooth"]),
                "iteration_over_filter_smooth": ms["iteration"] / (ms["filter_rec"] + ms["smooth"]),
                "nodes_per_s_pass": n * T / (ms["pass"] * 1e-3)}), flush=True)
            del ws, iws, Xf, Xp, Xs, Pf, Pp, Ab, Ps, Z, U, Xc, Uc, truth
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
