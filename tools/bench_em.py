#!/usr/bin/env python3
"""Times ac_ekf_em_f32 (the EM statistics for the EKF's noise variances: k_ekf_em_nodes + k_ekf_em_reduce) beside
ac_ekf_smooth_f32 and ac_ekf_filter_rec_f32 on the same n and T in the same run, and beside its byte floor.

    python tools/bench_em.py                              # (n, T) = (4096, 50), (65536, 50), (16, 16384); cubic fits and default
    python tools/bench_em.py --shapes 4096x50 --models poly

The records come from one ac_ekf_filter_rec_f32 run on trims with noisy measurements (GPS rows every tenth step) and the
smoothed trace from one ac_ekf_smooth_f32 run over them.  Each part is warmed up, then timed with device events around a
window of repeated calls at least --window seconds long (at least three calls); the median of --rounds rounds is reported with
the spread.  The calls go to the C ABI on preallocated buffers (no allocation inside the window).  The byte floor is what a
node must move, 330 floats read x 4 B x n x T, at the achievable HBM rate of 6.29 TB/s.  `iteration` is one EM iteration:
filter (recording), smoother, statistic.  One JSON line per model and shape.
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

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of one MI355X
NODE_READ = 330            # floats per instance and node: P-, P^s (144 each), x-, x^s (13 each), z (15), used (1)


def timed(torch, fn, window):
    """Milliseconds per call of fn: warm-up, a probe to size the window, then one window between two device events."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(2):
        fn()
    b.record()
    torch.cuda.synchronize()
    per = max(a.elapsed_time(b) / 2, 1e-3)
    reps = int(min(max(window * 1e3 / per, 3), 20000))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, default="4096x50,65536x50,16x16384", help="n x T, comma separated")
    ap.add_argument("--models", type=str, default="poly,default")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated calls per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, default="filter_rec,smooth,em,em_sums_only,iteration",
                    help="what to time (a counter run names em alone)")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_em.py needs the GPU: there is nothing to time without it")
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    for model in args.models.split(","):
        ac = make(model)
        for n, T in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
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
            z = ac.measure(ac.state_update(x, u, 0.01))
            Z = z.unsqueeze(0) + torch.sqrt(Rd).unsqueeze(0) * torch.randn((T, 15, n), generator=gen, **f32)
            U = u.unsqueeze(0).expand(T, 7, n).contiguous()
            mask = torch.full((T, n), 0x7FFF & ~0x3F, **i32)
            mask[9::10] = 0x7FFF
            ws = ac.ekf_workspace(n)
            ews = ac.ekf_em_workspace(n, T)
            Xo, Po, ll = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32), torch.empty(n, **f32)
            Xf, Xp, Xs = (torch.empty((T, 13, n), **f32) for _ in range(3))
            Pf, Pp, Ab, Ps = (torch.empty((T, 12, 12, n), **f32) for _ in range(4))
            used, fst, sst, est = (torch.empty((T, n), **i32) for _ in range(4))
            Qsum, Rsum, Qn, Rn = (torch.empty((rows, n), **f32) for rows in (12, 15, 12, 15))
            nq, nr = torch.empty((n,), **i32), torch.empty((15, n), **i32)
            lib = ac._sync()
            o = _lib.EkfOpts()
            o.mag_ned[:] = ac.EKF_MAG_NED
            o.predict = 1
            eo = _lib.EkfEmOpts()
            eo.mag_ned[:] = ac.EKF_MAG_NED
            eo.floor_rel = 0.0

            def filt():
                _lib.check(lib.ac_ekf_filter_rec_f32(
                    ac._handle, C.byref(o), x.data_ptr(), P.data_ptr(), U.data_ptr(), C.c_float(0.01), Z.data_ptr(), mask.data_ptr(),
                    Qd.data_ptr(), Rd.data_ptr(), n, T, Xo.data_ptr(), Po.data_ptr(), ll.data_ptr(), Xf.data_ptr(), Pf.data_ptr(), None, None,
                    None, used.data_ptr(), fst.data_ptr(), Xp.data_ptr(), Pp.data_ptr(), Ab.data_ptr(), ws.data_ptr(), ws.numel(),
                    ac._stream()), "ac_ekf_filter_rec_f32")

            def smooth():
                _lib.check(lib.ac_ekf_smooth_f32(ac._handle, None, None, Xf.data_ptr(), Pf.data_ptr(), Xp.data_ptr(), Pp.data_ptr(),
                                                 Ab.data_ptr(), n, T, Xs.data_ptr(), Ps.data_ptr(), None, None, None, sst.data_ptr(),
                                                 ac._stream()), "ac_ekf_smooth_f32")

            def em(new=True):
                _lib.check(lib.ac_ekf_em_f32(ac._handle, C.byref(eo), Xp.data_ptr(), Pp.data_ptr(), Xs.data_ptr(), Ps.data_ptr(), Z.data_ptr(),
                                             used.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), n, T, Qsum.data_ptr(), Rsum.data_ptr(),
                                             nq.data_ptr(), nr.data_ptr(), est.data_ptr(), Qn.data_ptr() if new else None,
                                             Rn.data_ptr() if new else None, ews.data_ptr(), ews.numel(), ac._stream()), "ac_ekf_em_f32")

            def iteration():
                filt()
                smooth()
                em()

            iteration()
            torch.cuda.synchronize()
            parts = {"filter_rec": filt, "smooth": smooth, "em": em, "em_sums_only": lambda: em(False), "iteration": iteration}
            parts = {k: parts[k] for k in args.parts.split(",")}
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            em()
            torch.cuda.synchronize()
            floor = NODE_READ * 4 * n * T / HBM_BYTES_PER_S * 1e3
            print(json.dumps({
                "model": model, "n": n, "T": T, "chunks": (T + _lib.EM_CHUNK - 1) // _lib.EM_CHUNK, "ms": ms, "spread_over_rounds": spread,
                "trimmed": int(trim.converged.sum().item()), "filter_status_ok": int((fst == 0).all(dim=0).sum().item()),
                "smooth_status_ok": int((sst == 0).all(dim=0).sum().item()), "em_status_ok": int((est == 0).all(dim=0).sum().item()),
                "byte_floor_ms": floor, "em_over_byte_floor": ms["em"] / floor if "em" in ms else None,
                "em_over_smooth": ms["em"] / ms["smooth"] if "em" in ms and "smooth" in ms else None,
                "em_nodes_per_s": n * T / (ms["em"] * 1e-3) if "em" in ms else None,
                "smooth_nodes_per_s": n * T / (ms["smooth"] * 1e-3) if "smooth" in ms else None,
                "sigma_q_new_over_old": [float(v) for v in torch.sqrt(Qn / Qd).mean(dim=1).cpu()],
                "sigma_r_new_over_old": [float(v) for v in torch.sqrt(Rn / Rd).mean(dim=1).cpu()]}), flush=True)
            del ws, ews, Xf, Xp, Xs, Pf, Pp, Ab, Ps, Z, U
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
