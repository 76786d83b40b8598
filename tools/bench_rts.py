#!/usr/bin/env python3
"""Times ac_ekf_smooth_f32 (the RTS smoother's one launch, k_ekf_smooth) beside ac_ekf_filter_f32 on the same n and T in the
same run, and beside the smoother's byte floor, per model and batch size.

    python tools/bench_rts.py                         # n = 4096 and 65 536, T = 50; cubic fits and default model
    python tools/bench_rts.py --sizes 4096 --models poly --steps 20

The records come from one ac_ekf_filter_rec_f32 run on trims with noisy measurements (GPS rows every tenth step).  Each part
is warmed up, then timed with device events around a window of repeated calls at least --window seconds long; the median of
--rounds rounds is reported with the spread.  The calls go to the C ABI on preallocated buffers (no allocation inside the
window).  The byte floor is what a link must move, (458 floats read + 157 written, + 144 with the gains) x 4 B x n x links,
at the achievable HBM rate of 6.29 TB/s.  One JSON line per model and size.
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

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy rate of one MI355X
LINK_READ, LINK_WRITE, LINK_GAINS = 458, 157, 144  # floats per instance and link


def floor_ms(n, links, gains):
    return (LINK_READ + LINK_WRITE + (LINK_GAINS if gains else 0)) * 4 * n * links / HBM_BYTES_PER_S * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default")
    ap.add_argument("--steps", type=int, default=50, help="T, the filter steps of the run")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of repeated calls per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", type=str, default="filter,filter_rec,smooth,smooth_gains,smooth_initial",
                    help="what to time (a counter run names the smoother parts alone)")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_rts.py needs the GPU: there is nothing to time without it")
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    T = args.steps
    for model in args.models.split(","):
        ac = make(model)
        for n in (int(s) for s in args.sizes.split(",")):
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
            Z = torch.stack([z + torch.sqrt(Rd) * torch.randn((15, n), generator=gen, **f32) for _ in range(T)])
            U = u.unsqueeze(0).expand(T, 7, n).contiguous()
            mask = torch.full((T, n), 0x7FFF & ~0x3F, **i32)
            mask[9::10] = 0x7FFF
            ws = ac.ekf_workspace(n)
            Xo, Po, ll = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32), torch.empty(n, **f32)
            Xf, Xp, Xs = (torch.empty((T, 13, n), **f32) for _ in range(3))
            Pf, Pp, Ab, Ps, Cg = (torch.empty((T, 12, 12, n), **f32) for _ in range(5))
            Xs0, Ps0 = torch.empty((13, n), **f32), torch.empty((12, 12, n), **f32)
            fst, sst = torch.empty((T, n), **i32), torch.empty((T, n), **i32)
            lib = ac._sync()
            o = _lib.EkfOpts()
            o.mag_ned[:] = ac.EKF_MAG_NED
            o.predict = 1
            head = (ac._handle, C.byref(o), x.data_ptr(), P.data_ptr(), U.data_ptr(), C.c_float(0.01), Z.data_ptr(), mask.data_ptr(),
                    Qd.data_ptr(), Rd.data_ptr(), n, T, Xo.data_ptr(), Po.data_ptr(), ll.data_ptr(), Xf.data_ptr(), Pf.data_ptr(), None,
                    None, None, None, fst.data_ptr())
            tail = (ws.data_ptr(), ws.numel(), ac._stream())

            def filt(record):
                if record:
                    _lib.check(lib.ac_ekf_filter_rec_f32(*head, Xp.data_ptr(), Pp.data_ptr(), Ab.data_ptr(), *tail), "ac_ekf_filter_rec_f32")
                else:
                    _lib.check(lib.ac_ekf_filter_f32(*head, *tail), "ac_ekf_filter_f32")

            def smooth(initial, gains):
                p0 = (x.data_ptr(), P.data_ptr()) if initial else (None, None)
                s0 = (Xs0.data_ptr(), Ps0.data_ptr()) if initial else (None, None)
                _lib.check(lib.ac_ekf_smooth_f32(ac._handle, *p0, Xf.data_ptr(), Pf.data_ptr(), Xp.data_ptr(), Pp.data_ptr(), Ab.data_ptr(),
                                                 n, T, Xs.data_ptr(), Ps.data_ptr(), *s0, Cg.data_ptr() if gains else None,
                                                 sst.data_ptr(), ac._stream()), "ac_ekf_smooth_f32")

            filt(True)
            torch.cuda.synchronize()
            parts = {
                "filter": lambda: filt(False),
                "filter_rec": lambda: filt(True),
                "smooth": lambda: smooth(False, False),
                "smooth_gains": lambda: smooth(False, True),
                "smooth_initial": lambda: smooth(True, False),
            }
            parts = {k: parts[k] for k in args.parts.split(",")}
            rounds = {k: [] for k in parts}
            for _ in range(args.rounds):
                for k, fn in parts.items():
                    rounds[k].append(timed(torch, fn, args.window))
            ms = {k: float(np.median(v)) for k, v in rounds.items()}
            spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()}
            smooth(True, True)
            torch.cuda.synchronize()
            floor = {"smooth": floor_ms(n, T - 1, False), "smooth_gains": floor_ms(n, T - 1, True), "smooth_initial": floor_ms(n, T, False)}
            floor = {k: v for k, v in floor.items() if k in ms}
            both = "smooth" in ms and "filter" in ms
            print(json.dumps({
                "model": model, "n": n, "T": T, "ms": ms, "spread_over_rounds": spread, "trimmed": int(trim.converged.sum().item()),
                "filter_status_ok": int((fst == 0).all(dim=0).sum().item()), "smooth_status_ok": int((sst == 0).all(dim=0).sum().item()),
                "byte_floor_ms": floor, "over_byte_floor": {k: ms[k] / v for k, v in floor.items()},
                "smooth_over_filter": ms["smooth"] / ms["filter"] if both else None,
                "record_cost_over_filter": ms["filter_rec"] / ms["filter"] - 1 if "filter_rec" in ms and "filter" in ms else None,
                "smoothed_nodes_per_s": n * T / (ms["smooth"] * 1e-3) if "smooth" in ms else None,
                "trace_P_smoothed_over_filtered_node0": float((Ps[0].diagonal(dim1=0, dim2=1).sum(-1) / Pf[0].diagonal(dim1=0, dim2=1).sum(-1)).mean().item())}),
                flush=True)
            del ws, Xf, Xp, Xs, Pf, Pp, Ab, Ps, Cg, Z, U
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
