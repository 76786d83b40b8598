#!/usr/bin/env python3
"""Times ac_modes_f32 and ac_eig_f32 per model, batch size, coordinate selection and loop, and appends
one JSON line each to profiles/modes_bench.jsonl.  (tools/bench_modes.py is an older tool: the modes of the hot path.)

    python tools/bench_flight_modes.py                       # n = 4096 and 65 536; cubic fits and default model
    python tools/bench_flight_modes.py --sizes 4096 --models poly

Every part is a raw ABI call on preallocated buffers, warmed up, then timed with device events around a window of repeated
launches at least --window seconds long; the median of --rounds rounds is reported with the spread.  k_modes_eig is not
callable alone: its time is the whole ac_modes_f32 call minus the handle's step-sensitivity launch and minus the
projection, both timed in the same run (the projection as ac_lqr_f32 with one doubling step minus the sensitivity launch
and one doubling step, which still holds the gain solve: an upper bound on the projection, so a lower bound on
k_modes_eig).  ac_eig_f32 on the same matrices (k_eig: the same unit without the assembly) is timed directly.  For context
only: ac_lqr_f32 on the same n, numpy eigvals on the host, torch.linalg.eigvals on the device tensors (null if it raises).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.bench_mppi import timed  # noqa: E402

COORDS = {"flight": 0xEF8, "all": 0xFFF}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=str, default="4096,65536")
    ap.add_argument("--models", type=str, default="poly,default")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of repeated launches per timing")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "modes_bench.jsonl"))
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_flight_modes.py needs the GPU: there is nothing to time without it")
    from aircraft_amd import _lib
    from aircraft_amd.build import source_sha
    from examples.glide_polar import make

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    sha = source_sha()
    out = open(args.out, "a")
    for model in args.models.split(","):
        ac = make(model)
        for n in (int(s) for s in args.sizes.split(",")):
            rng = np.random.default_rng(0)
            V = torch.tensor(rng.uniform(30, 60, n), dtype=torch.float32, device=dev)
            psid = torch.tensor(rng.uniform(-0.1, 0.1, n), dtype=torch.float32, device=dev)
            trim = ac.trim(V, turn_rate=psid)
            x, u = trim.x.contiguous(), trim.u.contiguous()
            q12 = [1.0] * 12
            lws = ac.lqr_workspace(n)
            design = ac.lqr((x, u), 0.01, q=q12, ws=lws)
            K = design.K.contiguous()
            ws = ac.modes_workspace(n)
            f32 = dict(device=dev, dtype=torch.float32)
            w = torch.empty((4, 12, n), **f32)
            S, it = torch.empty(n, device=dev, dtype=torch.int32), torch.empty(n, device=dev, dtype=torch.int32)
            A, B, P, Ko, res = (torch.empty(s, **f32) for s in ((12, 12, n), (12, 7, n), (12, 12, n), (7, 12, n), (n,)))
            sens_out = tuple(torch.empty(s, **f32) for s in ((13, n), (13, 13, n), (13, 7, n))) + (None,)
            lo = _lib.LqrOpts()
            lo.q[:], lo.r[:], lo.tol = q12, [1.0] * 7, 1e-6
            h, st = ac._handle, ac._stream()

            def modes(coords, k):
                o = _lib.ModesOpts()
                o.coords, o.max_iters = coords, 0
                return lambda: _lib.check(lib.ac_modes_f32(h, C.byref(o), x.data_ptr(), u.data_ptr(), C.c_float(0.01), k, n, None, None,
                                                           w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(),
                                                           S.data_ptr(), it.data_ptr(), ws.data_ptr(), ws.numel(), st))

            def lqr(iters):
                return lambda: _lib.check(lib.ac_lqr_f32(h, C.byref(lo), x.data_ptr(), u.data_ptr(), C.c_float(0.01), iters, n,
                                                         A.data_ptr(), B.data_ptr(), P.data_ptr(), Ko.data_ptr(), res.data_ptr(),
                                                         S.data_ptr(), it.data_ptr(), lws.data_ptr(), lws.numel(), st))

            def measure(parts):
                rounds = {k: [] for k in parts}
                for _ in range(args.rounds):
                    for k, fn in parts.items():
                        rounds[k].append(timed(torch, fn, args.window))
                return ({k: float(np.median(v)) for k, v in rounds.items()},
                        {k: float((max(v) - min(v)) / np.median(v)) for k, v in rounds.items()})

            # the parent commit's parts, once per model and size
            common = measure({"step_sens": lambda: ac.step_sens(x, u, 0.01, want_c=False, out=sens_out), "lqr": lqr(24),
                              "lqr_iters1": lqr(1)})
            for cname, coords in COORDS.items():
                m = bin(coords).count("1")
                idx = [i for i in range(12) if (coords >> i) & 1]
                for loop in ("open", "closed"):
                    kptr = K.data_ptr() if loop == "closed" else None
                    run = modes(coords, kptr)
                    run()
                    torch.cuda.synchronize()
                    iters = it.cpu().numpy().astype(np.float64) / m
                    status = S.cpu().numpy()
                    # the matrices k_modes_eig sees, for ac_eig_f32 and the host / torch yardsticks
                    r = ac.modes((x, u), 0.01, gains=K if loop == "closed" else None, coords=idx)
                    Mx = r.A.clone()
                    Mx[torch.tensor([3, 4, 5, 6, 7, 9, 10, 11])[:, None], torch.tensor([0, 1, 2, 8])[None, :]] = 0
                    if loop == "closed":
                        Mx = Mx - torch.einsum("ijn,jkn->ikn", r.B, K)
                    Mx = Mx[idx][:, idx].contiguous()
                    ew = torch.empty((2, m, n), **f32)
                    ms, spread = measure({"modes": run, "eig": lambda: _lib.check(lib.ac_eig_f32(
                        h, Mx.data_ptr(), m, 0, n, ew[0].data_ptr(), ew[1].data_ptr(), S.data_ptr(), it.data_ptr(), st))})
                    ms.update(common[0])
                    spread.update(common[1])
                    per_iter = (ms["lqr"] - ms["lqr_iters1"]) / 23
                    proj = ms["lqr_iters1"] - ms["step_sens"] - per_iter
                    # context: the host and torch
                    sub = min(n, 4096)
                    Mh = torch.nan_to_num(Mx[:, :, :sub].permute(2, 0, 1)).contiguous()  # (a design that broke down leaves NaN gains)
                    t0 = time.perf_counter()
                    np.linalg.eigvals(Mh.cpu().numpy())
                    numpy_ms = (time.perf_counter() - t0) * 1e3 * n / sub
                    try:
                        torch.linalg.eigvals(Mh)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        torch.linalg.eigvals(Mh)
                        torch.cuda.synchronize()
                        torch_ms = (time.perf_counter() - t0) * 1e3 * n / sub
                    except Exception:  # noqa: BLE001 (recorded as null: it is context, not a result)
                        torch_ms = None
                    line = {"model": model, "n": n, "coords": cname, "m": m, "loop": loop, "build": sha, "ms": ms,
                            "spread_over_rounds": spread, "projection_and_gain_upper_ms": proj,
                            "k_modes_eig_by_difference_ms": ms["modes"] - ms["step_sens"] - proj,
                            "k_eig_direct_ms": ms["eig"], "instances_per_s": n / (ms["modes"] * 1e-3),
                            "qr_iterations_per_eigenvalue": {"mean": float(iters.mean()), "max": float(iters.max())},
                            "status_counts": {str(k): int((status == k).sum()) for k in np.unique(status)},
                            "trimmed": int(trim.converged.sum().item()),
                            "context": {"lqr_ms": ms["lqr"], "numpy_eigvals_host_ms_scaled_from": sub, "numpy_eigvals_host_ms": numpy_ms,
                                        "torch_linalg_eigvals_ms": torch_ms},
                            "k_modes_eig_slower_than_lqr": bool(ms["modes"] - ms["step_sens"] - proj > ms["lqr"])}
                    print(json.dumps(line), flush=True)
                    out.write(json.dumps(line) + "\n")
                    out.flush()
            del ws, lws, w, A, B, P, Ko, sens_out
            torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
