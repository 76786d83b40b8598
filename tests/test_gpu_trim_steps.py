"""The trim solver's LM iteration step by step on the device (ac_trim_f32, k_trim_assemble, k_trim_update,
aircraft_amd/csrc/ac_trim.hpp).

The workspace is the caller's and is re-initialised at the first iteration, so a call with iters = k on a fresh workspace leaves
in it the whole LM state after exactly k evaluations: the assembled candidate, the model's f, df/dx, df/du there and the 57
state words of every instance.  On the last iteration no new candidate is formed, so z_c of the iters = k + 1 call is
trim_step of the state the iters = k call stored.  tests/trim_ref.py restates the layout and holds the checks; the bars are
8 x e32, the error of the g++ build of ac_trim.hpp against float64 on identical inputs (tests/test_trim_steps_ref.py asserts
e32 <= 1.25e-5 for every case).  Every call: outputs and workspace in guarded buffers, the workspace exactly
ac_trim_workspace_floats(n) long and 3 floats past a 256-byte boundary, inputs bit-unchanged, n in {1, 63, 64, 65, 257}."""
import ctypes as C

import numpy as np
import pytest

from aircraft_amd import _lib
from tests import riccati_ref as rr
from tests import trim_ref as T
from tests.helpers import parity_report
from tests.test_gpu_riccati import NAN_BITS, PAD, assert_guards, bits_equal, dev, guarded
from tests.test_trim_steps_ref import CHAIN_CASES, EVAL_CASES, STEP_CASES, STEP_CASES_POINT0, ids, initial_snapshot, step_points

pytestmark = pytest.mark.gpu

FRONT = 64 + 3   # floats in front of the workspace: a 256-byte boundary and 3 more


def run(c, gpu, tg, uh, z0, iters, finite=True):
    """One ac_trim_f32 call -> snapshot (numpy) plus the device views Xw, Uw, Xd, Fx, Fu of the workspace."""
    import torch

    lib = _lib.load()
    c.ac._sync()
    n = tg.shape[1]
    need = C.c_size_t()
    assert lib.ac_trim_workspace_floats(c.ac._handle, n, C.byref(need)) == 0 and need.value == n * T.WS_FLOATS + T.WS_PAD
    inp = dict(tg=dev(tg, gpu), uh=dev(uh, gpu), z0=dev(z0, gpu))
    before = {k: v.clone() for k, v in inp.items()}
    out = {k: guarded(s, gpu) for k, s in dict(Xo=(13, n), Uo=(7, n), Z=(6, n), R=(6, n), S=(n,)).items()}
    wbuf = torch.full((FRONT + need.value + PAD,), NAN_BITS, dtype=torch.int32, device=gpu).view(torch.float32)
    ws = wbuf[FRONT:FRONT + need.value]
    assert wbuf.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 12
    off, end = T.ws_layout(ws.data_ptr(), n)
    assert end <= need.value
    o = T.trim_opts(c.lateral, c.lo, c.hi, c.tol)
    rc = lib.ac_trim_f32(c.ac._handle, C.byref(o), inp["tg"].data_ptr(), inp["uh"].data_ptr(), inp["z0"].data_ptr(), int(iters), n,
                         *[out[k][1].data_ptr() for k in ("Xo", "Uo", "Z", "R", "S")], ws.data_ptr(), need.value, None)
    assert rc == 0
    torch.cuda.synchronize()
    for k, v in inp.items():
        assert bits_equal(v, before[k]), ("input changed", k)
    S = out.pop("S")
    sbits = S[0].view(torch.int32)
    assert bool((sbits[:PAD] == NAN_BITS).all()) and bool((sbits[-PAD:] == NAN_BITS).all()), "status: padding overwritten"
    if finite:
        assert_guards(out, "trim outputs")
    else:   # planted non-finite instances: NaN is a legitimate output there, the padding is still checked
        for k, (buf, _) in out.items():
            b = buf.view(torch.int32)
            assert bool((b[:PAD] == NAN_BITS).all()) and bool((b[-PAD:] == NAN_BITS).all()), (k, "padding overwritten")
    # the workspace: nothing written in front of it, behind it, or between its six arrays
    wbits = wbuf.view(torch.int32)
    used = torch.zeros(wbuf.numel(), dtype=torch.bool, device=gpu)
    view = {}
    for name, rows in T.WS_ROWS:
        a = FRONT + off[name]
        used[a:a + rows * n] = True
        view[name] = wbuf[a:a + rows * n].view(rows, n)
    assert bool((wbits[~used] == NAN_BITS).all()), "the workspace was written outside its six arrays"
    snap = {k: v[1].cpu().numpy() for k, v in out.items()}
    snap["S"] = S[1].view(torch.int32).cpu().numpy()
    snap.update(X=view["X"].cpu().numpy(), U=view["U"].cpu().numpy(), Xd=view["Xd"].cpu().numpy(),
                Fx=view["Fx"].cpu().numpy().reshape(13, 13, n), Fu=view["Fu"].cpu().numpy().reshape(13, 7, n),
                st=view["St"].cpu().numpy())
    return snap, view


_RUNS = {}


def run_pool(c, gpu, points, n, iters):
    """the call on n columns of the case's pool of starting points (cached: the step test reuses the evaluation's call)"""
    key = (c.name, c.lateral, points, n, iters)
    if key not in _RUNS:
        tg, uh, z0, pt = c.pool(points)
        col = T.columns(tg.shape[1], n, offset=7 * n)
        _RUNS[key] = (tg[:, col], uh[:, col], z0[:, col], np.asarray(pt)[col]) + run(c, gpu, tg[:, col], uh[:, col], z0[:, col], iters)
    return _RUNS[key]


# ---- a. one evaluation from prescribed points ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,lateral", EVAL_CASES, ids=ids(EVAL_CASES))
def test_one_evaluation(gpu, model, lateral):
    c = T.case(model, lateral)
    er, eJ = c.e32_chain()
    assert er <= rr.E32_MAX and eJ <= rr.E32_MAX
    worst = dict(r=0.0, J=0.0, cost_ulp=0.0, v=0.0, q=0.0, w=0.0, status1=0, status2=0, converged=0)
    for n in T.SIZES:
        tg, uh, z0, _, snap, view = run_pool(c, gpu, T.POINTS, n, 1)
        Xd, Fx, Fu = c.ac.state_derivative_sens(view["X"].clone(), view["U"].clone())
        assert bits_equal(Xd, view["Xd"]) and bits_equal(Fx.reshape(169, n), view["Fx"]) and bits_equal(Fu.reshape(91, n), view["Fu"]), \
            "the workspace holds the model's own f, df/dx, df/du at the assembled candidate"
        fig = T.check_evaluation(snap, tg, uh, z0, lateral, c.lo, c.hi, c.tol, rr.FACTOR * er, rr.FACTOR * eJ)
        print(f"[trim steps] {model} {lateral} n={n}: r {fig['r']:.2e} / {fig['bar_r']:.2e}  J {fig['J']:.2e} / {fig['bar_J']:.2e}  "
              f"cost {fig['cost_ulp']:.2f} ulp  v {fig['v']:.1e} q {fig['q']:.1e} w {fig['w']:.1e}  status 0/1/2: "
              f"{fig['converged']}/{fig['status1']}/{fig['status2']}  decisive {fig['decisive']:.1e}")
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    parity_report("trim_one_evaluation", model=model, lateral=lateral, e32_r=er, e32_J=eJ, bar_r=rr.FACTOR * er, bar_J=rr.FACTOR * eJ,
                  **worst)
    assert worst["status2"] > 0


# ---- b. one step ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,lateral", STEP_CASES + STEP_CASES_POINT0, ids=ids(STEP_CASES + STEP_CASES_POINT0))
def test_one_step(gpu, model, lateral):
    c = T.case(model, lateral)
    points = step_points(model)
    e32 = {k: c.e32_step_point(k) for k in points}
    assert all(v <= rr.E32_MAX for v in e32.values())
    worst, clipped = 0.0, 0
    for n in T.SIZES:
        *_, pt, one, _ = run_pool(c, gpu, points, n, 1)
        *_, two, _ = run_pool(c, gpu, points, n, 2)
        bar = rr.FACTOR * np.array([e32[k] for k in pt])
        w, cl = T.check_step(one, two, c.lo, c.hi, c.tol, bar)
        print(f"[trim steps] {model} {lateral} n={n}: step {w:.2e} / {bar.max():.2e}, {cl} clipped components")
        worst, clipped = max(worst, w), clipped + cl
    parity_report("trim_one_step", model=model, lateral=lateral, e32=e32, bar=rr.FACTOR * max(e32.values()), worst=worst, clipped=clipped)
    assert clipped > 0


# ---- c. the chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,lateral", CHAIN_CASES, ids=ids(CHAIN_CASES))
def test_chain(gpu, model, lateral):
    c = T.case(model, lateral)
    e_r, e_z = c.e32_chain()[0], c.e32_step_chain()
    assert e_r <= rr.E32_MAX and e_z <= rr.E32_MAX
    total = dict(accept=0, reject=0, freeze=0, undecided=0, status1=0, status2=0)
    worst, lams = 0.0, set()
    for n in T.SIZES:
        col = T.columns(c.tg.shape[1], n, offset=5 * n)
        tg, uh, z0 = c.tg[:, col], c.uh[:, col], c.z0[:, col]
        snaps = [initial_snapshot(z0, c.lo, c.hi)] + [run(c, gpu, tg, uh, z0, k)[0] for k in range(1, T.K + 1)]
        for k in range(T.K):
            cnt = T.check_transition(snaps[k], snaps[k + 1], tg, lateral, c.tol, rr.FACTOR * e_r)
            for key, v in cnt.items():
                if key in total:
                    total[key] += v
            if k:
                worst = max(worst, T.check_step(snaps[k], snaps[k + 1], c.lo, c.hi, c.tol, rr.FACTOR * e_z)[0])
            lams |= {float(v) for v in T.unpack(snaps[k + 1]["st"])["lam"]}
        s1, s2, dec = T.check_last_status(snaps[-1], c.lo, c.hi, c.tol)
        total["status1"] += s1
        total["status2"] += s2
        print(f"[trim steps] chain {model} {lateral} n={n}: step {worst:.2e} / {rr.FACTOR * e_z:.2e}, status 1 x {s1}, 2 x {s2}, "
              f"decisive {dec:.1e}, so far {total}")
    parity_report("trim_chain", model=model, lateral=lateral, e32_step=e_z, bar=rr.FACTOR * e_z, worst=worst, lambdas=len(lams), **total)
    assert total["accept"] and total["reject"] and total["freeze"] and total["status2"] and len(lams) >= 4


# ---- d. non-finite instances, and the independence of the others ---------------------------------------------------------------------
@pytest.mark.parametrize("model", ["poly", "net_3x64_valu"])
def test_non_finite_instances_and_independence(gpu, model):
    c = T.case(model, 0)
    n, iters = 65, 6
    col = T.columns(c.tg.shape[1], n, offset=11)
    good = (c.tg[:, col], c.uh[:, col], c.z0[:, col])
    tg, uh, z0 = (a.copy() for a in good)
    bad = dict(v_zero=3, v_nan=17, z_nan=40, v_huge=64)
    tg[3, bad["v_zero"]] = 0.0
    tg[3, bad["v_nan"]] = np.nan
    z0[1, bad["z_nan"]] = np.nan
    tg[3, bad["v_huge"]] = 3.0e38
    z0[0, bad["v_huge"]], z0[4, bad["v_huge"]] = 1.0, -25.0   # outside the bounds: the usable input is clipped
    z0[2, bad["v_zero"]] = 7.0                                # outside the bounds: an unusable input is returned as given
    ref, _ = run(c, gpu, *good, iters)
    got, _ = run(c, gpu, tg, uh, z0, iters, finite=False)
    idx = np.array(sorted(bad.values()))
    assert (got["S"][idx] == 3).all(), got["S"][idx]
    assert np.isnan(got["R"][:, idx]).all()
    want = T.c32(z0)[:, idx].copy()
    j = list(idx).index(bad["v_huge"])
    want[:, j] = np.clip(want[:, j], T.c32(c.lo), T.c32(c.hi))
    assert T.same_bits(got["Z"][:, idx], want), "Z is z0 as given (clipped where the inputs were usable)"
    flag = T.unpack(got["st"])["flag"]
    assert (flag[idx] == 3).all()
    rest = np.setdiff1d(np.arange(n), idx)
    for k in ("Xo", "Uo", "Z", "R", "st", "X", "U", "Xd", "Fx", "Fu"):
        assert T.same_bits(got[k][..., rest], ref[k][..., rest]), ("a bad instance moved its neighbours", k)
    assert np.array_equal(got["S"][rest], ref["S"][rest])
    assert np.isfinite(got["Z"][:, rest]).all() and np.isfinite(got["R"][:, rest]).all()
    parity_report("trim_non_finite", model=model, planted=len(idx), status=got["S"][idx].tolist(), others_bit_equal=True,
                  others_status=np.bincount(ref["S"], minlength=4).tolist())
