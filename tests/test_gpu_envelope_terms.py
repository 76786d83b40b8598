"""The flight-envelope kernels row by row, side by side and node by node against the float64 oracle (tests/envelope_ref.py
states the metric, the bar rule and the one exception): k_envelope, k_envelope_cost, k_envelope_model and
k_envelope_multipliers (csrc/ac_kernels_analytic.hpp) through their seven ABI entries.

Inputs are synthetic and fp32-exact: the kernels only read arrays (and epsilon from the handle), no dynamics kernel runs.
Every output is a view into a NaN-filled buffer whose padding must stay bit-unchanged and whose inside must be finite; every
input must be bit-unchanged; a repeat of every call must be bit-identical.  The e32 condition is asserted (bar_of) before a
GPU number is compared.

The q group of the speed row - its gradient, its vq / qq curvature blocks and d|v_rel|^2 / dq of k_envelope - is held to
8 x e32 of the row's v group on the row's v scale (DESIGN.md section 5 quotes the measured figures)."""
import ctypes as C

import numpy as np
import pytest

import ilqr_oracle as io
from tests import envelope_ref as er
from tests.helpers import f32_exact, make_aircraft, parity_report
from tests.test_gpu_riccati import assert_guards, bits_equal, dev, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ac(gpu):
    return er._aircraft()


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def host(t):
    return t.cpu().numpy().astype(np.float64)


def pen(lo, hi, w=er.W):
    from aircraft_amd import _lib

    p = _lib.EnvelopePenalty()
    p.lo[:] = [float(v) for v in lo]; p.hi[:] = [float(v) for v in hi]; p.weight = float(w)
    return p


class Inputs:
    """device copies of named host arrays (None stays None); unchanged() asserts that no kernel wrote to them"""

    def __init__(self, gpu, **arrays):
        self.t = {k: (None if v is None else dev(v, gpu)) for k, v in arrays.items()}
        self.before = {k: (None if v is None else v.clone()) for k, v in self.t.items()}

    def __getitem__(self, k):
        return self.t[k]

    def unchanged(self):
        for k, v in self.before.items():
            assert v is None or bits_equal(self.t[k], v), (k, "input modified")


def launched(ac, name, n):
    assert ac.last_launch()[:3] == (name, (n + 255) // 256, 256), ac.last_launch()


def summary(out):
    return "  ".join(f"{k} {w:.1e}/{e:.1e}" for k, (w, e) in out.items())


# ---- k_envelope: rows and Jx --------------------------------------------------------------------------------------------------------
def check_rows(name, rows, Jx, c, nodes):
    ref_r, ref_J = c["rows"][:nodes], c["Jx"][:nodes]
    e32_r = er.rows_err(c["rows32"][:nodes], ref_r)
    e32_J = er.jx_err(c["Jx32"][:nodes], ref_J)
    bars_r = [er.bar_of(float(e), f"{name}:rows:{er.ROWS[r]}") for r, e in enumerate(e32_r)]
    e32_J[("speed", "q")] = e32_J[("speed", "v")]              # the exception: held to the v group's bar on the v scale
    bars_J = {k: er.bar_of(v, f"{name}:Jx:{k}") for k, v in e32_J.items()}
    got_r, got_J = er.rows_err(rows, ref_r), er.jx_err(Jx, ref_J)
    n = rows.shape[-1]
    assert np.array_equal(rows[:, 3], ref_r[:, 3, :n]) and er.zeros_kept(Jx, ref_J[..., :n])
    rep = {er.ROWS[r]: dict(worst=float(got_r[r]), e32=float(e32_r[r])) for r in range(4)}
    rep.update({f"Jx.{k[0]}.{k[1]}": dict(worst=got_J[k], e32=e32_J[k]) for k in got_J if e32_J[k] or got_J[k]})
    parity_report(name, **rep)
    print(name, "  ".join(f"{k} {v['worst']:.1e}/{v['e32']:.1e}" for k, v in rep.items()))
    for r in range(4):
        assert got_r[r] <= bars_r[r], (name, er.ROWS[r], got_r[r], "beyond", bars_r[r])
    for k in got_J:
        assert got_J[k] <= bars_J[k], (name, "Jx", k, got_J[k], "beyond", bars_J[k])


@pytest.mark.parametrize("n", er.ROWS_N)
def test_envelope_rows_unit_by_unit(gpu, ac, n):
    """ac_envelope_f32 on the leading n units (node-major) of the 8-node parent batch: one lane per unit, n around one and two
    blocks; Jx NULL gives the same rows bit for bit"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    c = er.parent(7)
    flat = lambda a: np.ascontiguousarray(np.moveaxis(a, 0, -2).reshape(a.shape[1:-1] + (-1,)))  # noqa: E731  (N, r, B) -> (r, N B)
    Xu = flat(c["X"])[:, :n]
    inp = Inputs(gpu, X=Xu)
    runs = []
    for with_jx in (True, True, False):
        bufs = {"rows": guarded((4, n), gpu)}
        if with_jx:
            bufs["Jx"] = guarded((4, 13, n), gpu)
        _lib.check(lib.ac_envelope_f32(ac._handle, ptr(inp["X"]), n, ptr(bufs["rows"][1]), ptr(bufs["Jx"][1] if with_jx else None),
                                       ac._stream()), "ac_envelope_f32")
        torch.cuda.synchronize()
        launched(ac, "k_envelope", n)
        assert_guards(bufs, "envelope")
        runs.append(bufs)
    inp.unchanged()
    assert bits_equal(runs[0]["rows"][1], runs[1]["rows"][1]) and bits_equal(runs[0]["Jx"][1], runs[1]["Jx"][1]), "a repeat differs"
    assert bits_equal(runs[0]["rows"][1], runs[2]["rows"][1]), "Jx = NULL changes the rows"
    wide = dict(rows=flat(c["rows"])[None], Jx=flat(c["Jx"])[None], rows32=flat(c["rows32"])[None], Jx32=flat(c["Jx32"])[None])
    check_rows(f"envelope_rows[n{n}]", host(runs[0]["rows"][1])[None], host(runs[0]["Jx"][1])[None], wide, 1)


def test_envelope_rows_shooting_form(gpu, ac):
    """ac_shoot_envelope_f32 on B H = 37 x 7 nodes in the rollout layout (7, 13, 37)"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    c = er.parent(7)
    B, H = 37, 7
    inp = Inputs(gpu, X=np.ascontiguousarray(c["X"][:H, :, :B]))
    runs = []
    for _ in range(2):
        bufs = {"rows": guarded((H, 4, B), gpu), "Jx": guarded((H, 4, 13, B), gpu)}
        _lib.check(lib.ac_shoot_envelope_f32(ac._handle, ptr(inp["X"]), B, H, ptr(bufs["rows"][1]), ptr(bufs["Jx"][1]), ac._stream()),
                   "ac_shoot_envelope_f32")
        torch.cuda.synchronize()
        launched(ac, "k_envelope", B * H)
        assert_guards(bufs, "shoot_envelope")
        runs.append(bufs)
    inp.unchanged()
    assert all(bits_equal(runs[0][k][1], runs[1][k][1]) for k in runs[0])
    check_rows("envelope_rows[shoot-37x7]", host(runs[0]["rows"][1]), host(runs[0]["Jx"][1]), c, H)


# ---- k_envelope_cost ------------------------------------------------------------------------------------------------------------------
def cost_call(ac, gpu, p, inp, lam, Bl, pre):
    """cost = pre, then the kernel adds to it -> host copy of the guarded view; twice, bit-identical.  lam None goes through
    ac_envelope_cost_f32 (the penalty entry), a tensor through ac_envelope_al_cost_f32."""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    X = inp["X"]
    H, B = X.shape[0] - 1, X.shape[2]
    runs = []
    for _ in range(2):
        buf = {"cost": guarded((B,), gpu)}
        buf["cost"][1].copy_(dev(pre, gpu))
        if lam is None:
            _lib.check(lib.ac_envelope_cost_f32(ac._handle, C.byref(p), ptr(X), B, H, ptr(buf["cost"][1]), ac._stream()), "ac_envelope_cost_f32")
        else:
            _lib.check(lib.ac_envelope_al_cost_f32(ac._handle, C.byref(p), ptr(lam), Bl, ptr(X), B, H, ptr(buf["cost"][1]), ac._stream()),
                       "ac_envelope_al_cost_f32")
        torch.cuda.synchronize()
        launched(ac, "k_envelope_cost", B)
        assert_guards(buf, "envelope_cost")
        runs.append(buf["cost"][1])
    assert bits_equal(*runs), "a repeat of the call differs"
    inp.unchanged()
    return runs[0].cpu().numpy()


def cost_runs(name, ac, gpu, c, cols, Bl, forms, aux=None):
    """every run of er.COST_RUNS in the given forms on the leading `cols` columns of case c (multipliers: its leading Bl
    columns); e32 over all of c and, where given, over aux as well"""
    import torch

    X = np.ascontiguousarray(c["X"][:, :, :cols])
    out = {}
    for lam_on in forms:
        for label, row, side in er.COST_RUNS:
            ref = er.reference(c, row, side, lam_on)
            e32 = float(er.term_err(er.restated(c, row, side, lam_on)["cost"], ref["cost"], ref["S_abs"]).max())
            if aux is not None:
                ra = er.reference(aux, row, side, lam_on)
                e32 = max(e32, float(er.term_err(er.restated(aux, row, side, lam_on)["cost"], ra["cost"], ra["S_abs"]).max()))
            key = f"{label}{'' if lam_on else '(penalty)'}"
            bar = er.bar_of(e32, f"{name}:{key}")
            lam = np.ascontiguousarray(ref["lam"][:, :, :Bl]) if lam_on else None
            inp = Inputs(gpu, X=X, lam=lam)
            p = pen(ref["lo"], ref["hi"])
            got = cost_call(ac, gpu, p, inp, inp["lam"], Bl, np.zeros(cols))
            e = er.term_err(got, ref["cost"][:cols], ref["S_abs"][:cols])
            out[key] = (float(e.max()), e32)
            assert (e <= bar).all(), (name, key, "beyond", bar, "at instances", np.flatnonzero(e > bar)[:8].tolist(), "worst", float(e.max()))
            if not lam_on:        # multipliers all zero = multipliers NULL, bit for bit
                zin = Inputs(gpu, X=X, lam=np.zeros((X.shape[0], 8, Bl)))
                assert np.array_equal(cost_call(ac, gpu, p, zin, zin["lam"], Bl, np.zeros(cols)).view(np.int32), got.view(np.int32)), (key, "lam = 0 differs from lam = NULL")
            if label == "all":    # the kernel adds to what is there: within one fp32 ulp of p + J (the multiply may be fused into the add)
                pre = np.float32(np.random.default_rng(5).uniform(-0.5, 0.5, cols) * ref["S_abs"][:cols])
                got2 = cost_call(ac, gpu, p, inp, inp["lam"], Bl, pre)
                want = pre + got
                assert (np.abs(got2.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all(), (name, key, "cost += J")
    parity_report(name, **{k: dict(worst=w, e32=e, ratio=(w / e if e > 0 else 0.0)) for k, (w, e) in out.items()})
    print(name, summary(out))
    torch.cuda.synchronize()


@pytest.mark.parametrize("H", er.COST_H)
@pytest.mark.parametrize("B", er.COST_B)
def test_envelope_cost_row_by_row(gpu, ac, B, H):
    """ac_envelope_cost_f32 / ac_envelope_al_cost_f32: each row x {upper, lower, both} sides, then all rows, in the penalty and the
    augmented-Lagrangian form; one lane per instance, B = 257 crosses a block"""
    cost_runs(f"envelope_terms[B{B}-H{H}]", ac, gpu, er.parent(H), B, B, (True, False))


@pytest.mark.parametrize("H", er.COST_H)
@pytest.mark.parametrize("Bl", er.COST_BL)
def test_envelope_cost_candidate_batches(gpu, ac, Bl, H):
    """a line-search batch of 3 Bl columns that share Bl instances' multipliers: column o reads instance o % Bl (258 columns
    cross a block)"""
    cost_runs(f"envelope_terms[Bl{Bl}x3-H{H}]", ac, gpu, er.candidates(Bl, H), er.REPS * Bl, Bl, (True,), aux=er.parent(H))


def test_envelope_cost_columns_are_independent(gpu, ac):
    """columns 16:37 of a B = 37 call are bit-identical as a call of their own"""
    c = er.parent(3)
    ref = er.reference(c)
    p = pen(ref["lo"], ref["hi"])
    whole = Inputs(gpu, X=np.ascontiguousarray(c["X"][:, :, :37]), lam=np.ascontiguousarray(c["lam"][:, :, :37]))
    part = Inputs(gpu, X=np.ascontiguousarray(c["X"][:, :, 16:37]), lam=np.ascontiguousarray(c["lam"][:, :, 16:37]))
    a = cost_call(ac, gpu, p, whole, whole["lam"], 37, np.zeros(37))
    b = cost_call(ac, gpu, p, part, part["lam"], 21, np.zeros(21))
    assert np.array_equal(a[16:].view(np.int32), b.view(np.int32))


# ---- k_envelope_model -------------------------------------------------------------------------------------------------------------------
def model_call(ac, gpu, p, inp, lam, pre_g, pre_h, want=("glin", "Hz")):
    """glin = pre_g (H+1, 13, B) and Hz = pre_h (H+1, 21, 21, B: one node more than the kernel may touch), then the kernel adds;
    twice, bit-identical -> {name: device view}"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    X = inp["X"]
    H, B = X.shape[0] - 1, X.shape[2]
    runs = []
    for _ in range(2):
        bufs = {}
        if "glin" in want:
            bufs["glin"] = guarded((H + 1, 13, B), gpu); bufs["glin"][1].copy_(dev(pre_g, gpu))
        if "Hz" in want:
            bufs["Hz"] = guarded((H + 1, 21, 21, B), gpu); bufs["Hz"][1].copy_(dev(pre_h, gpu))
        args = (ptr(bufs["glin"][1] if "glin" in want else None), ptr(bufs["Hz"][1] if "Hz" in want else None), ac._stream())
        if lam is None:
            _lib.check(lib.ac_envelope_model_f32(ac._handle, C.byref(p), ptr(X), B, H, *args), "ac_envelope_model_f32")
        else:
            _lib.check(lib.ac_envelope_al_model_f32(ac._handle, C.byref(p), ptr(lam), ptr(X), B, H, *args), "ac_envelope_al_model_f32")
        torch.cuda.synchronize()
        launched(ac, "k_envelope_model", (H + 1) * B)
        assert_guards(bufs, "envelope_model")
        runs.append({k: v[1] for k, v in bufs.items()})
    for k in runs[0]:
        assert bits_equal(runs[0][k], runs[1][k]), (k, "a repeat of the call differs")
    inp.unchanged()
    return runs[0]


def model_prefill(ref, H, rng):
    """arbitrary fp32 tensors for glin (H+1, 13, PB) and Hz (H+1, 21, 21, PB): O(30) wherever the reference adds nothing,
    within half the metric's denominator where it adds (the sum is compared on the scale of the increments)"""
    PB = ref["grad"].shape[-1]
    pre_g = rng.normal(0, 30, (H + 1, 13, PB))
    for g, den in er.grad_den(ref["grad"]).items():
        sl = er.GROUPS[g]
        u = rng.uniform(-0.5, 0.5, pre_g[:, sl].shape)
        pre_g[:, sl] = np.where(den[:, None] > 0, u * den[:, None], pre_g[:, sl])
    pre_h = rng.normal(0, 30, (H + 1, 21, 21, PB))
    for pr, den in er.curv_den(ref["curv"][:H]).items():
        sa, sb = er.PAIRS[pr]
        for a, b in ((sa, sb), (sb, sa)):
            u = rng.uniform(-0.5, 0.5, pre_h[:H, a, b].shape)
            pre_h[:H, a, b] = np.where(den[:, None, None] > 0, u * den[:, None, None], pre_h[:H, a, b])
    return f32_exact(pre_g), f32_exact(pre_h)


@pytest.mark.parametrize("B,H", er.MODEL_SHAPES)
def test_envelope_model_node_by_node(gpu, ac, B, H):
    """ac_envelope_model_f32 / ac_envelope_al_model_f32, one lane per (node, instance), per row and with all rows: the gradient
    is ADDED to a pre-filled glin, the curvature to the (x, x) block of a pre-filled Hz at the nodes k < H only; whatever the
    reference leaves alone stays bit-unchanged; the height row is exact"""
    c = er.parent(H)
    rng = np.random.default_rng(17)
    X = np.ascontiguousarray(c["X"][:, :, :B])
    for lam_on in (True, False):
        for label, row, side in er.MODEL_RUNS:
            name = f"envelope_model[B{B}-H{H}-{label}{'' if lam_on else '-penalty'}]"
            ref, f32 = er.reference(c, row, side, lam_on), er.restated(c, row, side, lam_on)
            pre_g, pre_h = model_prefill(ref, H, rng)
            ref_g, ref_c = ref["grad"].sum(axis=1), ref["curv"][:H].sum(axis=1)
            g32 = (np.float32(pre_g) + f32["grad"]).astype(np.float64)
            h32 = np.float32(pre_h[:H, :13, :13])
            for r in range(4):
                h32 = h32 + f32["curv_rows"][:H, r]
            inp = Inputs(gpu, X=X, lam=np.ascontiguousarray(ref["lam"][:, :, :B]) if lam_on else None)
            p = pen(ref["lo"], ref["hi"])
            out = model_call(ac, gpu, p, inp, inp["lam"], pre_g[..., :B], pre_h[..., :B])
            gl, Hz = out["glin"].cpu().numpy(), out["Hz"].cpu().numpy()
            pg, ph = np.float32(pre_g[..., :B]), np.float32(pre_h[..., :B])
            # what the reference leaves alone is bit-unchanged: the terminal node of Hz, its rows and columns 13..20, every entry
            # of its (x, x) block and of glin that no row reaches
            keep = np.ones(Hz.shape, bool); keep[:H, :13, :13] = ref_c[..., :B] == 0
            assert np.array_equal(Hz.view(np.int32)[keep], ph.view(np.int32)[keep]), (name, "Hz changed where the reference adds nothing")
            keep_g = ref_g[..., :B] == 0
            assert np.array_equal(gl.view(np.int32)[keep_g], pg.view(np.int32)[keep_g]), (name, "glin changed where the reference adds nothing")
            assert (ref_c[:, [0, 1] + list(range(10, 13))] == 0).all() and (ref_g[:, 10:13] == 0).all() and (ref_g[:, :2] == 0).all()
            # the height row, bit for bit: 2 w viol at row 2, 2 w active at (2, 2)
            zg = np.float32(2 * er.W * (np.maximum(0.0, ref["up"][:, 3]) - np.maximum(0.0, ref["dn"][:, 3])))[:, :B]
            assert np.array_equal((pg[:, 2] + zg).view(np.int32)[zg != 0], gl[:, 2].view(np.int32)[zg != 0]), (name, "height row of the gradient")
            zc = np.float32(2 * er.W * ((ref["up"][:H, 3] > 0).astype(float) + (ref["dn"][:H, 3] > 0)))[:, :B]
            assert np.array_equal((ph[:H, 2, 2] + zc).view(np.int32), Hz[:H, 2, 2].view(np.int32)), (name, "entry (2, 2) of the curvature")
            d_g = gl.astype(np.float64) - pre_g[..., :B] - ref_g[..., :B]
            d_h = Hz[:H, :13, :13].astype(np.float64) - pre_h[:H, :13, :13, :B] - ref_c[..., :B]
            res = er.check_groups(name, "grad", d_g, g32 - pre_g - ref_g, ref["grad"])
            res.update(er.check_groups(name, "curv", d_h, h32.astype(np.float64) - pre_h[:H, :13, :13] - ref_c, ref["curv"][:H]))
            print(name, summary({k: v for k, v in res.items() if v[0] or v[1]}))
            if label == "all":
                only_g = model_call(ac, gpu, p, inp, inp["lam"], pre_g[..., :B], None, want=("glin",))
                only_h = model_call(ac, gpu, p, inp, inp["lam"], None, pre_h[..., :B], want=("Hz",))
                assert bits_equal(only_g["glin"], out["glin"]) and bits_equal(only_h["Hz"], out["Hz"]), (name, "glin only / Hz only differ from the joint call")
                if not lam_on:      # multipliers all zero = the penalty entry, bit for bit
                    zin = Inputs(gpu, X=X, lam=np.zeros((H + 1, 8, B)))
                    z = model_call(ac, gpu, p, zin, zin["lam"], pre_g[..., :B], pre_h[..., :B])
                    assert all(bits_equal(z[k], out[k]) for k in z), (name, "lam = 0 differs from lam = NULL")
                if B == 37 and lam_on:
                    sl = slice(16, 37)
                    sub = Inputs(gpu, X=np.ascontiguousarray(c["X"][:, :, sl]), lam=np.ascontiguousarray(ref["lam"][:, :, sl]))
                    part = model_call(ac, gpu, p, sub, sub["lam"], pre_g[..., sl], pre_h[..., sl])
                    assert all(bits_equal(part[k], out[k][..., sl]) for k in part), (name, "columns 16:37 differ from the parent batch")


# ---- k_envelope_multipliers -----------------------------------------------------------------------------------------------------------
def update_call(ac, gpu, p, inp, lam0, prior):
    """lam = lam0, viol = prior ('null': no array), then the update -> (lam host, viol host or None)"""
    import torch
    from aircraft_amd import _lib

    lib = ac._sync()
    X = inp["X"]
    H, B = X.shape[0] - 1, X.shape[2]
    runs = []
    for _ in range(2):
        bufs = {"lam": guarded((H + 1, 8, B), gpu)}
        bufs["lam"][1].copy_(dev(lam0, gpu))
        if prior is not None:
            bufs["viol"] = guarded((B,), gpu); bufs["viol"][1].copy_(dev(prior, gpu))
        _lib.check(lib.ac_envelope_al_update_f32(ac._handle, C.byref(p), ptr(X), B, H, ptr(bufs["lam"][1]),
                                                 ptr(bufs["viol"][1] if prior is not None else None), ac._stream()), "ac_envelope_al_update_f32")
        torch.cuda.synchronize()
        launched(ac, "k_envelope_multipliers", (H + 1) * B)
        assert_guards(bufs, "envelope_update")
        runs.append({k: v[1] for k, v in bufs.items()})
    for k in runs[0]:
        assert bits_equal(runs[0][k], runs[1][k]), (k, "a repeat of the call differs")
    inp.unchanged()
    return runs[0]["lam"].cpu().numpy(), (runs[0]["viol"].cpu().numpy() if prior is not None else None)


@pytest.mark.parametrize("B,H", er.MODEL_SHAPES)
def test_envelope_multiplier_update(gpu, ac, B, H):
    """ac_envelope_al_update_f32, one lane per (node, instance) ((37, 7) spreads an instance's nodes over two blocks): the new
    multipliers from zero, from random ones (half of them zero) and from large ones; the excess measure with no array, into
    zeros and into a prior value between the instances' excesses (the result is the larger); rows without a finite span
    (+-3e38) are measured unscaled"""
    c = er.parent(H)
    X = np.ascontiguousarray(c["X"][:, :, :B])
    inp = Inputs(gpu, X=X)
    starts = er.update_starts(c)
    for label, row, side in (("all", None, "both"), ("beta", 1, "both"), ("z.up", 3, "up")):
        lo, hi, _ = er.run_bounds(row, side)
        p = pen(lo, hi)
        exc = io.envelope_excess(c["rows"], lo, hi)
        for sname, lam0 in starts.items():
            name = f"envelope_update[B{B}-H{H}-{label}-{sname}]"
            want = io.envelope_al_update(c["rows"], lo, hi, er.W, lam0)
            f32 = er.al_np(np.float32, c["rows32"], c["Jx32"], lo, hi, er.W, lam0)
            e32 = er.lam_err(f32["new"], want).max(axis=(0, 2))
            e32x = float(er.excess_err(f32["excess"], exc).max())
            bars = np.array([er.bar_of(float(e), f"{name}:{i}") for i, e in enumerate(e32)])
            barx = er.bar_of(e32x, f"{name}:excess")
            mid = np.float32(np.median(exc))
            res = {}
            for vname, prior in (("null", None), ("zeroed", np.zeros(B)), ("prior", np.full(B, mid))):
                lam, viol = update_call(ac, gpu, p, inp, lam0[:, :, :B], prior)
                res[vname] = lam
                if viol is not None:
                    ref_v = np.maximum(exc, float(prior[0]))
                    ev = np.abs(viol.astype(np.float64) - ref_v[:B]) / np.maximum(ref_v[:B], exc.max())
                    assert (ev <= barx).all(), (name, vname, "excess beyond", barx, float(ev.max()))
                    below = exc[:B] < float(prior[0]) * (1 - 1e-5)
                    assert np.array_equal(viol[below].view(np.int32), np.float32(prior)[below].view(np.int32)), (name, "a smaller excess replaced the prior value")
                    worst_x = float(ev.max())
            assert all(np.array_equal(res["null"].view(np.int32), v.view(np.int32)) for v in res.values()), (name, "the excess array changes the multipliers")
            got = res["null"].astype(np.float64)
            assert (got >= 0).all() and er.zeros_kept(got, want[..., :B]), (name, "a clamped multiplier is not exactly zero")
            e = er.lam_err(got, want)
            assert (e <= bars[None, :, None]).all(), (name, "beyond", bars.tolist(), "worst per row and side", e.max(axis=(0, 2)).tolist())
            assert np.array_equal(got[:, [3, 7]], want[:, [3, 7], :B]), (name, "height row")
            parity_report(name, lam=dict(worst=float(e.max()), e32=float(e32.max())), excess=dict(worst=worst_x, e32=e32x))
            print(name, f"lam {e.max():.1e}/{e32.max():.1e}  excess {worst_x:.1e}/{e32x:.1e}")
            if sname == "random" and label == "all" and B >= 37:
                assert (want[..., :B] == 0)[lam0[..., :B] > 0].sum() >= 2      # multipliers driven to the clamp


# ---- other models, status codes -----------------------------------------------------------------------------------------------------------
def test_envelope_kernels_read_only_epsilon_from_the_model(gpu, ac):
    """the default model, the linear model and the shipped net have the cubic-fit aircraft's epsilon: cost, model and update
    are bit-identical on all of them"""
    c = er.parent(3)
    B, H = 7, 3
    ref = er.reference(c)
    p = pen(ref["lo"], ref["hi"])
    X, lam = np.ascontiguousarray(c["X"][:, :, :B]), np.ascontiguousarray(c["lam"][:, :, :B])
    rng = np.random.default_rng(3)
    pre_g, pre_h = f32_exact(rng.normal(0, 1, (H + 1, 13, B))), f32_exact(rng.normal(0, 1, (H + 1, 21, 21, B)))
    res = {}
    for model in ("poly", "default", "linear", "nn"):
        a = ac if model == "poly" else make_aircraft(model)
        assert a.epsilon == er.EPSILON
        inp = Inputs(gpu, X=X, lam=lam)
        m = model_call(a, gpu, p, inp, inp["lam"], pre_g, pre_h)
        res[model] = (cost_call(a, gpu, p, inp, inp["lam"], B, np.zeros(B)), m["glin"].cpu().numpy(), m["Hz"].cpu().numpy(),
                      *update_call(a, gpu, p, inp, lam, np.zeros(B)))
    for model in ("default", "linear", "nn"):
        for x, y in zip(res[model], res["poly"]):
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), model


def test_envelope_status_codes(gpu, ac):
    import torch
    from aircraft_amd import Quadrotor

    c = er.parent(1)
    B, H = 6, 1
    X = dev(np.ascontiguousarray(c["X"][:, :, :B]), gpu)
    lam = dev(np.ascontiguousarray(c["lam"][:, :, :B]), gpu)
    J, gl, Hz, viol = (torch.zeros(s, device=gpu) for s in ((B,), (H + 1, 13, B), (H, 21, 21, B), (B,)))
    p, p0 = pen(er.LO, er.HI), pen(er.LO, er.HI, w=0.0)

    def entries(a, p, lam, Bl=B, n=B, gl=gl, Hz=Hz):
        lib, h, s = a._sync(), a._handle, a._stream()
        return dict(cost=lib.ac_envelope_cost_f32(h, C.byref(p), ptr(X), n, H, ptr(J), s),
                    model=lib.ac_envelope_model_f32(h, C.byref(p), ptr(X), n, H, ptr(gl), ptr(Hz), s),
                    al_cost=lib.ac_envelope_al_cost_f32(h, C.byref(p), ptr(lam), Bl, ptr(X), n, H, ptr(J), s),
                    al_model=lib.ac_envelope_al_model_f32(h, C.byref(p), ptr(lam), ptr(X), n, H, ptr(gl), ptr(Hz), s),
                    al_update=lib.ac_envelope_al_update_f32(h, C.byref(p), ptr(X), n, H, ptr(lam), ptr(viol), s))

    assert set(entries(Quadrotor(), p, lam).values()) == {-3}                       # the fixed-wing plugin's rows
    assert set(entries(ac, p, lam, n=0).values()) == {0}                            # B = 0: nothing to do
    st = entries(ac, p0, lam)                                                       # multipliers need a positive weight
    assert st["al_cost"] == st["al_model"] == st["al_update"] == -1 and st["cost"] == st["model"] == 0
    assert entries(ac, p, lam, Bl=4)["al_cost"] == -1                               # B % Bl != 0
    st = entries(ac, p, lam, gl=None, Hz=None)                                      # both outputs NULL
    assert st["model"] == st["al_model"] == -1
    torch.cuda.synchronize()
