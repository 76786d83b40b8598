"""Block-by-block reference for the width-128 plane routes of the sensitivity kernels (k_nn_step_sens<8, true, HID> and
k_nn_step_sens_pair<8, HID>, MlpEngine::layer_bf): the metric, the bar rule and the case matrix that
tests/test_sens_blocks_ref.py (CPU) and tests/test_gpu_plane_routes.py (GPU) share.

Metric.  The net reaches A only through the off-identity blocks of the v and omega rows (d omega+/d q ~ 0.17, d omega+/d v ~ 0.012,
d v+/d omega ~ 0.0012 beside a diagonal of 1), so one norm per unit hides a lost plane product.  Here every unit is cut into
blocks — A - I by row group x column group, B by row group x (aileron/elevator | rudder | thrust), c by row group — and a
block's error is  max|got - ref| over the block / max(max|ref| over the block, FLOOR x the unit's largest block of that array).
What the reference has exactly (A[:, :3] = [I; 0], the dead control columns of B) must match exactly.

Bar.  8 x e_ref per case and block, e_ref = the worst error against the float64 oracle, on the case's own sampled units, of
the fp32 restatement of the step (tests/host_dyn/dyn_host.cpp::host_nn_sens) in plain fp32 or in the route's own arithmetic,
whichever is larger — never a GPU figure.  A case is usable only while every e_ref <= E_REF_CAP, so that no bar exceeds the
suite's SENS_BLOCK_TOL = 1e-4; a case that breaks the cap gets other inputs, never a wider bar."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np

from aircraft_amd import Aircraft, AircraftConfiguration, AircraftOpts, MlpData
from tests.helpers import GLIDER, block_rel_err, f32_exact, synthetic_units

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 1e-3          # as helpers.unit_rowblock_rel
BAR_FACTOR = 8.0
E_REF_CAP = 1.25e-5   # 8 x 1.25e-5 = SENS_BLOCK_TOL
MODES = {"fp32": 0, "f16": 1, "bf16": 2}
HOST_THREADS = 8      # fixed: the units of one host call are cut into this many slices (ctypes releases the GIL)
MI355X_CUS = 256
# The step of every case.  The diagonal entries of A are 1 + O(dt) in fp32: they carry an absolute quantum of 2^-24 whatever
# computes them, so the error of the (v, v) and (omega, omega) blocks relative to A - I is at least 2^-24 / |A - I|, and the
# cap needs |A - I| >= 4.8e-3 on every sampled unit.  At the suite's usual dt = 0.01 the smallest such block is 8e-4 (e_ref
# 2e-5 .. 7.5e-5, measured, in ANY fp32 arithmetic: above the cap); the blocks grow with dt, and 2^-4 — exact in fp32, so the
# oracle and the kernels step by the same number — brings every case under the cap (tests/test_sens_blocks_ref.py).  2^-3
# does not: RK4 then amplifies rounding on the fastest units (e_ref 7e-5 on the omega rows of the 2 x 128 net).
DT = 0.0625

ROWS = {"p": slice(0, 3), "v": slice(3, 6), "q": slice(6, 10), "w": slice(10, 13)}
EYE = np.eye(13)[:, :, None]


# ---- metric -------------------------------------------------------------------------------------------------------------
def families(A, B, c):
    """{array: {block: (rows, cols, n) view}} of one result; A enters as A - I"""
    Am = np.asarray(A, dtype=np.float64) - EYE
    B = np.asarray(B, dtype=np.float64); c = np.asarray(c, dtype=np.float64)
    fa = {f"A[{r},{k}]": Am[ROWS[r], ROWS[k]] for r in "vqw" for k in "vqw"}
    fa.update({f"A[p,{k}]": Am[ROWS["p"], ROWS[k]] for k in "vq"})
    fb = {}
    for r in "vw":
        fb[f"B[{r},ae]"] = B[ROWS[r], 0:2]
        fb[f"B[{r},rud]"] = B[ROWS[r], 2:3]
    for r in "pvqw":
        fb[f"B[{r},thr]"] = B[ROWS[r], 6:7]
    fc = {f"c[{r}]": c[ROWS[r], None] for r in "pvqw"}
    return {"A": fa, "B": fb, "c": fc}


def block_errors(got, ref, floor=FLOOR):
    """got, ref: (A, B, c) -> {block: (n,) error}"""
    fg, fr = families(*got), families(*ref)
    out = {}
    for fam in fr:
        n = next(iter(fr[fam].values())).shape[-1]
        scale = {k: np.abs(v).reshape(-1, n).max(axis=0) for k, v in fr[fam].items()}
        largest = np.max(np.stack(list(scale.values())), axis=0)
        for k, v in fr[fam].items():
            d = np.abs(fg[fam][k] - v).reshape(-1, n).max(axis=0)
            with np.errstate(all="ignore"):
                e = d / np.maximum(np.maximum(scale[k], floor * largest), 1e-300)
            out[k] = np.where(np.isfinite(e), e, np.inf)
    return out


def block_scales(ref):
    """{block: (n,) max|ref| over the block} — what the medians quoted in DESIGN.md section 5 are taken from"""
    return {k: np.abs(v).reshape(-1, v.shape[-1]).max(axis=0) for fam in families(*ref).values() for k, v in fam.items()}


def assert_exact_structure(A, B):
    A = np.asarray(A); B = np.asarray(B)
    assert np.array_equal(A[:, :3], np.broadcast_to(np.eye(13, dtype=A.dtype)[:, :3, None], A[:, :3].shape)), "A[:, :3] != [I; 0]"
    assert not B[:, 3:6].any(), "dead control columns of B are not zero"


def state_errors(F, Fr):
    """x+ per unit in the metric of block_rel_err -> (n,)"""
    return np.array([block_rel_err(F[:, k:k + 1], Fr[:, k:k + 1]) for k in range(F.shape[1])])


def worst(err):
    return {k: float(v.max()) for k, v in err.items()}


def merge_worst(*ws):
    return {k: max(w[k] for w in ws) for k in ws[0]}


# ---- the two host libraries ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dyn_lib():
    from tests.test_host_dyn import _lib  # (one build recipe for libdyn_host.so: g++ -O1 -ffp-contract=off)

    L = _lib()
    fp, vp = C.POINTER(C.c_float), C.c_void_p
    L.host_nn_sens.restype = C.c_int
    L.host_nn_sens.argtypes = [vp, C.c_int, vp, vp, vp, vp, fp, fp, fp, fp, C.c_int, C.c_int, fp, fp, C.c_float, fp, C.c_long,
                               fp, fp, fp, fp]
    L.host_plane_round.restype = None
    L.host_plane_round.argtypes = [C.c_int, fp, C.c_long, fp]
    return L


@functools.lru_cache(maxsize=None)
def gate_lib():
    src = os.path.join(HERE, "host_f16", "f16_pack_host.cpp")
    so = os.path.join(HERE, "host_f16", "libf16_pack_host.so")
    deps = [src, os.path.join(HERE, "..", "aircraft_amd", "csrc", "ac_f16_pack.hpp"),
            os.path.join(HERE, "..", "aircraft_amd", "csrc", "ac_bf16_pack.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        tmp = f"{so}.{os.getpid()}"
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src], check=True)
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.host_f16_gate.restype = C.c_int
    L.host_f16_gate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def host_f16_gate(net):
    """(verdict, worst) of f16_gate (ac_f16_pack.hpp) on an MlpData: 0 passes"""
    Ws, bs = net.weights, net.biases
    widths = (C.c_int * (len(Ws) + 1))(*net.widths)
    pw = (C.c_void_p * len(Ws))(*[W.ctypes.data for W in Ws])
    pb = (C.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    w = C.c_double()
    return gate_lib().host_f16_gate(len(Ws), widths, pw, pb, C.byref(w)), w.value


def host_nn_sens(ac, X, U, dt, mode, drop=-1):
    """The fp32 restatement of the step with tangents on the host: (Xn, A, B, c), float32, component-major."""
    L = dyn_lib()
    fp = C.POINTER(C.c_float)
    md = ac.coefficient_model.oracle_data()
    Ws = [np.ascontiguousarray(w, dtype=np.float32) for w in md["weights"]]
    bs = [np.ascontiguousarray(b, dtype=np.float32) for b in md["biases"]]
    nl = len(Ws)
    widths = (C.c_int * (nl + 1))(Ws[0].shape[1], *[w.shape[0] for w in Ws])
    act = (C.c_int * nl)(*[int(a) for a in md["act"]])
    pw = (C.c_void_p * nl)(*[w.ctypes.data for w in Ws])
    pb = (C.c_void_p * nl)(*[b.ctypes.data for b in bs])
    sc = [np.ascontiguousarray(md[k], dtype=np.float32) for k in ("input_mean", "input_std", "output_mean", "output_std")]
    p = ac._param_struct()
    n = X.shape[1]
    per_unit = np.ndim(dt) > 0
    dtv = np.ascontiguousarray(dt, dtype=np.float32) if per_unit else None

    def piece(sl):
        Xf = np.ascontiguousarray(X[:, sl], dtype=np.float32); Uf = np.ascontiguousarray(U[:, sl], dtype=np.float32)
        m = Xf.shape[1]
        out = [np.zeros(s, dtype=np.float32) for s in ((13, m), (13, 13, m), (13, 7, m), (13, m))]
        dts = np.ascontiguousarray(dtv[sl]) if per_unit else None
        rc = L.host_nn_sens(C.byref(p), nl, widths, act, pw, pb, *[a.ctypes.data_as(fp) for a in sc], mode, drop,
                            Xf.ctypes.data_as(fp), Uf.ctypes.data_as(fp), 0.0 if per_unit else float(dt),
                            dts.ctypes.data_as(fp) if per_unit else None, m, *[a.ctypes.data_as(fp) for a in out])
        assert rc == 0, rc
        return out

    cuts = np.linspace(0, n, min(HOST_THREADS, n) + 1).astype(int)
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        parts = list(ex.map(piece, [slice(a, b) for a, b in zip(cuts[:-1], cuts[1:])]))
    return tuple(np.concatenate([pt[i] for pt in parts], axis=-1) for i in range(4))


# ---- nets and cases -----------------------------------------------------------------------------------------------------
def scaled_hidden(net, scale):
    W = [w.copy() for w in net.weights]
    for l in range(1, len(W) - 1):
        W[l] = W[l] * np.float32(scale)
    return MlpData(W, net.biases, net.act, net.input_mean, net.input_std, net.output_mean, net.output_std)


def with_weights(net, W, act=None):
    return MlpData(W, net.biases, net.act if act is None else act, net.input_mean, net.input_std, net.output_mean, net.output_std)


def gate_scale(net):
    """1.0 if f16_gate accepts the net, else the largest power of two below 1 on every hidden layer that makes it accept"""
    s = 1.0
    while host_f16_gate(scaled_hidden(net, s))[0] != 0:
        s *= 0.5
        assert s > 2.0 ** -12, "no power-of-two scale of the hidden layers passes the gate"
    return s


@functools.lru_cache(maxsize=None)
def gate_edge_shift():
    """the largest k for which the cfg3 net (seed 42) with W0 2^-k still passes f16_gate"""
    syn = MlpData.synthetic((128,) * 4, seed=42)
    k = 0
    while host_f16_gate(with_weights(syn, [syn.weights[0] * np.float32(2.0 ** -(k + 1))] + syn.weights[1:]))[0] == 0:
        k += 1
        assert k < 40
    return k


@dataclass(frozen=True)
class Case:
    name: str
    hidden: tuple
    route: str                    # "bf16" | "f16" | "auto" | "fp32" (use_mfma=False)
    mode: str                     # the route's own host arithmetic: "bf16" | "f16" | "fp32"
    kind: str = "depth"           # "depth" | "edge" | "arg"
    net_seed: int = 42
    unit_seed: int = 5
    w0_shift: int = 0             # W0 2^-w0_shift
    tanh_last: bool = False
    arg: str = ""                 # "dt" | "shoot" | "nonorm" | "sub2"

    @property
    def use_mfma(self):
        return self.route != "fp32"

    @property
    def normalise(self):
        return self.arg != "nonorm"

    @property
    def substeps(self):
        return 2 if self.arg == "sub2" else 1


@functools.lru_cache(maxsize=None)
def case_net(case):
    """(MlpData, hidden-layer scale that the gate made necessary)"""
    net = MlpData.synthetic(case.hidden, seed=case.net_seed)
    if case.w0_shift:
        net = with_weights(net, [net.weights[0] * np.float32(2.0 ** -case.w0_shift)] + net.weights[1:])
    if case.tanh_last:
        net = with_weights(net, net.weights, act=[1] * len(net.weights))
    scale = 1.0
    if case.route == "f16":
        scale = gate_scale(net)
        if scale != 1.0:
            net = scaled_hidden(net, scale)
    return net, scale


def case_aircraft(case):
    net, _ = case_net(case)
    opts = AircraftOpts(coeff_model_type="nn", coeff_model_path=net, aircraft_config=AircraftConfiguration(dict(GLIDER)),
                        physical_integration_substeps=case.substeps, use_mfma=case.use_mfma)
    ac = Aircraft(opts)
    ac.normalise = case.normalise
    if case.route in ("bf16", "f16", "auto"):
        ac.hidden_route = case.route
    return ac


def depth_cases():
    out = []
    for k in range(2, 8):
        for route in ("bf16", "f16"):
            out.append(Case(f"k{k}-{route}", (128,) * k, route, route))
    out.append(Case("k4-fp32", (128,) * 4, "fp32", "fp32"))
    for route in ("bf16", "f16"):
        out.append(Case(f"ragged-{route}", (100, 128, 90), route, route))
        out.append(Case(f"tanhlast-{route}", (128,) * 4, route, route, tanh_last=True))
    return out


def edge_cases():
    k = gate_edge_shift()
    return [Case("edge-f16", (128,) * 4, "f16", "f16", kind="edge", w0_shift=k),
            Case("edge-bf16", (128,) * 4, "bf16", "bf16", kind="edge", w0_shift=k),
            Case("rejected-auto", (128,) * 4, "auto", "bf16", kind="edge", w0_shift=20)]


def arg_cases():
    return [Case(f"{arg}-k{k}-{route}", (128,) * k, route, route, kind="arg", arg=arg)
            for arg in ("dt", "shoot", "nonorm", "sub2") for k in (2, 4) for route in ("bf16", "f16")]


def all_cases():
    return depth_cases() + edge_cases() + arg_cases()


SHOOT_B, SHOOT_H = 37, 3
SMALL_N = 101


def depth_sizes(cus):
    """(n of the issue's call, n of the three-round call, chunk length).  n = 96 CUs + 64 + 37 leaves a remainder above half a
    round, so everything goes to the one-wave kernel — in ONE and a half rounds (64 CUs units are a round): no workgroup gets a
    third task.  The second size adds a whole round, 160 CUs + 64 + 37: half of the workgroups then run a third task, the last
    one ragged, and its first n units are the first call's."""
    return 96 * cus + 101, 160 * cus + 101, 32 * cus


def depth_sample(cus):
    """sampled unit indices of a depth x route case (into the three-round call's units): the whole first task, one whole
    second-round and one whole third-round task, both ragged tails, the first 16 units of every chunk"""
    n, n3, chunk = depth_sizes(cus)
    idx = set(range(64))
    t2, t3 = cus + 3, 2 * cus + 5
    idx.update(range(64 * t2, 64 * t2 + 64)); idx.update(range(64 * t3, 64 * t3 + 64))
    idx.update(range(n - 37, n)); idx.update(range(n3 - 37, n3))
    for s in range(0, n3, chunk):
        idx.update(range(s, min(s + 16, n3)))
    return np.array(sorted(idx))


@functools.lru_cache(maxsize=None)
def _units(n, seed):
    X, U = synthetic_units(n, seed=seed)
    return f32_exact(X), f32_exact(U)


def case_units(case, cus=MI355X_CUS):
    """(X, U, dt, sample): the case's inputs as float64 holding fp32 values, and the sampled indices the bar is taken on"""
    if case.kind == "depth":
        X, U = _units(depth_sizes(cus)[1], case.unit_seed)
        return X, U, DT, depth_sample(cus)
    n = SHOOT_B * SHOOT_H if case.arg == "shoot" else SMALL_N
    X, U = _units(n, case.unit_seed + 1)
    dt = DT
    if case.arg == "dt":
        dt = f32_exact(DT * np.random.default_rng(9).uniform(0.8, 1.2, n))
    return X, U, dt, np.arange(n)


def case_oracle(case, net=None):
    from oracle import Oracle

    ac = case_aircraft(case)
    md = dict(ac.coefficient_model.oracle_data())
    if net is not None:
        md["weights"], md["biases"] = net.weights, net.biases
    md["weights"] = [np.asarray(w, dtype=np.float64) for w in md["weights"]]
    md["biases"] = [np.asarray(b, dtype=np.float64) for b in md["biases"]]
    return Oracle(ac.airframe_dict(), "nn", md, substeps=ac.physical_integration_substeps, normalise=ac.normalise,
                  stall_scaling=ac.stall_scaling, epsilon=ac.epsilon, gravity=ac.gravity)


OWN_SCALE = ("B[v,ae]", "B[w,ae]")  # the pure tangent paths of B: through the net's Jacobian and nothing else


def case_errors(case, got, ref):
    """block_errors; the gate-edge cases also hold the pure tangent paths of B on their OWN scale (no floor), as `block|own`:
    their first layer is scaled down by 2^-12 and more, and these blocks with it, next to the analytic rudder and thrust columns"""
    err = block_errors(got, ref)
    if case.kind == "edge":
        own = block_errors(got, ref, floor=0.0)
        err.update({f"{k}|own": own[k] for k in OWN_SCALE})
    return err


@functools.lru_cache(maxsize=None)
def case_reference(case, cus=MI355X_CUS):
    """On the case's sampled units: (oracle (F, A, B, c), e_ref {block: worst}, e_mode0, e_route, eF_ref).  Cached: one host and
    one oracle run per case and process.  Sub-stepped cases have no host entry: e_ref is None."""
    X, U, dt, idx = case_units(case, cus)
    Xs, Us = X[:, idx], U[:, idx]
    dts = dt[idx] if np.ndim(dt) > 0 else dt
    ref = case_oracle(case).step_sens(Xs, Us, dts)
    if case.substeps > 1:
        return ref, None, None, None, None
    ac = case_aircraft(case)
    h0 = host_nn_sens(ac, Xs, Us, dts, 0)
    e0 = worst(case_errors(case, h0[1:], ref[1:]))
    eF = float(state_errors(h0[0], ref[0]).max())
    assert_exact_structure(h0[1], h0[2])
    em = e0
    if MODES[case.mode] != 0:
        hm = host_nn_sens(ac, Xs, Us, dts, MODES[case.mode])
        em = worst(case_errors(case, hm[1:], ref[1:]))
        eF = max(eF, float(state_errors(hm[0], ref[0]).max()))
        assert_exact_structure(hm[1], hm[2])
    return ref, merge_worst(e0, em), e0, em, eF


def check_case_blocks(case, got, cus=MI355X_CUS):
    """got = (F, A, B, c) of the GPU on the case's sampled units.  Asserts the cap BEFORE a GPU number is read and the exact
    structure, then measures every block of every unit against 8 x e_ref.  Returns ({block: worst GPU / e_ref},
    {block: (units beyond the bar, worst, e_ref)} — empty when the case passes —, x+ worst of the GPU, x+ worst of the host);
    the caller reports them and asserts."""
    ref, e_ref, _, _, eF = case_reference(case, cus)
    over = {k: v for k, v in e_ref.items() if not v <= E_REF_CAP}
    assert not over, (case.name, "e_ref above the cap: the case needs other inputs", over)
    assert_exact_structure(got[1], got[2])
    err = case_errors(case, got[1:], ref[1:])
    ratio = {k: float(err[k].max() / max(e_ref[k], 1e-300)) for k in err}
    bad = {k: (int((err[k] > BAR_FACTOR * e_ref[k]).sum()), float(err[k].max()), e_ref[k]) for k in err
           if (err[k] > BAR_FACTOR * e_ref[k]).any()}
    gF = float(state_errors(np.asarray(got[0], dtype=np.float64), ref[0]).max())
    return ratio, bad, gF, eF
