"""The host side of the two-plane f16 hidden layers (aircraft_amd/csrc/ac_f16_pack.hpp, compiled with g++ here): the split,
the packed image, a NumPy emulation of the kernel's arithmetic (MlpEngine::layer_bf, f16 form) chained through the three
hidden layers with tangents, and the range gate that decides whether a net takes the route.  No GPU.

Subnormal f16 values: the kernel and the host packer KEEP them (the behaviour the code assumes of the matrix core,
v_cvt_pk_f16_f32 and v_fma_mix_f32 of gfx950; tools/experiments/f16_subnormals.hip probes it), so the
emulation keeps them; the variant that flushes them in the matrix core only (residual taken from an unflushed hi) is
emulated as well and must be flagged as failing, and the consistent flush must stay inside the bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aircraft_amd.utils import MlpData
from tests.helpers import golden

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_f16", "f16_pack_host.cpp")
S = np.float32(2048.0)
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("f16") / "libf16_pack_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.host_f16_layer_bytes.restype = C.c_int
    L.host_f16_front_bytes.restype = C.c_int
    L.host_f16_split2.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    L.host_f16_pack_layer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.host_f16_gate.restype = C.c_int
    L.host_f16_gate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def split2(lib, w):
    w = np.ascontiguousarray(w, dtype=f32).ravel()
    p = np.zeros((w.size, 2), dtype=np.uint16)
    lib.host_f16_split2(w.ctypes.data, w.size, p.ctypes.data)
    return p


def h2f(bits):
    return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(f32)


def ulp32(w):
    w = np.abs(np.asarray(w, dtype=f32))
    return (np.nextafter(w, f32(np.inf)) - w).astype(f64)


def chunk_row(c, kk):
    g, q = kk >> 3, kk & 7
    return 32 * c + (16 if q & 4 else 0) + 4 * g + (q & 3)


def unpack(img, wt, nin, nout):
    """Inverse of f16_pack_layer, written independently: (hi [nout][nin], lo' [nout][nin], b [nout])."""
    half, kc = wt // 2, wt // 2
    front = (half * kc * 2 + 1) * 1024
    raw = np.frombuffer(img, dtype=np.uint8)
    P = np.zeros((2, 16 * wt, 16 * wt), dtype=np.uint16)
    for nt in range(wt):
        base = 0 if nt < half else front
        for c in range(kc):
            for p in range(2):
                off = base + (((nt % half) * kc + c) * 2 + p) * 1024
                frag = raw[off:off + 1024].view(np.uint16).reshape(64, 8)
                for lane in range(64):
                    for q in range(8):
                        P[p, 16 * nt + (lane & 15), chunk_row(c, 8 * (lane >> 4) + q)] = frag[lane, q]
    b = raw[half * kc * 2 * 1024:half * kc * 2 * 1024 + 64 * wt].view(f32)
    return P[0, :nout, :nin], P[1, :nout, :nin], b[:nout]


def check_split(w, p):
    """hi = RNE f16 of w (subnormals kept); |hi + lo'/S - w| <= max(2 ulp32(w), 2^-25)."""
    w = np.ascontiguousarray(w, dtype=f32).ravel()
    hi, lo = h2f(p[:, 0]), h2f(p[:, 1])
    assert np.array_equal(p[:, 0], w.astype(np.float16).view(np.uint16))  # NumPy's conversion: RNE, gradual underflow
    assert np.array_equal(p[:, 1], ((w - hi).astype(f32) * S).astype(f32).astype(np.float16).view(np.uint16))
    err = np.abs(hi.astype(f64) + lo.astype(f64) / 2048.0 - w.astype(f64))
    bound = np.maximum(2.0 * ulp32(w), 2.0 ** -25)
    assert (err <= bound).all(), float((err / bound).max())
    return float((err / ulp32(w)).max())


def nets():
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    w = golden("scaledmodel_weights.npz")
    return [("cfg3", syn.weights[1:-1], syn.biases[1:-1]), ("checkpoint", [w["W1"]], [w["b1"]])]


@pytest.mark.parametrize("name,Ws,bs", nets(), ids=lambda v: v if isinstance(v, str) else "")
def test_split_within_two_ulps_and_image_unpacks(lib, name, Ws, bs):
    wt = 8
    for W, b in zip(Ws, bs):
        W = np.ascontiguousarray(W, dtype=f32); b = np.ascontiguousarray(b, dtype=f32)
        p = split2(lib, W)
        worst = check_split(W, p)
        print(f"{name}: worst split error {worst:.2f} ulp32")
        img = np.zeros(lib.host_f16_layer_bytes(wt), dtype=np.uint8)
        nout, nin = W.shape
        lib.host_f16_pack_layer(W.ctypes.data, b.ctypes.data, nin, nout, wt, img.ctypes.data)
        hi, lo, bu = unpack(img.tobytes(), wt, nin, nout)
        assert np.array_equal(hi.ravel(), p[:, 0]) and np.array_equal(lo.ravel(), p[:, 1])
        assert np.array_equal(bu.view(np.uint32), b.view(np.uint32))  # bias bit-exact
    assert lib.host_f16_layer_bytes(8) == 65 * 1024 and lib.host_f16_front_bytes(8) == 33 * 1024


def test_split_over_a_log_uniform_sample(lib):
    rng = np.random.default_rng(11)
    w = (10.0 ** rng.uniform(-9, 2, size=250_000) * rng.choice([-1.0, 1.0], size=250_000)).astype(f32)
    p = split2(lib, w)
    check_split(w, p)
    # the subnormal rule: hi keeps f16 subnormals (gradual underflow), it is zero only under half the smallest subnormal
    small = np.abs(w) < 2.0 ** -14
    assert small.any() and (h2f(p[small, 0])[np.abs(w[small]) > 2.0 ** -24] != 0).all()
    assert (p[np.abs(w) < 2.0 ** -25, 0] & 0x7fff == 0).all()


# ---- the kernel's arithmetic, emulated ------------------------------------------------------------------------------------
def f16r(x, mode):
    """fp32 -> f16 -> fp32.  mode "keep": subnormals honoured; "flush": every subnormal result is zero."""
    h = x.astype(np.float16).astype(f32)
    if mode == "flush":
        h = np.where(np.abs(h) < 2.0 ** -14, f32(0), h)
    return h


def split_h2(x, mode):
    """mode "keep" / "flush" (consistent: the residual is taken from the hi the matrix core sees) / "inconsistent" (residual
    from an unflushed hi, the matrix core flushing both planes)."""
    hi_v = f16r(x, "flush" if mode == "flush" else "keep")
    lo_v = f16r(((x - hi_v).astype(f32) * S).astype(f32), "flush" if mode == "flush" else "keep")
    if mode == "inconsistent":
        flush = lambda h: np.where(np.abs(h) < 2.0 ** -14, f32(0), h)  # noqa: E731
        return [flush(hi_v), flush(lo_v)]
    return [hi_v, lo_v]


def layer_f16(mode):
    """One hidden layer in the order of MlpEngine::layer_bf (f16): per 32-deep chunk lo' hi, then hi lo' into `lo`, hi hi into
    `hi`; every MFMA an exact sum rounded once into its fp32 accumulator; the tile is fma(lo, 1/S, hi)."""
    def run(W, X, bias):
        w, x = split_h2(W, mode), split_h2(X, mode)
        hi = np.zeros((W.shape[0], X.shape[1]), f32) if bias is None else np.broadcast_to(bias[:, None], (W.shape[0], X.shape[1])).astype(f32)
        lo = np.zeros((W.shape[0], X.shape[1]), f32)
        for c in range(4):
            k = slice(32 * c, 32 * c + 32)
            for i, j in ((1, 0), (0, 1)):
                lo = (lo.astype(f64) + w[i][:, k].astype(f64) @ x[j][k].astype(f64)).astype(f32)
            hi = (hi.astype(f64) + w[0][:, k].astype(f64) @ x[0][k].astype(f64)).astype(f32)
        return (hi.astype(f64) + lo.astype(f64) / 2048.0).astype(f32)  # one rounding: the fma
    return run


def layer_fp32(W, X, bias):
    acc = np.zeros((W.shape[0], X.shape[1]), f32) if bias is None else np.broadcast_to(bias[:, None], (W.shape[0], X.shape[1])).astype(f32)
    for c in range(4):
        k = slice(32 * c, 32 * c + 32)
        acc = (acc.astype(f64) + W[:, k].astype(f64) @ X[k].astype(f64)).astype(f32)
    return acc


def chain(layer, syn, Z, dt):
    """value + 5 tangents through the net; hidden layers by `layer` (None: float64); edge layers exactly in dt."""
    Ws, bs = syn.weights, syn.biases
    pre = Ws[0].astype(dt) @ Z.astype(dt) + bs[0].astype(dt)[:, None]
    h = np.tanh(pre); sp = 1 - h * h
    T = [sp * Ws[0][:, j].astype(dt)[:, None] for j in range(5)]
    for W, b in zip(Ws[1:-1], bs[1:-1]):
        if layer is None:
            pre = W.astype(f64) @ h + b.astype(f64)[:, None]
            Tn = [W.astype(f64) @ t for t in T]
        else:
            pre = layer(W.astype(f32), h.astype(f32), b.astype(f32))
            Tn = [layer(W.astype(f32), t.astype(f32), None) for t in T]
        h = np.tanh(pre).astype(dt); sp = (1 - h * h).astype(dt)
        T = [(sp * t).astype(dt) for t in Tn]
    y = Ws[-1].astype(f64) @ h.astype(f64) + bs[-1].astype(f64)[:, None]
    J = np.stack([Ws[-1].astype(f64) @ t.astype(f64) for t in T], axis=1)  # (6, 5, n)
    return y, J


def chain_errors(layer, syn, Z):
    n = Z.shape[1]
    yr, Jr = chain(None, syn, Z, f64)
    y, J = chain(layer, syn, Z, f32)
    ey = np.abs(y - yr).max(axis=0) / np.abs(yr).max(axis=0)
    eJ = np.abs(J - Jr).reshape(-1, n).max(axis=0) / np.abs(Jr).reshape(-1, n).max(axis=0)
    return float(eJ.max()), float(ey.max())


@pytest.mark.parametrize("net_seed,in_seed", [(42, 7), (1, 2), (3, 4), (5, 6), (8, 9)])
def test_f16_route_emulated_against_float64(net_seed, in_seed):
    syn = MlpData.synthetic((128, 128, 128, 128), seed=net_seed)
    Z = (np.random.default_rng(in_seed).normal(size=(5, 2048)) * 1.5).astype(f32)
    rJ, ry = chain_errors(layer_fp32, syn, Z)
    eJ, ey = chain_errors(layer_f16("keep"), syn, Z)
    print(f"seeds {net_seed}/{in_seed}: fp32 chain J {rJ:.2e} y {ry:.2e}; f16 two planes J {eJ:.2e} y {ey:.2e}")
    assert eJ <= 3.0 * rJ and ey <= 3.0 * ry, (eJ / rJ, ey / ry)
    assert eJ < 1e-6 and ey < 1e-6


def test_inconsistent_flush_is_flagged():
    """A matrix core that flushed subnormal inputs beside a vector ALU that keeps them would break the route; the same
    bounds catch it.  (The consistent flush stays inside them: it is the split that must agree with the matrix core.)"""
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    Z = (np.random.default_rng(7).normal(size=(5, 2048)) * 1.5).astype(f32)
    rJ, ry = chain_errors(layer_fp32, syn, Z)
    bJ, by = chain_errors(layer_f16("inconsistent"), syn, Z)
    cJ, cy = chain_errors(layer_f16("flush"), syn, Z)
    print(f"inconsistent flush J {bJ:.2e} y {by:.2e}; consistent flush J {cJ:.2e} y {cy:.2e}")
    assert bJ > 3.0 * rJ or by > 3.0 * ry or bJ >= 1e-6 or by >= 1e-6
    assert cJ < 1e-6 and cy < 1e-6


# ---- the range gate -----------------------------------------------------------------------------------------------------
def gate(lib, Ws, bs):
    Ws = [np.ascontiguousarray(W, dtype=f32) for W in Ws]
    bs = [np.ascontiguousarray(b, dtype=f32) for b in bs]
    widths = (C.c_int * (len(Ws) + 1))(Ws[0].shape[1], *[W.shape[0] for W in Ws])
    pw = (C.c_void_p * len(Ws))(*[W.ctypes.data for W in Ws])
    pb = (C.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
    worst = C.c_double()
    return lib.host_f16_gate(len(Ws), widths, pw, pb, C.byref(worst)), worst.value


def test_gate_accepts_the_headline_nets_and_rejects_out_of_range_ones(lib):
    OK, WEIGHT, BOUND, TINY = 0, 1, 2, 3
    for seed in (42, 17):
        syn = MlpData.synthetic((128, 128, 128, 128), seed=seed)
        assert gate(lib, syn.weights, syn.biases)[0] == OK
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    W = [w.copy() for w in syn.weights]
    W[2] = W[2] * f32(1024.0)                       # one hidden layer scaled by 2^10: the tangents may overflow
    assert gate(lib, W, syn.biases)[0] == BOUND
    W = [w.copy() for w in syn.weights]
    W[1][3, 5] = f32(40000.0)                       # a weight above 2^15
    assert gate(lib, W, syn.biases)[0] == WEIGHT
    W = [w.copy() for w in syn.weights]
    W[0] = W[0] * f32(2.0 ** -20)                   # uniformly tiny tangents: f16's subnormal range
    assert gate(lib, W, syn.biases)[0] == TINY
