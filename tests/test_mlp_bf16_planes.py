"""The host side of the bf16 hidden layers (aircraft_amd/csrc/ac_bf16_pack.hpp, compiled with g++ here): the three-plane
split is exact, the packed image unpacks to W bit for bit (the k permutation included), and a NumPy emulation of the kernel's
product order (MlpEngine::layer_bf) stays within 2e-6 of float64.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from aircraft_amd.utils import MlpData
from tests.helpers import golden

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_bf16", "bf16_pack_host.cpp")
HDR = os.path.join(HERE, "..", "aircraft_amd", "csrc", "ac_bf16_pack.hpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bf16") / "libbf16_pack_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.host_bf16_layer_bytes.restype = C.c_int
    L.host_bf16_front_bytes.restype = C.c_int
    L.host_bf16_split3.argtypes = [C.c_void_p, C.c_long, C.c_void_p]
    L.host_bf16_pack_layer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint32) << 16).view(np.float32)


def split3(lib, w):
    w = np.ascontiguousarray(w, dtype=np.float32).ravel()
    p = np.zeros((w.size, 3), dtype=np.uint16)
    lib.host_bf16_split3(w.ctypes.data, w.size, p.ctypes.data)
    return p


def bf16_rne_np(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def split3_np(x):  # the kernel's activation split (v_cvt_pk_bf16_f32 rounds to nearest even)
    p1 = bf16_rne_np(x)
    r = (x - bf16_to_f32(p1)).astype(np.float32)
    p2 = bf16_rne_np(r)
    r = (r - bf16_to_f32(p2)).astype(np.float32)
    return [bf16_to_f32(p1), bf16_to_f32(p2), bf16_to_f32(bf16_rne_np(r))]


def chunk_row(c, kk):
    g, q = kk >> 3, kk & 7
    return 32 * c + (16 if q & 4 else 0) + 4 * g + (q & 3)


def unpack(img, wt, nin, nout):
    """Inverse of bf16_pack_layer, written independently: (W [nout][nin], b [nout])."""
    half, kc = wt // 2, wt // 2
    front = (half * kc * 3 + 1) * 1024
    raw = np.frombuffer(img, dtype=np.uint8)
    W = np.zeros((16 * wt, 16 * wt), dtype=np.float32)
    for nt in range(wt):
        base = 0 if nt < half else front
        for c in range(kc):
            pl = []
            for p in range(3):
                off = base + (((nt % half) * kc + c) * 3 + p) * 1024
                pl.append(bf16_to_f32(raw[off:off + 1024].view(np.uint16).reshape(64, 8)))
            tot = (pl[0] + pl[1]).astype(np.float32) + pl[2]  # exact: the planes hold disjoint bits of w
            for lane in range(64):
                for q in range(8):
                    W[16 * nt + (lane & 15), chunk_row(c, 8 * (lane >> 4) + q)] = tot[lane, q]
    b = raw[half * kc * 3 * 1024:half * kc * 3 * 1024 + 64 * wt].view(np.float32)
    return W[:nout, :nin], b[:nout]


def nets():
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    w = golden("scaledmodel_weights.npz")
    return [("cfg3", syn.weights[1:-1], syn.biases[1:-1]), ("checkpoint", [w["W1"]], [w["b1"]])]


@pytest.mark.parametrize("name,Ws,bs", nets(), ids=lambda v: v if isinstance(v, str) else "")
def test_planes_sum_exactly_and_image_unpacks_bit_for_bit(lib, name, Ws, bs):
    wt = 8
    for W, b in zip(Ws, bs):
        W = np.ascontiguousarray(W, dtype=np.float32); b = np.ascontiguousarray(b, dtype=np.float32)
        p = split3(lib, W)
        f = bf16_to_f32(p)
        assert np.array_equal(((f[:, 0] + f[:, 1]) + f[:, 2]).astype(np.float32).view(np.uint32), W.ravel().view(np.uint32))
        assert np.array_equal(f[:, 0], bf16_to_f32(bf16_rne_np(W.ravel())))  # plane 1 = RNE of w
        img = np.zeros(lib.host_bf16_layer_bytes(wt), dtype=np.uint8)
        nout, nin = W.shape
        lib.host_bf16_pack_layer(W.ctypes.data, b.ctypes.data, nin, nout, wt, img.ctypes.data)
        Wu, bu = unpack(img.tobytes(), wt, nin, nout)
        assert np.array_equal(Wu.view(np.uint32), W.view(np.uint32)) and np.array_equal(bu.view(np.uint32), b.view(np.uint32))
    assert lib.host_bf16_layer_bytes(8) == 97 * 1024 and lib.host_bf16_front_bytes(8) == 49 * 1024


def test_kernel_product_order_emulated_within_2e6(lib):
    """Each 32-deep MFMA is taken as an exact sum rounded once into its fp32 accumulator: `hi` gets w1 x1, `lo` the five
    small products smallest first, the tile is hi + lo — the order of MlpEngine::layer_bf."""
    syn = MlpData.synthetic((128, 128, 128, 128), seed=42)
    rng = np.random.default_rng(3)
    worst = 0.0
    for W, b in zip(syn.weights[1:-1], syn.biases[1:-1]):
        f = bf16_to_f32(split3(lib, W)).reshape(W.shape + (3,))
        w = [f[..., i].astype(np.float64) for i in range(3)]
        X = np.tanh(rng.normal(size=(128, 256))).astype(np.float32)  # hidden activations of 256 units
        x = [v.astype(np.float64) for v in split3_np(X)]
        hi = np.broadcast_to(b.astype(np.float32)[:, None], (128, 256)).astype(np.float32)
        lo = np.zeros((128, 256), dtype=np.float32)
        for c in range(4):
            k = slice(32 * c, 32 * c + 32)
            for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1)):
                lo = (lo + w[i][:, k] @ x[j][k]).astype(np.float32)
            hi = (hi + w[0][:, k] @ x[0][k]).astype(np.float32)
        got = (hi + lo).astype(np.float64)
        ref = W.astype(np.float64) @ X.astype(np.float64) + b.astype(np.float64)[:, None]
        err = np.abs(got - ref).max(axis=0) / np.abs(ref).max(axis=0)
        worst = max(worst, float(err.max()))
    assert worst < 2e-6, worst
