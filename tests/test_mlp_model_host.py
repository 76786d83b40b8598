"""The host-side MLP model builder (aircraft_amd/csrc/ac_mlp_model.hpp, compiled with g++ here): what ac_set_mlp uploads and
hands to the kernels — the folded net, the packed blob, the seven LDS plans and the vector-ALU image.  No GPU.

Every check is written from the layouts the kernels read (DESIGN.md §4.3 and the header comments), with the inverse layouts
in NumPy, and every comparison is exact.

The LDS rule's rejection ("MLP does not fit the LDS plan"): no net inside AC_MAX_WIDTH = 128 and AC_MAX_LAYERS = 8 reaches
it — the hidden blocks are one size class (66 560 B at width 128) and always stream, which leaves at most 12 288 + 9 216 B
resident beside the 2 x 66 560 B ring (test_lds_rule_is_unreachable_inside_the_width_limit counts every case).  The rule
itself is therefore driven through plan_lds directly, with the block sizes a 5-256-256-6 net would have."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import golden
from tests.rollout_matrix import MLP_ROW_IDS, MLP_ROWS, mlp_data

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_mlp", "mlp_model_host.cpp")
f32, f64 = np.float32, np.float64
MAXL, LDS = 8, 160 * 1024
AC_OK, AC_ERR_BAD_ARG, AC_ERR_UNSUPPORTED = 0, -1, -3
PLAN = np.dtype([("n_layers", "i4"), ("KT", "i4", MAXL), ("NT", "i4", MAXL), ("act", "i4", MAXL), ("g_off", "i4", MAXL),
                 ("bytes", "i4", MAXL), ("lds_off", "i4", MAXL), ("ring_off", "i4", 2), ("n_streamed", "i4"),
                 ("first_streamed", "i4"), ("streamed", "i4", MAXL), ("lds_total", "i4"), ("bf_region", "i4", 3)])
VPLAN = np.dtype([("n_layers", "i4"), ("act_last", "i4"), ("w_off", "i4", MAXL), ("b_off", "i4", MAXL), ("image_floats", "i4")])
PLAN_NAMES = ["plan", "plan_sens", "plan_rev", "plan_bf", "plan_bf_pair", "plan_f16", "plan_f16_pair"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mlp") / "libmlp_model_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC], check=True)
    L = C.CDLL(so)
    L.host_mlp_build.restype = C.c_void_p
    L.host_mlp_build.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.host_mlp_free.argtypes = [C.c_void_p]
    L.host_mlp_rc.argtypes = [C.c_void_p]
    L.host_mlp_err.argtypes = [C.c_void_p]
    L.host_mlp_err.restype = C.c_char_p
    L.host_mlp_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.host_mlp_vplan.argtypes = [C.c_void_p, C.c_void_p]
    L.host_mlp_scalars.argtypes = [C.c_void_p, C.c_void_p]
    for f in (L.host_mlp_blob, L.host_mlp_vimage):
        f.restype = C.c_long
        f.argtypes = [C.c_void_p, C.c_void_p]
    L.host_mlp_folded_shape.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in (L.host_mlp_folded_W, L.host_mlp_folded_b):
        f.restype = C.POINTER(C.c_float)
        f.argtypes = [C.c_void_p, C.c_int]
    for f in (L.host_mlp_bf16_pack_layer, L.host_mlp_f16_pack_layer):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.host_mlp_f16_gate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.host_mlp_plan_lds.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    assert L.host_mlp_plan_ints() * 4 == PLAN.itemsize and L.host_mlp_vplan_ints() * 4 == VPLAN.itemsize
    return L


class Model:
    """One build_mlp_model call, copied out of the harness."""

    def __init__(self, lib, Ws, bs, act, use_mfma):
        Ws = [np.ascontiguousarray(W, dtype=f32) for W in Ws]
        bs = [np.ascontiguousarray(b, dtype=f32) for b in bs]
        n = len(Ws)
        widths = (C.c_int * (n + 1))(Ws[0].shape[1], *[W.shape[0] for W in Ws])
        pw = (C.c_void_p * n)(*[W.ctypes.data for W in Ws])
        pb = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
        h = lib.host_mlp_build(n, widths, (C.c_int * n)(*act), pw, pb, use_mfma)
        try:
            self.rc, self.err = lib.host_mlp_rc(h), lib.host_mlp_err(h).decode()
            if self.rc != AC_OK:
                return
            for i, name in enumerate(PLAN_NAMES):
                p = np.zeros(1, PLAN)
                lib.host_mlp_plan(h, i, p.ctypes.data)
                setattr(self, name, p[0])
            vp = np.zeros(1, VPLAN)
            lib.host_mlp_vplan(h, vp.ctypes.data)
            self.vplan = vp[0]
            s = np.zeros(9, np.int32)
            lib.host_mlp_scalars(h, s.ctypes.data)
            (self.wt, self.use_mfma, self.has_bf, self.f16_gate, self.has_rev, self.rev_layers, self.has_vplan, self.vwidth,
             self.n) = (int(v) for v in s)
            ptr = C.POINTER(C.c_float)()
            nb = lib.host_mlp_blob(h, C.byref(ptr))
            self.blob = np.ctypeslib.as_array(ptr, (nb,)).copy()
            nv = lib.host_mlp_vimage(h, C.byref(ptr))
            self.vimage = np.ctypeslib.as_array(ptr, (nv,)).copy() if nv else np.zeros(0, f32)
            w, a = np.zeros(self.n + 1, np.int32), np.zeros(self.n, np.int32)
            lib.host_mlp_folded_shape(h, w.ctypes.data, a.ctypes.data)
            self.widths, self.act = [int(v) for v in w], [int(v) for v in a]
            self.W = [np.ctypeslib.as_array(lib.host_mlp_folded_W(h, l), (self.widths[l + 1], self.widths[l])).copy() for l in range(self.n)]
            self.b = [np.ctypeslib.as_array(lib.host_mlp_folded_b(h, l), (self.widths[l + 1],)).copy() for l in range(self.n)]
        finally:
            lib.host_mlp_free(h)


def random_net(hidden, seed, act=None):
    rng = np.random.default_rng(seed)
    widths = [5] + list(hidden) + [6]
    Ws = [rng.uniform(-1, 1, (widths[i + 1], widths[i])).astype(f32) / f32(np.sqrt(widths[i])) for i in range(len(widths) - 1)]
    bs = [rng.uniform(-1, 1, widths[i + 1]).astype(f32) / f32(np.sqrt(widths[i])) for i in range(len(widths) - 1)]
    return Ws, bs, act if act is not None else [1] * len(hidden) + [0]


def checkpoint_net():
    w = golden("scaledmodel_weights.npz")
    return [w["W0"], w["W1"], w["W2"]], [w["b0"], w["b1"], w["b2"]], [0, 1, 0]  # 5-16-32-6, activation-free first layer


NETS = {
    "checkpoint": (checkpoint_net, [5, 32, 6]),
    "2x32": (lambda: random_net((32, 32), 1), [5, 32, 32, 6]),
    "3x64": (lambda: random_net((64, 64, 64), 2), [5, 64, 64, 64, 6]),
    "1x128": (lambda: random_net((128,), 3), [5, 128, 6]),
    "2x128": (lambda: random_net((128, 128), 4), [5, 128, 128, 6]),
    "4x128": (lambda: random_net((128, 128, 128, 128), 5), [5, 128, 128, 128, 128, 6]),
    "3x100": (lambda: random_net((100, 100, 100), 6), [5, 100, 100, 100, 6]),
    "single": (lambda: random_net((), 7), [5, 6]),
    "two_linear": (lambda: random_net((8, 12, 24), 8, act=[0, 0, 1, 0]), [5, 24, 6]),  # two consecutive activation-free layers
}
CASES = [("checkpoint", 1), ("checkpoint", 0), ("2x32", 0), ("2x32", 1), ("3x64", 0), ("3x64", 1), ("1x128", 1), ("2x128", 1),
         ("2x128", 0), ("4x128", 1), ("3x100", 1), ("single", 1), ("single", 0), ("two_linear", 1), ("two_linear", 0)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-mfma{c[1]}")
def built(request, lib):
    name, mf = request.param
    Ws, bs, act = NETS[name][0]()
    m = Model(lib, Ws, bs, act, mf)
    assert m.rc == AC_OK, m.err
    return name, mf, (Ws, bs, act), m


# ---- the fold ---------------------------------------------------------------------------------------------------------------
def fold64(Ws, bs, act):
    """W2 (W1 x + b1) + b2 = (W2 W1) x + (W2 b1 + b2) in float64, terms added in ascending order of the inner index."""
    net = [[W.astype(f64), b.astype(f64), int(bool(a))] for W, b, a in zip(Ws, bs, act)]
    l = 0
    while l + 1 < len(net):
        if net[l][2]:
            l += 1
            continue
        (Wa, ba, _), (Wb, bb, ab) = net[l], net[l + 1]
        M, mb = np.zeros((Wb.shape[0], Wa.shape[1])), bb.copy()
        for k in range(Wb.shape[1]):
            M += Wb[:, k:k + 1] * Wa[k:k + 1, :]
            mb += Wb[:, k] * ba[k]
        net[l:l + 2] = [[M, mb, ab]]
    return [n[0].astype(f32) for n in net], [n[1].astype(f32) for n in net], [n[2] for n in net]


def test_fold(built):
    name, mf, (Ws, bs, act), m = built
    fW, fb, fact = fold64(Ws, bs, act)
    assert m.widths == NETS[name][1] and m.act == fact and m.n == len(fW)
    assert all(a == 1 for a in m.act[:-1])  # tanh on every layer but the last
    for l in range(m.n):
        assert np.array_equal(m.W[l].view(np.uint32), fW[l].view(np.uint32)) and np.array_equal(m.b[l].view(np.uint32), fb[l].view(np.uint32))
    assert m.use_mfma == mf and m.rev_layers == m.n
    maxh = max(m.widths[1:-1], default=0)
    assert m.wt == (2 if maxh <= 32 else 4 if maxh <= 64 else 8)
    assert m.has_bf == (m.wt == 8 and m.n >= 3)


# ---- the blocks, read back through the plans ------------------------------------------------------------------------------
def pad(M, rows, cols):
    out = np.zeros((rows, cols), f32)
    out[:M.shape[0], :M.shape[1]] = M
    return out


def unfrag(block, NT, KT):
    """MFMA fragment order [nt][kt][lane][4]: lane = col + 16 g holds M[16 nt + col][16 kt + 4 g + j]."""
    fr = block.reshape(NT, KT, 4, 16, 4)  # nt, kt, g, col, j
    return fr.transpose(0, 3, 1, 2, 4).reshape(16 * NT, 16 * KT)


def unwlt(block, wt):
    """[tile][lane group][kp][rp] float4 = {W(2kp, n), W(2kp+1, n), W(2kp, n+1), W(2kp+1, n+1)}, n = 16 t + 4 g + 2 rp."""
    q = block[:wt * 96].reshape(wt, 4, 3, 2, 2, 2)  # t, g, kp, rp, dn, dk
    return q.transpose(2, 5, 0, 1, 3, 4).reshape(6, 16 * wt)  # row 2 kp + dk, column 16 t + 4 g + 2 rp + dn


def block_of(m, plan, l):
    return m.blob[plan["g_off"][l]:plan["g_off"][l] + plan["bytes"][l] // 4]


def eq(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_bias_piece(piece, b, n):
    assert piece.size == 256 and eq(piece, pad(b[None, :], 1, 256)[0]) and n <= 256


def test_plan_blocks_hold_the_folded_net(built):
    _, _, _, m = built
    n, wt, last, p = m.n, m.wt, m.n - 1, m.plan
    wlt_floats = -(-wt * 384 // 1024) * 256
    assert p["n_layers"] == n
    for l in range(n):
        KT, NT = int(p["KT"][l]), int(p["NT"][l])
        assert KT == (1 if l == 0 else wt) and NT == (1 if l == last else wt) and p["act"][l] == m.act[l]
        blk = block_of(m, p, l)
        frag = NT * KT * 256
        assert eq(unfrag(blk[:frag], NT, KT), pad(m.W[l], 16 * NT, 16 * KT))
        check_bias_piece(blk[frag:frag + 256], m.b[l], 16 * NT)
        tail = blk[frag + 256:]
        if l == 0 and n > 1:  # W0 transposed [5][16 wt], whole 1-KiB pieces
            assert tail.size == -(-5 * wt * 64 // 1024) * 256
            assert eq(tail[:5 * 16 * wt].reshape(5, 16 * wt), pad(m.W[0].T, 5, 16 * wt)) and not tail[5 * 16 * wt:].any()
        else:
            assert tail.size == 0
        if l == last and n > 1:  # wlt follows the last block in the blob
            wl = m.blob[p["g_off"][l] + p["bytes"][l] // 4:][:wlt_floats]
            assert eq(unwlt(wl, wt), pad(m.W[l], 6, 16 * wt)) and not wl[wt * 96:].any()
    # plan_sens: edge blocks without their fragments — [bias][W0 transposed] and [bias][wlt]; hidden blocks as in plan
    s = m.plan_sens
    if n == 1:
        assert s.tobytes() == p.tobytes()
    else:
        assert s["n_layers"] == n
        for f in ("KT", "NT", "act"):
            assert np.array_equal(s[f], p[f])
        b0, bl = block_of(m, s, 0), block_of(m, s, last)
        check_bias_piece(b0[:256], m.b[0], 16 * wt)
        assert eq(b0[256:256 + 5 * 16 * wt].reshape(5, 16 * wt), pad(m.W[0].T, 5, 16 * wt)) and not b0[256 + 5 * 16 * wt:].any()
        assert b0.size == 256 + -(-5 * wt * 64 // 1024) * 256
        check_bias_piece(bl[:256], m.b[last], 16)
        assert bl.size == 256 + wlt_floats and eq(unwlt(bl[256:], wt), pad(m.W[last], 6, 16 * wt)) and not bl[256 + wt * 96:].any()
        for l in range(1, last):
            assert s["g_off"][l] == p["g_off"][l] and s["bytes"][l] == p["bytes"][l]


def test_reverse_sweep_blocks_are_the_transposes(built):
    _, _, _, m = built
    n, wt, n_hid, r, s = m.n, m.wt, m.n - 2, m.plan_rev, m.plan_sens
    if not (wt == 8 and n_hid >= 1 and n + n_hid <= MAXL):
        assert not m.has_rev and r.tobytes() == s.tobytes()
        return
    assert r["n_layers"] == n + n_hid
    for f in ("KT", "NT", "act", "g_off", "bytes"):
        assert np.array_equal(r[f][:n], s[f][:n])
    for i in range(n_hid):  # top hidden layer first
        e, l = n + i, n_hid - i
        assert r["KT"][e] == wt and r["NT"][e] == wt and r["act"][e] == 0 and r["bytes"][e] == wt * wt * 1024 + 1024
        blk = block_of(m, r, e)
        assert eq(unfrag(blk[:wt * wt * 256], wt, wt), pad(m.W[l].T, 16 * wt, 16 * wt)) and not blk[wt * wt * 256:].any()
    # the kernel expects the hidden and the transposed blocks to stream and the edge blocks to stay
    assert m.has_rev == (r["n_streamed"] == 2 * n_hid and r["lds_off"][0] >= 0 and r["lds_off"][n - 1] >= 0)
    assert m.has_rev
    assert sorted(r["streamed"][:2 * n_hid]) == list(range(1, n - 1)) + list(range(n, n + n_hid))


def test_plane_images_and_gate(built, lib):
    _, _, _, m = built
    n, wt = m.n, m.wt
    if not m.has_bf:
        for name in PLAN_NAMES[3:]:
            assert getattr(m, name).tobytes() == m.plan_sens.tobytes()
        assert m.f16_gate == 0
        return
    for plan, nbytes, pack in ((m.plan_bf, lib.host_mlp_bf16_layer_bytes(wt), lib.host_mlp_bf16_pack_layer),
                               (m.plan_f16, lib.host_mlp_f16_layer_bytes(wt), lib.host_mlp_f16_pack_layer)):
        for l in (0, n - 1):  # the edge blocks of plan_sens
            assert plan["g_off"][l] == m.plan_sens["g_off"][l] and plan["bytes"][l] == m.plan_sens["bytes"][l]
        for l in range(1, n - 1):
            img = np.zeros(nbytes, np.uint8)
            W, b = np.ascontiguousarray(m.W[l]), np.ascontiguousarray(m.b[l])
            pack(W.ctypes.data, b.ctypes.data, m.widths[l], m.widths[l + 1], wt, img.ctypes.data)
            assert plan["bytes"][l] == nbytes and block_of(m, plan, l).tobytes() == img.tobytes()
    widths = (C.c_int * (n + 1))(*m.widths)
    Ws, bs = [np.ascontiguousarray(W) for W in m.W], [np.ascontiguousarray(b) for b in m.b]
    pw = (C.c_void_p * n)(*[W.ctypes.data for W in Ws])
    pb = (C.c_void_p * n)(*[b.ctypes.data for b in bs])
    assert m.f16_gate == lib.host_mlp_f16_gate(n, widths, pw, pb)


def test_blob_regions_tile_the_blob(built):
    _, _, _, m = built
    n, wt = m.n, m.wt
    spans = [(int(m.plan["g_off"][l]), int(m.plan["bytes"][l]) // 4) for l in range(n)]
    if n > 1:
        spans.append((int(m.plan_sens["g_off"][n - 1]) + 256, -(-wt * 384 // 1024) * 256))  # wlt
    if m.has_rev:
        spans += [(int(m.plan_rev["g_off"][e]), int(m.plan_rev["bytes"][e]) // 4) for e in range(n, 2 * n - 2)]
    if m.has_bf:
        spans += [(int(p["g_off"][l]), int(p["bytes"][l]) // 4) for p in (m.plan_bf, m.plan_f16) for l in range(1, n - 1)]
    spans.sort()
    assert spans[0][0] == 0 and all(a + na == b for (a, na), (b, _) in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == m.blob.size


# ---- the LDS plans ------------------------------------------------------------------------------------------------------------
def disjoint_inside(spans, total):
    spans = sorted(spans)
    assert all(a >= 0 and a + na <= total for a, na in spans)
    assert all(a + na <= b for (a, na), (b, _) in zip(spans, spans[1:]))


def test_lds_plans(built, lib):
    _, _, _, m = built
    for name in PLAN_NAMES:
        p = getattr(m, name)
        nl = int(p["n_layers"])
        ring = name in ("plan", "plan_sens", "plan_rev") or not m.has_bf
        by, off = p["bytes"][:nl], p["lds_off"][:nl]
        assert (by % 1024 == 0).all() and p["lds_total"] % 1024 == 0 and 0 < p["lds_total"] <= LDS
        assert ((off % 1024 == 0) | (off == -1)).all()
        streamed = [l for l in range(nl) if off[l] < 0]
        assert p["n_streamed"] == len(streamed) and list(p["streamed"][:len(streamed)]) == streamed
        assert p["first_streamed"] == (streamed[0] if streamed else -1)
        spans = [(int(off[l]), int(by[l])) for l in range(nl) if off[l] >= 0]
        if ring:
            if streamed:
                big = int(by.max())
                assert streamed == [l for l in range(nl) if by[l] == big] and (p["ring_off"] % 1024 == 0).all()
                spans += [(int(p["ring_off"][0]), big), (int(p["ring_off"][1]), big)]
                assert p["lds_total"] == sum(na for _, na in spans)
            else:
                assert p["lds_total"] == by.sum() and by.sum() <= LDS
            # streams only what it must (plan_rev: always, the kernel sequences its blocks through the ring by hand)
            assert bool(streamed) == (by.sum() > LDS or (name == "plan_rev" and m.has_rev))
        else:
            planes = 3 if "bf" in name else 2
            region = (m.wt // 2) ** 2 * planes * 1024 + 1024  # a half layer: front fragments + the bias piece
            assert streamed == list(range(1, m.n - 1)) and p["first_streamed"] == 1 and (p["ring_off"] == -1).all()
            nreg = 2 if name.endswith("_pair") else 3
            assert (p["bf_region"][:nreg] % 1024 == 0).all() and (p["bf_region"][nreg:] == -1).all()
            spans += [(int(r), region) for r in p["bf_region"][:nreg]]
            assert (by[1:m.n - 1] == 2 * region - 1024).all()
            assert p["lds_total"] == sum(na for _, na in spans)
        disjoint_inside(spans, int(p["lds_total"]))
    if m.has_bf:  # the pair plans: their parents minus the third region
        for parent, pair in ((m.plan_bf, m.plan_bf_pair), (m.plan_f16, m.plan_f16_pair)):
            want = parent.copy()
            want["lds_total"] = parent["bf_region"][2]
            want["bf_region"][2] = -1
            assert pair.tobytes() == want.tobytes()
            assert parent["lds_total"] - pair["lds_total"] == parent["bf_region"][1] - parent["bf_region"][0]


# ---- the vector-ALU image ----------------------------------------------------------------------------------------------------
def test_valu_image(built):
    _, mf, _, m = built
    maxh = max(m.widths[1:-1], default=0)
    assert m.vwidth == (32 if maxh <= 32 else 64)
    assert m.has_vplan == (not mf and m.n >= 2 and maxh <= 64)
    v = m.vplan
    if not m.has_vplan:
        assert m.vimage.size == 0 and v.tobytes() == np.zeros(1, VPLAN).tobytes()
        return
    vw, n = m.vwidth, m.n
    assert v["n_layers"] == n and v["act_last"] == m.act[-1]
    assert v["image_floats"] % 256 == 0 and m.vimage.size == v["image_floats"] and v["image_floats"] * 4 + 4 * 96 * (vw + 4) * 4 <= LDS
    want, off = np.zeros(m.vimage.size, f32), 0
    for l in range(n):
        K, N = (8 if l == 0 else vw), (8 if l == n - 1 else vw)
        assert v["w_off"][l] == off
        if l == n - 1:  # transposed: [8][K + 4], padded rows
            want[off:off + N * (K + 4)] = pad(m.W[l], N, K + 4).ravel()
            off += N * (K + 4)
        else:           # k-major [K][N]
            want[off:off + K * N] = pad(m.W[l].T, K, N).ravel()
            off += K * N
        assert v["b_off"][l] == off
        want[off:off + m.widths[l + 1]] = m.b[l]
        off += N
    assert off <= m.vimage.size < off + 256 and eq(m.vimage, want)


# ---- the rollout-engine matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", MLP_ROWS, ids=MLP_ROW_IDS)
def test_rollout_matrix_rows_reach_the_instance_they_claim(lib, row):
    """tests/rollout_matrix.py names one net per rollout-engine instance; the host picks the instance from wt, the number of
    folded layers and (for the cooperative engine's weight ring) plan.n_streamed.  Pinned here, so that a change of the fold
    or of the LDS rule cannot take an instance — the ring above all — out of tests/test_gpu_rollout_engines.py unnoticed."""
    md = mlp_data(row)
    m = Model(lib, md.weights, md.biases, md.act, int(row.use_mfma))
    assert m.rc == AC_OK, m.err
    assert (m.wt, m.n, int(m.plan["n_streamed"])) == (row.wt, row.layers, row.n_streamed)
    assert int(m.plan["n_layers"]) == m.n and m.use_mfma == int(row.use_mfma)
    # the dispatch of ac_rollout_f32 / ac_rollout_policy_f32, restated
    nh = m.n - 2
    if not row.use_mfma:
        want = ("k_nn_rollout_tiled8", "k_nn_rollout_policy_tiled8") if m.has_vplan else ("k_nn_rollout", None)
        assert not m.has_vplan or m.vwidth == (32 if row.wt == 2 else 64)
    elif 1 <= nh <= 3:
        want = ("k_nn_rollout_reg", "k_nn_rollout_policy_reg")
    else:
        want = ("k_nn_rollout_coop", "k_nn_rollout_policy_coop")
    assert (row.open_kernel, row.policy_kernel) == want
    if row.n_streamed:  # the hidden x hidden blocks stream, the edge blocks stay
        assert list(m.plan["streamed"][:row.n_streamed]) == list(range(1, m.n - 1))
    if row.act is not None and row.act[-1]:
        assert m.act[-1] == 1  # the tanh on the output layer survives the fold


def test_rollout_matrix_covers_every_instance():
    """3 x 3 register-engine instances, the three cooperative widths with and without hidden x hidden layers, an even and an
    odd number of streamed layers, the one-layer net, both tiled widths, and the sequential vector-ALU kernel."""
    reg = {(r.wt, r.layers - 2) for r in MLP_ROWS if r.open_kernel == "k_nn_rollout_reg"}
    assert reg == {(wt, nh) for wt in (2, 4, 8) for nh in (1, 2, 3)}
    coop = [r for r in MLP_ROWS if r.open_kernel == "k_nn_rollout_coop"]
    assert {r.wt for r in coop} == {2, 4, 8} and {r.layers for r in coop} >= {1, 2, 6, 7}
    assert sorted(r.n_streamed for r in coop if r.n_streamed) == [4, 5]  # the ring runs in these two rows only
    assert {r.wt for r in MLP_ROWS if r.open_kernel == "k_nn_rollout_tiled8"} == {2, 4}
    assert [r.wt for r in MLP_ROWS if r.open_kernel == "k_nn_rollout"] == [8]
    assert any(r.hidden is not None and len(set(r.hidden)) > 1 for r in MLP_ROWS if r.wt == 8)  # ragged widths at width 128
    assert len(set(MLP_ROW_IDS)) == len(MLP_ROWS)


# ---- error paths ------------------------------------------------------------------------------------------------------------
def test_width_limit(lib):
    Ws, bs, act = random_net((129,), 9)
    m = Model(lib, Ws, bs, act, 1)
    assert m.rc == AC_ERR_UNSUPPORTED and m.err == "MLP width 129 > AC_MAX_WIDTH 128"
    Ws, bs, act = random_net((16,), 9)
    assert Model(lib, [Ws[0], Ws[1][:5]], [bs[0], bs[1][:5]], act, 1).rc == AC_ERR_BAD_ARG  # five outputs
    assert Model(lib, Ws * 5, bs * 5, act * 5, 1).rc == AC_ERR_BAD_ARG                       # ten layers


def net_plan(wt, n):
    """Block sizes of an n-layer net of wt tiles, as `plan` has them."""
    p = np.zeros(1, PLAN)
    p["n_layers"] = n
    for l in range(n):
        KT, NT = (1 if l == 0 else wt), (1 if l == n - 1 else wt)
        p["bytes"][0, l] = NT * KT * 1024 + 1024 + (-(-5 * wt * 64 // 1024) * 1024 if l == 0 and n > 1 else 0)
    return p


def rejected(by):
    """the rule: everything resident if it fits, else the largest size class through a two-slot ring beside the rest"""
    big = max(by)
    return sum(by) > LDS and sum(b for b in by if b < big) + 2 * big > LDS


def test_lds_rule_rejects_what_does_not_fit(lib):
    p = net_plan(16, 3)  # 5-256-256-6: a hidden block of 16 x 16 KiB + 1 KiB
    by = [int(b) for b in p["bytes"][0, :3]]
    big, resident = max(by), sum(b for b in by if b < max(by))
    assert rejected(by) and big == 263168 and resident == 22528 + 17408
    err = C.create_string_buffer(512)
    assert lib.host_mlp_plan_lds(p.ctypes.data, 0, err, 512) == AC_ERR_UNSUPPORTED
    assert err.value.decode() == f"MLP does not fit the LDS plan ({resident} resident + 2 x {big} ring)"


def test_lds_rule_is_unreachable_inside_the_width_limit(lib):
    err = C.create_string_buffer(512)
    for wt in (2, 4, 8):
        for n in range(1, MAXL + 1):
            p = net_plan(wt, n)
            assert not rejected([int(b) for b in p["bytes"][0, :n]])
            assert lib.host_mlp_plan_lds(p.ctypes.data, 0, err, 512) == AC_OK and p["lds_total"][0] <= LDS
