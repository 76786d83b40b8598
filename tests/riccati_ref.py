"""Inputs, fp32 restatement and per-node metric for the Riccati backward kernel and the costate kernel
(aircraft_amd/csrc/ac_ilqr.hpp: k_ilqr_backward<NODE, NEWTON>, k_ilqr_costate<NODE>).  TEST INFRASTRUCTURE, NOT PRODUCT.

The reference is oracle/ilqr_oracle.py (float64).  What is new here:

 * `synthetic_riccati`: inputs in which every node of every instance differs by O(1) from its neighbours, so that a stale ring
   slot, a wrong instance column or a swapped index moves that node by O(1) and not by the smoothness of a trajectory;
 * `backward_f32` / `costate_f32`: the same recursions in np.float32 throughout.  They are never compared with the GPU: they
   measure what fp32 arithmetic costs on a case (`e32`), and the bar of the case is 8 x that (the factor this project gives
   its conditioning clauses), provided e32 <= E32_MAX, so that the bar never exceeds 1e-4 — below the 4.4e-4 that a 0.1 %
   change of `reg` produces;
 * `node_rel` / `check_riccati` / `check_costate`: the error of EVERY (node, instance), max|a - ref| / max|ref| over the
   node's entries, instead of one Frobenius norm over everything.

tests/test_riccati_ref.py checks all of this on the CPU; tests/test_gpu_riccati.py runs the matrix below on the card."""
from __future__ import annotations

import functools
import os
import re
import subprocess
import tempfile

import numpy as np

import ilqr_oracle as io
from aircraft_amd.control import QuadraticCost
from tests.helpers import f32_exact, parity_report

E32_MAX = 1.25e-5   # condition on a case's inputs: fp32 restatement vs float64, worst (node, instance)
FACTOR = 8.0        # bar = FACTOR x e32  (<= 1e-4)
QUU_MIN = 0.3       # smallest eigenvalue of the float64 Quu at every node: the kernel's fmaxf(d, 1e-12f) clamp is never in play

# The five ways the kernel is instantiated and fed: name -> (NODE, NEWTON, uglin)
VARIANTS = {
    "gn": (False, False, False),            # <false, false>
    "node": (True, False, False),           # <true, false>
    "newton": (False, True, False),         # <false, true>
    "node_newton": (True, True, False),     # <true, true>, uglin == nullptr (ac_ilqr_backward_newton_f32)
    "goal": (True, True, True),             # <true, true> with uglin (ac_ilqr_backward_goal_f32)
}
PARENT_B = 7    # odd stride
WIDE_B = 65     # the parent of the sub-batch comparisons, at H = kDepth + 1 only
COSTATE_BLOCK = 256   # kBlock of ac_kernels_analytic.hpp: lanes per workgroup of k_ilqr_costate


def k_depth(newton):
    """IlqrRing<NODE, NEWTON>::kDepth: nodes in flight (the ring is shallower when the 21 x 21 blocks travel too)."""
    return 5 if newton else 8


def ring_lds_bytes(newton, shoot=False, rate=False):
    """LDS of one backward kernel from the constants of IlqrRing<NODE, NEWTON, SHOOT, RATE> (ac_ilqr.hpp):
    4 x (kWork + kDepth x kNodeFloats) — the work area, then the node ring."""
    work = 944 if rate else 736
    node_floats = (776 if newton else 336) if rate else (768 if newton else 320) + (26 if shoot else 0)
    return 4 * (work + k_depth(newton) * node_floats)


@functools.lru_cache(maxsize=None)
def backward_unit_resources():
    """The compiler's resource remarks for csrc/ilqr_backward_inst.hip, the unit of all 24 backward kernels, compiled ONCE per
    test run with the flags of the build -> {mangled name: dict(family, node, newton, box, vgpr, scratch, lds)}."""
    from aircraft_amd import build as B

    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc", *B.CFLAGS, *B.UNIT_FLAGS.get("ilqr_backward_inst", []), "-S", "--cuda-device-only",
               "-Rpass-analysis=kernel-resource-usage", os.path.join(B.CSRC, "ilqr_backward_inst.hip"), "-o", os.path.join(tmp, "backward.s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        name = b.split("\n")[0].split()[0]
        m = re.match(r"_ZN2ac\d+k_ilqr_backward(_shoot|_rate|)ILb([01])ELb([01])ELb([01])EE", name)
        if m:
            out[name] = dict(family=m.group(1).lstrip("_"), node=m.group(2) == "1", newton=m.group(3) == "1", box=m.group(4) == "1",
                             vgpr=int(re.search(r"VGPRs: (\d+)", b).group(1)),
                             scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)),
                             lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    return out


def horizons(newton):
    """never full (1, 2, kDepth-1), exactly full without a refill, the first refill, the first slot reused twice (2 kDepth-1,
    2 kDepth, 2 kDepth+1), and a long run where it % kDepth wraps with an odd remainder"""
    d = k_depth(newton)
    return sorted({1, 2, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 23})


def matrix():
    """[(variant, B, H)]: every variant at every horizon with the parent batch, and the wide parent at H = kDepth + 1."""
    rows = []
    for v, (_, newton, _) in VARIANTS.items():
        rows += [(v, PARENT_B, H) for H in horizons(newton)]
        rows.append((v, WIDE_B, k_depth(newton) + 1))
    return rows


def synthetic_riccati(B, H, seed, node=False, newton=False, uglin=False):
    """Per-node-distinct inputs, all rounded to float32 and returned as float64.  The draws do not depend on the switches:
    the same (B, H, seed) gives the same A, Bm, X, U, cost to every variant.
    -> dict(cost, X, U, A, Bm, node, Hz, uglin); node = (q, xref, glin) or None."""
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.normal(size=s)  # noqa: E731
    A = f32_exact(np.eye(13)[None, :, :, None] + 0.05 * n(H, 13, 13, B))
    Bm = f32_exact(0.1 * n(H, 13, 7, B))
    X = f32_exact(n(H + 1, 13, B)); U = f32_exact(n(H, 7, B))
    f = lambda a: [float(v) for v in f32_exact(a)]  # noqa: E731
    cost = QuadraticCost(q=f(rng.uniform(0.2, 2, 13)), qf=f(rng.uniform(0.5, 3, 13)), r=f(rng.uniform(0.3, 1, 7)),
                         x_ref=f(n(13)), x_goal=f(n(13)), reg=0.25, u_lin=f(0.3 * n(7)))
    nq = f32_exact(rng.uniform(0.2, 2, (H + 1, 13, B))); nx = f32_exact(n(H + 1, 13, B)); ng = f32_exact(0.5 * n(H + 1, 13, B))
    S = 0.03 * n(H, 21, 21, B)
    Hz = f32_exact(S + S.transpose(0, 2, 1, 3))   # symmetric, indefinite, the dt row and column (20) filled too
    ug = f32_exact(0.5 * n(H, 7, B))
    return dict(cost=cost, X=X, U=U, A=A, Bm=Bm, node=(nq, nx, ng) if node else None, Hz=Hz if newton else None,
                uglin=ug if uglin else None)


def columns(inp, sl):
    """the same inputs restricted to the instance columns `sl` (a slice)"""
    cut = lambda a: None if a is None else np.ascontiguousarray(a[..., sl])  # noqa: E731
    return dict(cost=inp["cost"], X=cut(inp["X"]), U=cut(inp["U"]), A=cut(inp["A"]), Bm=cut(inp["Bm"]),
                node=None if inp["node"] is None else tuple(cut(a) for a in inp["node"]), Hz=cut(inp["Hz"]),
                uglin=cut(inp["uglin"]))


def reference(inp):
    return io.backward(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"], uglin=inp["uglin"])


def _bt(a):
    """(..., B) -> (B, ...)"""
    return np.moveaxis(a, -1, 0)


def backward_np(dtype, c, X, U, A, Bm, node=None, Hz=None, uglin=None):
    """The recursion of io.backward in `dtype` throughout (all instances at once), Quu by Cholesky plus two triangular solves,
    Quu and V symmetrised.  -> K, kff, dV, and the smallest eigenvalue of Quu over all nodes and instances."""
    t = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    H, _, B = U.shape
    q, qf, r, reg = t(c.q), t(c.qf), t(c.r), dtype(c.reg)
    ulin = t(getattr(c, "u_lin", [0.0] * 7))
    X, U, A, Bm = t(X), t(U), t(A), t(Bm)
    half = dtype(0.5)
    eye13, eye7 = np.eye(13, dtype=dtype), np.eye(7, dtype=dtype)
    T = lambda M: np.swapaxes(M, -1, -2)  # noqa: E731
    mv = lambda M, v: (M @ v[..., None])[..., 0]  # noqa: E731
    K = np.zeros((H, 7, 13, B), dtype=dtype); kff = np.zeros((H, 7, B), dtype=dtype); dV = np.zeros((2, B), dtype=dtype)
    if node is None:
        Vx = qf[None] * (_bt(X[H]) - t(c.x_goal)[None]); Vxx = np.broadcast_to(np.diag(qf), (B, 13, 13)).copy()
    else:
        nq, nx, ng = (t(a) for a in node)
        Vx = _bt(nq[H]) * (_bt(X[H]) - _bt(nx[H])) + _bt(ng[H]); Vxx = _bt(nq[H])[:, :, None] * eye13[None]
    lo = np.inf
    for k in range(H - 1, -1, -1):
        Ak, Bk = _bt(A[k]), _bt(Bm[k])              # (B, 13, 13), (B, 13, 7)
        xk, uk = _bt(X[k]), _bt(U[k])
        if node is None:
            qk = np.broadcast_to(q, (B, 13)); lx = qk * (xk - t(c.x_ref)[None])
        else:
            qk = _bt(nq[k]); lx = qk * (xk - _bt(nx[k])) + _bt(ng[k])
        lu = r[None] * uk + ulin[None]
        if uglin is not None:
            lu = lu + _bt(t(uglin)[k])
        Qx = lx + mv(T(Ak), Vx); Qu = lu + mv(T(Bk), Vx)
        VA, VB = Vxx @ Ak, Vxx @ Bk
        Qxx = qk[:, :, None] * eye13[None] + T(Ak) @ VA
        Qux = T(Bk) @ VA
        Quu = (r + reg)[None, :, None] * eye7[None] + T(Bk) @ VB
        if Hz is not None:
            Hk = _bt(t(Hz)[k])
            Qxx = Qxx + Hk[:, :13, :13]; Qux = Qux + Hk[:, 13:20, :13]; Quu = Quu + Hk[:, 13:20, 13:20]
        Quu = half * (Quu + T(Quu))
        lo = min(lo, float(np.linalg.eigvalsh(Quu.astype(np.float64)).min()))
        L = np.linalg.cholesky(Quu)
        assert L.dtype == dtype
        rhs = np.concatenate([Qux, Qu[:, :, None]], axis=2)
        sol = -np.linalg.solve(T(L), np.linalg.solve(L, rhs))   # two triangular systems
        assert sol.dtype == dtype
        Kk, kk = sol[:, :, :13], sol[:, :, 13]
        K[k] = np.moveaxis(Kk, 0, -1); kff[k] = kk.T
        Quukk = mv(Quu, kk)
        dV[0] += (kk * Qu).sum(axis=1); dV[1] += half * (kk * Quukk).sum(axis=1)
        Vx = Qx + mv(T(Kk), Quukk) + mv(T(Kk), Qu) + mv(T(Qux), kk)
        Vxx = Qxx + T(Kk) @ Quu @ Kk + T(Kk) @ Qux + T(Qux) @ Kk
        Vxx = half * (Vxx + T(Vxx))
    return K, kff, dV, lo


def backward_f32(c, X, U, A, Bm, node=None, Hz=None, uglin=None):
    """io.backward in np.float32 throughout -> K, kff, dV (float32).  Estimates what fp32 arithmetic costs on the case."""
    return backward_np(np.float32, c, X, U, A, Bm, node=node, Hz=Hz, uglin=uglin)[:3]


def quu_min_eig(inp):
    return backward_np(np.float64, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"],
                       uglin=inp["uglin"])[3]


def costate_f32(c, X, A, node=None):
    """io.costate in np.float32 throughout -> (H, 13, B) float32."""
    t = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    H, B = A.shape[0], A.shape[3]
    X, A = t(X), t(A)
    Lam = np.zeros((H, 13, B), dtype=np.float32)
    if node is None:
        lam = t(c.qf)[:, None] * (X[H] - t(c.x_goal)[:, None])
    else:
        nq, nx, ng = (t(a) for a in node)
        lam = nq[H] * (X[H] - nx[H]) + ng[H]
    for k in range(H - 1, -1, -1):
        Lam[k] = lam
        if k == 0:
            break
        lx = t(c.q)[:, None] * (X[k] - t(c.x_ref)[:, None]) if node is None else nq[k] * (X[k] - nx[k]) + ng[k]
        lam = lx + np.einsum("mjb,mb->jb", A[k], lam)
        assert lam.dtype == np.float32
    return Lam


def node_rel(a, ref):
    """(H, ..., B) -> (H, B): per node and instance, max|a - ref| / max|ref| over the node's entries."""
    a = np.asarray(a, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    H, B = ref.shape[0], ref.shape[-1]
    d = np.abs(a - ref).reshape(H, -1, B).max(axis=1)
    with np.errstate(all="ignore"):
        out = d / np.maximum(np.abs(ref).reshape(H, -1, B).max(axis=1), 1e-300)
    return np.where(np.isnan(out), np.inf, out)


def row_rel(a, ref):
    """dV (2, B): per row and instance |a - ref| / |ref|"""
    a = np.asarray(a, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        out = np.abs(a - ref) / np.maximum(np.abs(ref), 1e-300)
    return np.where(np.isnan(out), np.inf, out)


def e32_of(ref, f32):
    """worst per-(node, instance) error of the fp32 restatement against the float64 reference, over K, kff and dV"""
    return float(max(node_rel(f32[0], ref[0]).max(), node_rel(f32[1], ref[1]).max(), row_rel(f32[2], ref[2]).max()))


def bar_of(e32, name=""):
    """the case's bar; the condition on its inputs is asserted here, before any GPU result is looked at"""
    assert e32 <= E32_MAX, (name, "fp32 restatement vs float64:", e32, "> ", E32_MAX, "- choose another case, never a wider bar")
    return FACTOR * e32


def check_riccati(name, K, kff, dV, ref, f32, quu_min=None, report=True):
    """Assert for EVERY (node, instance): node_rel(K) <= bar and node_rel(kff) <= bar, and per instance and row
    |dV - ref| / |ref| <= bar, with bar = 8 x e32 of the same inputs (ref = io.backward's (K, kff, dV), f32 = backward_f32's).
    Nothing is excluded.  Writes the parity_report line riccati[name].  -> (worst K, worst kff, worst dV, bar)."""
    e32 = e32_of(ref, f32)
    bar = bar_of(e32, name)
    if quu_min is not None:
        assert quu_min >= QUU_MIN, (name, "smallest eigenvalue of the reference's Quu", quu_min)
    eK, ek, eV = node_rel(K, ref[0]), node_rel(kff, ref[1]), row_rel(dV, ref[2])
    worst = max(eK.max(), ek.max(), eV.max())
    if report:
        H, B = eK.shape
        parity_report(f"riccati[{name}]", H=int(H), B=int(B), worst_K=float(eK.max()), worst_kff=float(ek.max()),
                      worst_dV=float(eV.max()), e32=e32, bar=bar, worst_over_e32=float(worst / max(e32, 1e-300)),
                      violations=int((eK > bar).sum() + (ek > bar).sum() + (eV > bar).sum()))
    where = lambda e: [tuple(int(i) for i in w) for w in np.argwhere(e > bar)[:8]]  # noqa: E731
    assert (eK <= bar).all(), (name, "K beyond", bar, "at (node, instance)", where(eK), "worst", float(eK.max()))
    assert (ek <= bar).all(), (name, "kff beyond", bar, "at (node, instance)", where(ek), "worst", float(ek.max()))
    assert (eV <= bar).all(), (name, "dV beyond", bar, "at (row, instance)", where(eV), "worst", float(eV.max()))
    return float(eK.max()), float(ek.max()), float(eV.max()), bar


def check_costate(name, Lam, ref, e32, report=True):
    """Every (node, instance) of the costate within 8 x e32, the error of the fp32 restatement on the case's parent batch
    (same condition on e32)."""
    bar = bar_of(e32, name)
    e = node_rel(Lam, ref)
    if report:
        parity_report(f"costate[{name}]", H=int(e.shape[0]), B=int(e.shape[1]), worst=float(e.max()), e32=e32, bar=bar,
                      worst_over_e32=float(e.max() / max(e32, 1e-300)), violations=int((e > bar).sum()))
    assert (e <= bar).all(), (name, "Lam beyond", bar, "at (node, instance)",
                              [tuple(int(i) for i in w) for w in np.argwhere(e > bar)[:8]], "worst", float(e.max()))
    return float(e.max()), bar


def case_seed(variant, B, H):
    return 1000 * list(VARIANTS).index(variant) + 10 * H + (B != PARENT_B)


@functools.lru_cache(maxsize=None)
def riccati_case(variant, B, H):
    """One row of the matrix, computed once and shared (treat as read-only): inputs, float64 reference, fp32 restatement,
    e32 and the smallest Quu eigenvalue of the reference."""
    nodef, newton, ug = VARIANTS[variant]
    inp = synthetic_riccati(B, H, case_seed(variant, B, H), node=nodef, newton=newton, uglin=ug)
    ref = reference(inp)
    f32 = backward_f32(inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], node=inp["node"], Hz=inp["Hz"], uglin=inp["uglin"])
    for a in list(ref) + list(f32) + [v for v in (inp["X"], inp["U"], inp["A"], inp["Bm"], inp["Hz"], inp["uglin"]) if v is not None]:
        a.setflags(write=False)
    return dict(inp=inp, ref=ref, f32=f32, e32=e32_of(ref, f32), quu_min=quu_min_eig(inp))


COSTATE_B = (1, 65, COSTATE_BLOCK + 1)   # one lane, a partial wave past the first, one lane of a second workgroup
COSTATE_CASES = [(nodef, B, H) for nodef in (False, True) for H in (1, 2, 9) for B in COSTATE_B]


@functools.lru_cache(maxsize=None)
def costate_parent(nodef, H):
    """The parent batch (B = kBlock + 1) of the costate cases at this H.  The smaller batches are its leading columns and
    share its e32: a node of one instance has 13 entries, and the worst of 13 roundings is by luck often far below what fp32
    costs on the case, so the estimate is taken over the 257 instances of the parent."""
    B = COSTATE_BLOCK + 1
    inp = synthetic_riccati(B, H, 7000 + 100 * int(nodef) + H, node=nodef)
    ref = io.costate(inp["cost"], inp["X"], inp["A"], node=inp["node"])
    f32 = costate_f32(inp["cost"], inp["X"], inp["A"], node=inp["node"])
    return dict(inp=inp, ref=ref, f32=f32, e32=float(node_rel(f32, ref).max()))
