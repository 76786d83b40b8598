"""The exact control-rate Riccati pass (aircraft_amd/csrc/ac_ilqr_rate.hpp: k_ilqr_backward_rate<NODE, NEWTON>), its rate
models and its closed-loop law, restated in NumPy.  TEST INFRASTRUCTURE, NOT PRODUCT.  In the style of tests/riccati_ref.py,
whose inputs, metric and bars it uses.

 * `backward_rate_np`: the recursion that carries p_k = u_{k-1} (V_k(x_k, p_k): Vx, Vp, Vxx, Vxp, Vpp) in a chosen precision;
   float64 is the reference of the GPU tests, float32 measures what fp32 arithmetic costs on a case (e32; bar = 8 x e32);
 * `dense_solution`: the same linear-quadratic problem stacked over the horizon and solved in one piece — what the float64
   recursion is checked against (tests/test_riccati_rate_ref.py);
 * `quad_rate_*` / `l0_rate_model`: the two rate models (gradient and diagonal curvature per difference d_k = u_k - u_{k-1});
 * `forward_rate`: the closed-loop law  u_k = clip(U_k + alpha k_k + Kx_k (x - Xnom_k) + Kp_k (u_applied_{k-1} - U_{k-1}))
   over the oracle's state_update.

Ring depths of k_ilqr_backward_rate (IlqrRing<NODE, NEWTON, false, true>::kDepth, beside kInstr = 7 / 14 DMA instructions per node):
8 without the second-order blocks, 5 with them — the depths of k_ilqr_backward, so `riccati_ref.horizons` is the set of
ring edges of this kernel too; stated here once as K_DEPTH."""
from __future__ import annotations

import functools

import numpy as np

import ilqr_oracle as io
from tests.helpers import f32_exact
from tests.riccati_ref import E32_MAX, FACTOR, QUU_MIN, bar_of, node_rel, row_rel, synthetic_riccati  # noqa: F401

K_DEPTH = {False: 8, True: 5}    # IlqrRing<., NEWTON, false, true>::kDepth
PARENT_B = 7
WIDE_B = 65

# the four instantiations: name -> (NODE, NEWTON)
VARIANTS = {"gn": (False, False), "node": (True, False), "newton": (False, True), "node_newton": (True, True)}


def k_depth(newton):
    return K_DEPTH[bool(newton)]


def horizons(newton):
    """riccati_ref.horizons recomputed for this kernel's ring: never full (1, 2, kDepth-1), exactly full, the first refill, a
    slot reused twice (2 kDepth-1 .. 2 kDepth+1), and 23"""
    d = k_depth(newton)
    return sorted({1, 2, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 23})


def matrix():
    rows = []
    for v, (_, newton) in VARIANTS.items():
        rows += [(v, PARENT_B, H) for H in horizons(newton)]
        rows.append((v, WIDE_B, k_depth(newton) + 1))
    return rows


def synthetic_rate(B, H, seed):
    """g = 0.5 N(0, 1), h ~ U(0.2, 2), rounded to fp32 -> (rate_g, rate_h), each (H, 7, B)"""
    rng = np.random.default_rng(seed)
    return f32_exact(0.5 * rng.normal(size=(H, 7, B))), f32_exact(rng.uniform(0.2, 2.0, (H, 7, B)))


def _bt(a):
    return np.moveaxis(a, -1, 0)


def backward_rate_np(dtype, c, X, U, A, Bm, rate_g, rate_h, node=None, Hz=None):
    """The recursion of ac_ilqr_rate.hpp in `dtype` throughout (all instances at once).
    -> K (H,7,13,B), Kp (H,7,7,B), kff (H,7,B), dV (2,B), and the smallest eigenvalue of Quu over nodes and instances."""
    t = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    H, _, B = U.shape
    q, qf, r, reg = t(c.q), t(c.qf), t(c.r), dtype(c.reg)
    ulin = t(getattr(c, "u_lin", [0.0] * 7))
    X, U, A, Bm, G, Hh = t(X), t(U), t(A), t(Bm), t(rate_g), t(rate_h)
    half = dtype(0.5)
    eye13, eye7 = np.eye(13, dtype=dtype), np.eye(7, dtype=dtype)
    T = lambda M: np.swapaxes(M, -1, -2)  # noqa: E731
    mv = lambda M, v: (M @ v[..., None])[..., 0]  # noqa: E731
    K = np.zeros((H, 7, 13, B), dtype); Kp = np.zeros((H, 7, 7, B), dtype); kff = np.zeros((H, 7, B), dtype)
    dV = np.zeros((2, B), dtype)
    if node is None:
        Vx = qf[None] * (_bt(X[H]) - t(c.x_goal)[None]); Vxx = np.broadcast_to(np.diag(qf), (B, 13, 13)).copy()
    else:
        nq, nx, ng = (t(a) for a in node)
        Vx = _bt(nq[H]) * (_bt(X[H]) - _bt(nx[H])) + _bt(ng[H]); Vxx = _bt(nq[H])[:, :, None] * eye13[None]
    Vp = np.zeros((B, 7), dtype); Vxp = np.zeros((B, 13, 7), dtype); Vpp = np.zeros((B, 7, 7), dtype)
    lo = np.inf
    for k in range(H - 1, -1, -1):
        Ak, Bk = _bt(A[k]), _bt(Bm[k])
        xk, uk = _bt(X[k]), _bt(U[k])
        g, h = _bt(G[k]), _bt(Hh[k])                       # (B, 7)
        if node is None:
            qk = np.broadcast_to(q, (B, 13)); lx = qk * (xk - t(c.x_ref)[None])
        else:
            qk = _bt(nq[k]); lx = qk * (xk - _bt(nx[k])) + _bt(ng[k])
        lu = r[None] * uk + ulin[None]
        D = h[:, :, None] * eye7[None]                     # diag(h)
        Qx = lx + mv(T(Ak), Vx)
        Qu = lu + mv(T(Bk), Vx) + Vp + g
        Qp = -g
        M = T(Bk) @ Vxx + T(Vxp)                           # B'V'xx + V'px
        Qxx = qk[:, :, None] * eye13[None] + T(Ak) @ (Vxx @ Ak)
        Qux = M @ Ak
        Quu = (r + reg)[None, :, None] * eye7[None] + T(Bk) @ (Vxx @ Bk) + T(Bk) @ Vxp + T(Vxp) @ Bk + Vpp + D
        if Hz is not None:
            Hk = _bt(t(Hz)[k])
            Qxx = Qxx + Hk[:, :13, :13]; Qux = Qux + Hk[:, 13:20, :13]; Quu = Quu + Hk[:, 13:20, 13:20]
        Qup, Qpp = -D, D
        Quu = half * (Quu + T(Quu))
        lo = min(lo, float(np.linalg.eigvalsh(Quu.astype(np.float64)).min()))
        L = np.linalg.cholesky(Quu)
        rhs = np.concatenate([Qux, Qup, Qu[:, :, None]], axis=2)       # 13 + 7 + 1 right-hand sides
        sol = -np.linalg.solve(T(L), np.linalg.solve(L, rhs))
        assert sol.dtype == dtype
        Kx, Kpk, kk = sol[:, :, :13], sol[:, :, 13:20], sol[:, :, 20]
        K[k] = np.moveaxis(Kx, 0, -1); Kp[k] = np.moveaxis(Kpk, 0, -1); kff[k] = kk.T
        Quukk = mv(Quu, kk)
        dV[0] += (kk * Qu).sum(axis=1); dV[1] += half * (kk * Quukk).sum(axis=1)
        res = Quukk + Qu
        Vx = Qx + mv(T(Kx), res) + mv(T(Qux), kk)
        Vp = Qp + mv(T(Kpk), res) + mv(T(Qup), kk)
        Vxx = Qxx + T(Kx) @ Quu @ Kx + T(Kx) @ Qux + T(Qux) @ Kx
        Vxp = T(Kx) @ Quu @ Kpk + T(Kx) @ Qup + T(Qux) @ Kpk
        Vpp = Qpp + T(Kpk) @ Quu @ Kpk + T(Kpk) @ Qup + T(Qup) @ Kpk
        Vxx = half * (Vxx + T(Vxx)); Vpp = half * (Vpp + T(Vpp))
    return K, Kp, kff, dV, lo


def reference(inp, rate):
    return backward_rate_np(np.float64, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], rate[0], rate[1], node=inp["node"],
                            Hz=inp["Hz"])


def dense_solution(c, X, U, A, Bm, rate_g, rate_h, b, node=None, Hz=None):
    """Instance b of the same problem as ONE quadratic in the stacked control steps du = (du_0 .. du_{H-1}), with dx_0 = 0,
    dp_0 = 0, dx_{k+1} = A_k dx_k + B_k du_k:  J(du) = 1/2 du'M du + m'du.  -> (du* (H, 7), dx* (H+1, 13), J(du*))."""
    H = U.shape[0]
    n = 7 * H
    q, qf, r = np.asarray(c.q, float), np.asarray(c.qf, float), np.asarray(c.r, float)
    ulin = np.asarray(getattr(c, "u_lin", [0.0] * 7), float)
    # dx_k = G_k du
    G = [np.zeros((13, n))]
    for k in range(H):
        Gn = A[k, :, :, b] @ G[k]
        Gn[:, 7 * k:7 * k + 7] += Bm[k, :, :, b]
        G.append(Gn)
    M = np.zeros((n, n)); m = np.zeros(n)
    for k in range(H + 1):
        if node is None:
            qk = qf if k == H else q
            lx = qk * (X[k, :, b] - np.asarray(c.x_goal if k == H else c.x_ref, float))
        else:
            qk = node[0][k, :, b]
            lx = qk * (X[k, :, b] - node[1][k, :, b]) + node[2][k, :, b]
        Qxx = np.diag(qk)
        if k < H and Hz is not None:
            Qxx = Qxx + Hz[k, :13, :13, b]
        M += G[k].T @ Qxx @ G[k]; m += G[k].T @ lx
        if k == H:
            break
        E = np.zeros((7, n)); E[:, 7 * k:7 * k + 7] = np.eye(7)      # du_k = E du
        Ruu = np.diag(r + c.reg)
        if Hz is not None:
            Ruu = Ruu + Hz[k, 13:20, 13:20, b]
            Hux = Hz[k, 13:20, :13, b]
            cross = E.T @ Hux @ G[k]
            M += cross + cross.T
        M += E.T @ (0.5 * (Ruu + Ruu.T)) @ E
        m += E.T @ (r * U[k, :, b] + ulin)
        Dd = E.copy()                                                  # d(du_k - du_{k-1}); dp_0 = 0
        if k > 0:
            Dd[:, 7 * (k - 1):7 * k] -= np.eye(7)
        M += Dd.T @ np.diag(rate_h[k, :, b]) @ Dd; m += Dd.T @ rate_g[k, :, b]
    M = 0.5 * (M + M.T)
    du = -np.linalg.solve(M, m)
    dx = np.stack([Gk @ du for Gk in G])
    return du.reshape(H, 7), dx, float(0.5 * m @ du), float(np.linalg.eigvalsh(M).min())


def policy_on_linear_model(K, Kp, kff, A, Bm, b):
    """du_k = k_k + Kx_k dx_k + Kp_k du_{k-1} rolled out on dx_{k+1} = A_k dx_k + B_k du_k from dx_0 = 0, dp_0 = 0 -> du (H, 7)"""
    H = kff.shape[0]
    dx = np.zeros(13); dp = np.zeros(7); out = np.zeros((H, 7))
    for k in range(H):
        du = kff[k, :, b] + K[k, :, :, b] @ dx + Kp[k, :, :, b] @ dp
        out[k] = du
        dx = A[k, :, :, b] @ dx + Bm[k, :, :, b] @ du
        dp = du
    return out


def e32_of(ref, f32):
    """worst per-(node, instance) error of the fp32 restatement over K, Kp, kff and dV; ref / f32 = (K, Kp, kff, dV, ...)"""
    return float(max(node_rel(f32[0], ref[0]).max(), node_rel(f32[1], ref[1]).max(), node_rel(f32[2], ref[2]).max(),
                     row_rel(f32[3], ref[3]).max()))


def case_seed(variant, B, H):
    return 50000 + 1000 * list(VARIANTS).index(variant) + 10 * H + (B != PARENT_B)


@functools.lru_cache(maxsize=None)
def rate_case(variant, B, H):
    """One row of the GPU matrix, computed once and shared (read-only): inputs, rate arrays, float64 reference, e32, min eig."""
    nodef, newton = VARIANTS[variant]
    seed = case_seed(variant, B, H)
    inp = synthetic_riccati(B, H, seed, node=nodef, newton=newton)
    rate = synthetic_rate(B, H, seed + 7)
    ref = reference(inp, rate)
    f32 = backward_rate_np(np.float32, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], rate[0], rate[1], node=inp["node"],
                           Hz=inp["Hz"])
    for a in list(ref[:4]) + list(rate):
        a.setflags(write=False)
    return dict(inp=inp, rate=rate, ref=ref[:4], e32=e32_of(ref, f32), quu_min=ref[4])


def columns_rate(rate, sl):
    return tuple(np.ascontiguousarray(a[..., sl]) for a in rate)


# ---- rate models ---------------------------------------------------------------------------------------------------------------
def quad_rate_cost(dtype, w, U, u_prev=None):
    """1/2 sum_k sum_i w_i (u_k,i - u_{k-1},i)^2, the k = 0 term against u_prev (7, Bn) when given; U (H, 7, Bc) -> (Bc,)"""
    w, U = np.asarray(w, dtype), np.asarray(U, dtype)
    d = U[1:] - U[:-1]
    J = (dtype(0.5) * w[None, :, None] * d * d).sum(axis=(0, 1), dtype=dtype)
    if u_prev is not None:
        up = np.tile(np.asarray(u_prev, dtype), (1, U.shape[2] // u_prev.shape[1]))
        d0 = U[0] - up
        J = J + (dtype(0.5) * w[:, None] * d0 * d0).sum(axis=0, dtype=dtype)
    return J


def quad_rate_sabs(w, U, u_prev=None):
    return quad_rate_cost(np.float64, w, U, u_prev)      # every summand is >= 0


def quad_rate_model(dtype, w, U, u_prev=None):
    """-> rate_g = w d, rate_h = w, each (H, 7, B); row 0 zeros without u_prev"""
    w, U = np.asarray(w, dtype), np.asarray(U, dtype)
    g = np.zeros_like(U); h = np.zeros_like(U)
    g[1:] = w[None, :, None] * (U[1:] - U[:-1]); h[1:] = w[None, :, None]
    if u_prev is not None:
        g[0] = w[:, None] * (U[0] - np.asarray(u_prev, dtype)); h[0] = w[:, None]
    return g, h


def l0_rate_model(dtype, gl, U):
    """The l0 term of the goal loss per difference: rate_g = w_rate l0'(d_k), rate_h = w_rate l0'^2 / (2 l0) (-> 2 w_rate / eps
    at d = 0), d_k = u_k - u_{k-1}; row 0 and the time row zero.  gl: io.GoalLoss."""
    U = np.asarray(U, dtype)
    eps, w = dtype(gl.eps_rate), dtype(gl.w_rate)
    d = U[1:] - U[:-1]
    e = np.exp(-(d * d) / eps)
    gp = (dtype(2) * d / eps) * e
    l0 = -np.expm1(-(d * d) / eps)
    with np.errstate(all="ignore"):
        hp = np.where(l0 > dtype(1e-12), (gp * gp) / (dtype(2) * np.maximum(l0, dtype(1e-30))), (dtype(2) / eps) * e)
    mask = np.zeros(7, dtype); mask[io._rate_rows(gl)] = 1
    g = np.zeros_like(U); h = np.zeros_like(U)
    g[1:] = w * gp * mask[None, :, None]; h[1:] = w * hp * mask[None, :, None]
    assert g.dtype == dtype and h.dtype == dtype
    return g, h


# ---- closed loop ---------------------------------------------------------------------------------------------------------------
def forward_rate(orc, c, x0, Xnom, U, K, Kp, kff, alphas, dt):
    """io.forward with the previous-control term: column a*B + b;  Kp None = io.forward's law.
    -> Xc (H+1,13,na*B), Uc (H,7,na*B), and whether the control was clipped at any node, per row and column (7, na*B)"""
    H, _, B = U.shape
    na = len(alphas)
    Xc = np.zeros((H + 1, 13, na * B)); Uc = np.zeros((H, 7, na * B)); clipped = np.zeros((7, na * B), dtype=bool)
    umin, umax = np.asarray(c.u_min, float)[:, None], np.asarray(c.u_max, float)[:, None]
    row = getattr(c, "dt_row", 0)
    for a, al in enumerate(alphas):
        x = x0.copy(); sl = slice(a * B, (a + 1) * B)
        Xc[0, :, sl] = x
        u = None
        for k in range(H):
            raw = U[k] + al * kff[k] + np.einsum("imb,mb->ib", K[k], x - Xnom[k])
            if Kp is not None and k > 0:
                raw = raw + np.einsum("imb,mb->ib", Kp[k], u - U[k - 1])
            u = np.clip(raw, umin, umax)
            clipped[:, sl] |= (u != raw)
            Uc[k, :, sl] = u
            x = orc.state_update(x, u, u[row] if row > 0 else dt)
            Xc[k + 1, :, sl] = x
    return Xc, Uc, clipped
