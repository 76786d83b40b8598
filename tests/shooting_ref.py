"""Gauss-Newton multiple shooting (aircraft_amd/csrc/ac_shoot.hpp, ilqr_shoot_inst.hip, ilqr_backward_inst.hip, the SHOOT switch of ac_ilqr.hpp,
ILQR(shooting="multiple")) restated in NumPy.  TEST INFRASTRUCTURE, NOT PRODUCT.  In the style of tests/riccati_ref.py and
tests/box_ddp_ref.py, whose inputs, metric and bars it uses.

 * `backward_shoot_np(dtype, ...)`: the recursion of riccati_ref.backward_np in which node k reads v = V'_x + V'_xx d_k, d_k = F_k - x_{k+1},
   in place of V'_x; with box=True the QP of box_ddp_ref per node.  Also returns Vx[k], Vxx[k] = the expansion node k starts from.
 * `direction_np`: dx_0, du_k = kff_k + K_k dx_k, dx_{k+1} = A_k dx_k + B_k du_k + d_k, lam_k = Vx[k] + Vxx[k] dx_{k+1}.
 * `kkt_np`: the same QP by one dense KKT solve (float64, one instance) — what the two above are checked against.
 * `candidates_np`, `merit_weight_f32`, `merit_np`: the line-search pieces.
 * `solve_np`: the whole iteration on oracle.Oracle in a chosen precision.
float64 is the reference of the GPU tests; np.float32 measures what fp32 arithmetic costs on a case (e32), the bar is 8 x that."""
from __future__ import annotations

import functools

import numpy as np

from tests import box_ddp_ref as bx
from tests import riccati_ref as rf
from tests.helpers import f32_exact

MUTATIONS = (None, "drop_vxx_d", "flip_d", "x_k")   # for the tests: each must leave the GPU bar on every case
GAP = 0.3   # F = f32_exact(X[1:] + GAP N(0, 1))


def _bt(a):
    return np.moveaxis(a, -1, 0)


def backward_shoot_np(dtype, c, X, U, A, Bm, F, node=None, Hz=None, uglin=None, box=False, mutation=None, min_margin=None):
    """-> dict(K (H,7,13,B), kff (H,7,B), dV (2,B), Vx (H,13,B), Vxx (H,13,13,B), quu_min, and with box: act (H,7,B) int8,
    stat (2,B), margin_g, margin_x (H,B) as box_ddp_ref.backward_box_np).  min_margin (seed search): None at the first node where a
    margin falls below it or a QP hits a cap."""
    t = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    H, _, B = U.shape
    q, qf, r, reg = t(c.q), t(c.qf), t(c.r), dtype(c.reg)
    ulin = t(getattr(c, "u_lin", [0.0] * 7))
    umin, umax = t(c.u_min), t(c.u_max)
    X, U, A, Bm, F = t(X), t(U), t(A), t(Bm), t(F)
    half = dtype(0.5)
    eye13, eye7 = np.eye(13, dtype=dtype), np.eye(7, dtype=dtype)
    T = lambda M: np.swapaxes(M, -1, -2)  # noqa: E731
    mv = lambda M, v: (M @ v[..., None])[..., 0]  # noqa: E731
    K = np.zeros((H, 7, 13, B), dtype); kff = np.zeros((H, 7, B), dtype); dV = np.zeros((2, B), dtype)
    Vxo = np.zeros((H, 13, B), dtype); Vxxo = np.zeros((H, 13, 13, B), dtype)
    act = np.zeros((H, 7, B), np.int8); stat = np.zeros((2, B), np.int64)
    margin_g = np.full((H, B), np.inf); margin_x = np.full((H, B), np.inf)
    if node is None:
        Vx = qf[None] * (_bt(X[H]) - t(c.x_goal)[None]); Vxx = np.broadcast_to(np.diag(qf), (B, 13, 13)).copy()
    else:
        nq, nx, ng = (t(a) for a in node)
        Vx = _bt(nq[H]) * (_bt(X[H]) - _bt(nx[H])) + _bt(ng[H]); Vxx = _bt(nq[H])[:, :, None] * eye13[None]
    lo_eig = np.inf
    for k in range(H - 1, -1, -1):
        Vxo[k] = Vx.T; Vxxo[k] = np.moveaxis(Vxx, 0, -1)
        Ak, Bk = _bt(A[k]), _bt(Bm[k])
        xk, uk = _bt(X[k]), _bt(U[k])
        d = _bt(F[k]) - _bt(X[k + 1] if mutation != "x_k" else X[k])
        if mutation == "flip_d":
            d = -d
        v = Vx if mutation == "drop_vxx_d" else Vx + mv(Vxx, d)
        if node is None:
            qk = np.broadcast_to(q, (B, 13)); lx = qk * (xk - t(c.x_ref)[None])
        else:
            qk = _bt(nq[k]); lx = qk * (xk - _bt(nx[k])) + _bt(ng[k])
        lu = r[None] * uk + ulin[None]
        if uglin is not None:
            lu = lu + _bt(t(uglin)[k])
        Qx = lx + mv(T(Ak), v); Qu = lu + mv(T(Bk), v)
        VA, VB = Vxx @ Ak, Vxx @ Bk
        Qxx = qk[:, :, None] * eye13[None] + T(Ak) @ VA
        Qux = T(Bk) @ VA
        Quu = (r + reg)[None, :, None] * eye7[None] + T(Bk) @ VB
        if Hz is not None:
            Hk = _bt(t(Hz)[k])
            Qxx = Qxx + Hk[:, :13, :13]; Qux = Qux + Hk[:, 13:20, :13]; Quu = Quu + Hk[:, 13:20, 13:20]
        Quu = half * (Quu + T(Quu))
        lo_eig = min(lo_eig, float(np.linalg.eigvalsh(Quu.astype(np.float64)).min()))
        if not box:
            L = np.linalg.cholesky(Quu)
            rhs = np.concatenate([Qux, Qu[:, :, None]], axis=2)
            sol = -np.linalg.solve(T(L), np.linalg.solve(L, rhs))
            Kk, kk = sol[:, :, :13], sol[:, :, 13]
        else:
            Kk = np.zeros((B, 7, 13), dtype); kk = np.zeros((B, 7), dtype)
            for b in range(B):
                lo, hi = umin - uk[b], umax - uk[b]
                x, a, it, capped = bx.boxqp_np(dtype, Quu[b], Qu[b], lo, hi)
                cl = a != 0
                kk[b] = x
                Kk[b] = bx.free_solve(dtype, Quu[b], Qux[b], cl)
                act[k, :, b] = a
                stat[0, b] = max(stat[0, b], it); stat[1, b] += int(capped)
                grad = (Qu[b] + Quu[b] @ x).astype(np.float64)
                cn, fr = cl & (a != 2), ~cl
                if cn.any():
                    margin_g[k, b] = np.abs(grad[cn]).min() / np.abs(Qu[b]).max()
                if fr.any():
                    margin_x[k, b] = (np.minimum(x[fr] - lo[fr], hi[fr] - x[fr]) / (hi[fr] - lo[fr])).min()
            if min_margin is not None and (min(margin_g[k].min(), margin_x[k].min()) < min_margin or stat[1].any()):
                return None
        assert Kk.dtype == dtype and kk.dtype == dtype
        K[k] = np.moveaxis(Kk, 0, -1); kff[k] = kk.T
        Quukk = mv(Quu, kk)
        dV[0] += (kk * Qu).sum(axis=1); dV[1] += half * (kk * Quukk).sum(axis=1)
        Vx = Qx + mv(T(Kk), Quukk) + mv(T(Kk), Qu) + mv(T(Qux), kk)
        Vxx = Qxx + T(Kk) @ Quu @ Kk + T(Kk) @ Qux + T(Qux) @ Kk
        Vxx = half * (Vxx + T(Vxx))
    out = dict(K=K, kff=kff, dV=dV, Vx=Vxo, Vxx=Vxxo, quu_min=lo_eig)
    if box:
        out.update(act=act, stat=stat, margin_g=margin_g, margin_x=margin_x)
    return out


def direction_np(dtype, X, F, A, Bm, K, kff, Vx=None, Vxx=None, dx0=None, limits=None):
    """-> dX (H+1,13,B), dU (H,7,B), Lam (H,13,B) or None.  limits = (U, u_min, u_max): du_k = clip(U_k + kff_k + K_k dx_k) - U_k"""
    t = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    X, F, A, Bm, K, kff = t(X), t(F), t(A), t(Bm), t(K), t(kff)
    H, _, B = kff.shape
    dX = np.zeros((H + 1, 13, B), dtype); dU = np.zeros((H, 7, B), dtype)
    Lam = np.zeros((H, 13, B), dtype) if Vx is not None else None
    if dx0 is not None:
        dX[0] = t(dx0)
    for k in range(H):
        dU[k] = kff[k] + np.einsum("imb,mb->ib", K[k], dX[k])
        if limits is not None:
            Uk = t(limits[0])[k]
            dU[k] = np.minimum(np.maximum(Uk + dU[k], t(limits[1])[:, None]), t(limits[2])[:, None]) - Uk
        dX[k + 1] = np.einsum("jmb,mb->jb", A[k], dX[k]) + np.einsum("jib,ib->jb", Bm[k], dU[k]) + (F[k] - X[k + 1])
        if Vx is not None:
            Lam[k] = t(Vx)[k] + np.einsum("jmb,mb->jb", t(Vxx)[k], dX[k + 1])
    assert dX.dtype == dtype and dU.dtype == dtype
    return dX, dU, Lam


def kkt_np(c, X, U, A, Bm, F, b, node=None, Hz=None, uglin=None, dx0=None):
    """The QP of one iteration for instance b by ONE dense solve (float64): variables z = (dx_1..dx_H, du_0..du_{H-1}),
        min  sum_k lx_k'dx_k + lu_k'du_k + 1/2 dx_k'Lxx_k dx_k + du_k'Lux_k dx_k + 1/2 du_k'Luu_k du_k  +  terminal
        s.t. dx_{k+1} = A_k dx_k + B_k du_k + d_k          (multiplier nu_k;  lam_k = -nu_k)
    -> dX (H+1,13), dU (H,7), Lam (H,13)"""
    H = U.shape[0]
    q, qf, r = np.asarray(c.q, float), np.asarray(c.qf, float), np.asarray(c.r, float)
    ulin = np.asarray(getattr(c, "u_lin", [0.0] * 7), float)
    dx0 = np.zeros(13) if dx0 is None else np.asarray(dx0, float)
    nx, nu = 13 * H, 7 * H
    n = nx + nu
    Hm = np.zeros((n, n)); g = np.zeros(n)
    G = np.zeros((nx, n)); rhs = np.zeros(nx)
    ix = lambda k: slice(13 * (k - 1), 13 * k)          # dx_k, k = 1..H  # noqa: E731
    iu = lambda k: slice(nx + 7 * k, nx + 7 * (k + 1))  # du_k, k = 0..H-1  # noqa: E731
    for k in range(H + 1):
        if node is None:
            qk = qf if k == H else q
            lx = qk * (X[k, :, b] - np.asarray(c.x_goal if k == H else c.x_ref, float))
        else:
            qk = node[0][k, :, b]
            lx = qk * (X[k, :, b] - node[1][k, :, b]) + node[2][k, :, b]
        Lxx = np.diag(qk).astype(float)
        Lux = np.zeros((7, 13)); Luu = None
        if k < H:
            lu = r * U[k, :, b] + ulin + (uglin[k, :, b] if uglin is not None else 0.0)
            Luu = np.diag(r + c.reg)
            if Hz is not None:
                Hk = Hz[k, :, :, b]
                Lxx = Lxx + Hk[:13, :13]; Lux = Hk[13:20, :13]; Luu = Luu + Hk[13:20, 13:20]
            Luu = 0.5 * (Luu + Luu.T)
            Hm[iu(k), iu(k)] = Luu; g[iu(k)] = lu
        if k >= 1:
            Hm[ix(k), ix(k)] = Lxx; g[ix(k)] = lx
            if k < H:
                Hm[iu(k), ix(k)] = Lux; Hm[ix(k), iu(k)] = Lux.T
        elif k < H:  # dx_0 is data: its cross term moves into the gradient of du_0
            g[iu(0)] = g[iu(0)] + Lux @ dx0
        if k < H:
            row = slice(13 * k, 13 * (k + 1))
            G[row, ix(k + 1)] = np.eye(13)
            G[row, iu(k)] = -Bm[k, :, :, b]
            d = F[k, :, b] - X[k + 1, :, b]
            if k >= 1:
                G[row, ix(k)] = -A[k, :, :, b]
                rhs[row] = d
            else:
                rhs[row] = d + A[0, :, :, b] @ dx0
    KKT = np.block([[Hm, G.T], [G, np.zeros((nx, nx))]])
    sol = np.linalg.solve(KKT, np.concatenate([-g, rhs]))
    dX = np.concatenate([dx0[None], sol[:nx].reshape(H, 13)])
    return dX, sol[nx:n].reshape(H, 7), -sol[n:].reshape(H, 13)


# ---- the line-search pieces ------------------------------------------------------------------------------------------------------
def candidates_np(X, U, dX, dU, alphas, u_min, u_max):
    """float64 formula -> Xc (H+1,13,na B), Uc (H,7,na B); column a B + b"""
    lo, hi = np.asarray(u_min, float)[None, :, None], np.asarray(u_max, float)[None, :, None]
    Xc = np.concatenate([X + a * dX for a in alphas], axis=2)
    Uc = np.concatenate([np.clip(U + a * dU, lo, hi) for a in alphas], axis=2)
    return Xc, Uc


def merit_weight_f32(mu, Lam, factor):
    """mu, Lam float32 -> max(mu, fl32(factor * max |Lam|)) bit for bit"""
    m = np.abs(np.asarray(Lam, np.float32)).max(axis=(0, 1)).astype(np.float32)
    return np.maximum(np.asarray(mu, np.float32), (np.float32(factor) * m).astype(np.float32))


def merit_np(dtype, J, mu, R):
    """phi[c] = J[c] + mu[c % Bn] sum |R[:, :, c]| with the rows summed in their order, defect_inf[c] = max |R|, and S_abs =
    |J| + mu sum |R| (the metric's denominator)"""
    J, mu, R = np.asarray(J, dtype), np.asarray(mu, dtype), np.asarray(R, dtype)
    H, _, Bc = R.shape
    s = np.zeros(Bc, dtype)
    for row in np.abs(R).reshape(H * 13, Bc):
        s = s + row
    m = np.tile(mu, Bc // mu.shape[0])
    assert s.dtype == dtype
    return J + m * s, np.abs(R).max(axis=(0, 1)), np.abs(J) + m * s


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def shoot_inputs(variant, B, H, seed, gap=GAP):
    """riccati_ref.synthetic_riccati plus F = f32_exact(X[1:] + gap N(0, 1))"""
    nodef, newton, ug = rf.VARIANTS[variant]
    inp = dict(rf.synthetic_riccati(B, H, seed, node=nodef, newton=newton, uglin=ug))
    rng = np.random.default_rng(seed + 424242)
    inp["F"] = f32_exact(inp["X"][1:] + gap * rng.normal(size=(H, 13, B))) if gap else inp["X"][1:].copy()
    return inp


def run_np(dtype, inp, box=False, mutation=None, min_margin=None):
    return backward_shoot_np(dtype, inp["cost"], inp["X"], inp["U"], inp["A"], inp["Bm"], inp["F"], node=inp["node"], Hz=inp["Hz"],
                             uglin=inp["uglin"], box=box, mutation=mutation, min_margin=min_margin)


FIELDS = ("K", "kff", "Vx", "Vxx")


def errors(got, ref):
    """per field the (node, instance) errors of riccati_ref.node_rel, dV per row and instance"""
    e = {f: rf.node_rel(got[f], ref[f]) for f in FIELDS if got.get(f) is not None}
    e["dV"] = rf.row_rel(got["dV"], ref["dV"])
    return e


def e32_of(ref, f32):
    return float(max(e.max() for e in errors(f32, ref).values()))


def case_seed(variant, B, H):
    return 500000 + rf.case_seed(variant, B, H)


@functools.lru_cache(maxsize=None)
def shoot_case(variant, B, H):
    """One row of the backward matrix (read-only): inputs, float64 reference, fp32 restatement, e32, smallest Quu eigenvalue."""
    inp = shoot_inputs(variant, B, H, case_seed(variant, B, H))
    ref, f32 = run_np(np.float64, inp), run_np(np.float32, inp)
    return dict(inp=inp, ref=ref, f32=f32, e32=e32_of(ref, f32), quu_min=ref["quu_min"])


def columns(inp, sl):
    out = rf.columns(inp, sl)
    out["F"] = np.ascontiguousarray(inp["F"][..., sl])
    return out


# ---- backward with the box ---------------------------------------------------------------------------------------------------------
BOX_VARIANTS = ("gn", "goal")
BOX_SEARCH = 64


def box_inputs(variant, B, H, seed, wide=False):
    inp, _ = bx.box_inputs(variant, None if wide else "sym", B, H, seed)
    rng = np.random.default_rng(seed + 424242)
    inp["F"] = f32_exact(inp["X"][1:] + GAP * rng.normal(size=(H, 13, B)))
    return inp


def box_conditions(ref, f32):
    fig = dict(margin_g=float(ref["margin_g"].min()), margin_x=float(ref["margin_x"].min()),
               same_act=bool(np.array_equal(ref["act"], f32["act"])), e32=e32_of(ref, f32),
               capped=int(ref["stat"][1].sum() + f32["stat"][1].sum()))
    ok = (fig["margin_g"] >= bx.MARGIN and fig["margin_x"] >= bx.MARGIN and fig["same_act"] and fig["e32"] <= rf.E32_MAX
          and fig["capped"] == 0)
    return ok, fig


@functools.lru_cache(maxsize=None)
def box_case(variant, B, H):
    """the first of BOX_SEARCH consecutive seeds on which the float64 reference keeps box_ddp_ref.MARGIN at every (node, instance,
    row), the fp32 restatement has the same active set, e32 <= E32_MAX and no QP hits a cap (as box_ddp_ref.find_seed)"""
    base = 700000 + bx.seed_base(variant, "sym", B, H)
    for off in range(BOX_SEARCH):
        inp = box_inputs(variant, B, H, base + off)
        ref = run_np(np.float64, inp, box=True, min_margin=bx.MARGIN)
        if ref is None:
            continue
        f32 = run_np(np.float32, inp, box=True)
        ok, fig = box_conditions(ref, f32)
        if ok:
            return dict(inp=inp, ref=ref, f32=f32, e32=fig["e32"], fig=fig, offset=off)
    raise AssertionError(("no seed within", BOX_SEARCH, "meets the case conditions", variant, B, H))


# ---- direction ---------------------------------------------------------------------------------------------------------------------
DIRECTION_LANES = 64      # k_shoot_direction: one wave per instance
DIRECTION_B = (1, 65, 257)
DIRECTION_H = (1, 2, 9)
DIRECTION_BOX = 0.75      # half-width of the box of the clipped-direction cases


@functools.lru_cache(maxsize=None)
def direction_parent(H):
    """The parent batch (B = 257) at this H; the smaller batches are its leading columns and share its e32 (as
    riccati_ref.costate_parent).  The inputs are the float64 backward's outputs rounded to float32."""
    B = DIRECTION_B[-1]
    inp = shoot_inputs("gn", B, H, 900000 + H)
    bw = run_np(np.float64, inp)
    t = {k: f32_exact(bw[k]) for k in ("K", "kff", "Vx", "Vxx")}
    args = (inp["X"], inp["F"], inp["A"], inp["Bm"], t["K"], t["kff"], t["Vx"], t["Vxx"])
    ref, f32 = direction_np(np.float64, *args), direction_np(np.float32, *args)
    e32 = float(max(rf.node_rel(f32[0][1:], ref[0][1:]).max(), rf.node_rel(f32[1], ref[1]).max(), rf.node_rel(f32[2], ref[2]).max()))
    # the same sweep with the control step clipped into a box that binds on a good part of the rows
    lim = (np.clip(inp["U"], -DIRECTION_BOX, DIRECTION_BOX), [-DIRECTION_BOX] * 7, [DIRECTION_BOX] * 7)
    cref, c32 = direction_np(np.float64, *args, limits=lim), direction_np(np.float32, *args, limits=lim)
    ce32 = float(max(rf.node_rel(c32[0][1:], cref[0][1:]).max(), rf.node_rel(c32[1], cref[1]).max(), rf.node_rel(c32[2], cref[2]).max()))
    return dict(inp=inp, t=t, ref=ref, f32=f32, e32=e32, lim=lim, cref=cref, c32=c32, ce32=ce32)


# ---- the whole iteration on the oracle -----------------------------------------------------------------------------------------------
def _cost_np(c, X, U):
    import ilqr_oracle as io

    return io.cost(c, X, U)


def solve_np(dtype, orc, c, x0, X0, U0, alphas, iters, dt, defect_weight=1.0, merit_factor=2.0):
    """ILQR(shooting='multiple').solve with the constant quadratic cost, box='clip', in `dtype` (the oracle's step and
    sensitivities are float64, rounded to `dtype` where dtype is float32).
    -> dict(X, U, J (iters+1,B), dinf (iters+1,B), arg (iters,B) accepted alpha index or -1, phic (iters,na,B), phi0 (iters,B),
            mu (iters,B))"""
    t = lambda a: np.asarray(a, dtype=dtype)  # noqa: E731
    X, U = t(X0).copy(), t(U0).copy()
    X[0] = t(x0)
    H, _, B = U.shape
    na = len(alphas)
    mu = np.full(B, dtype(defect_weight))
    tr = dict(J=[], dinf=[], arg=[], phic=[], phi0=[], mu=[])

    def lin(X, U):
        F = np.zeros((H, 13, B), dtype); A = np.zeros((H, 13, 13, B), dtype); Bm = np.zeros((H, 13, 7, B), dtype)
        for k in range(H):
            Fk, Ak, Bk, _ = orc.step_sens(X[k].astype(np.float64), U[k].astype(np.float64), dt)
            F[k], A[k], Bm[k] = t(Fk), t(Ak), t(Bk)
        return F, A, Bm

    def step(Xc, Uc):
        Fc = np.zeros((H, 13, Xc.shape[2]), dtype)
        for k in range(H):
            Fc[k] = t(orc.state_update(Xc[k].astype(np.float64), Uc[k].astype(np.float64), dt))
        return Fc

    for _ in range(iters):
        F, A, Bm = lin(X, U)
        bw = backward_shoot_np(dtype, c, X, U, A, Bm, F)
        dX, dU, Lam = direction_np(dtype, X, F, A, Bm, bw["K"], bw["kff"], bw["Vx"], bw["Vxx"], limits=(U, c.u_min, c.u_max))
        mu = np.maximum(mu, dtype(merit_factor) * np.abs(Lam).max(axis=(0, 1))).astype(dtype)
        lo, hi = t(c.u_min)[None, :, None], t(c.u_max)[None, :, None]
        Xc = np.concatenate([X] * na, axis=2); Uc = np.concatenate([U] * na, axis=2)
        for a, al in enumerate(alphas):
            sl = slice(a * B, (a + 1) * B)
            Xc[1:, :, sl] = X[1:] + dtype(al) * dX[1:]
            Uc[:, :, sl] = np.minimum(np.maximum(U + dtype(al) * dU, lo), hi)
        Rc = Xc[1:] - step(Xc, Uc)
        Jc, J0 = t(_cost_np(c, Xc, Uc)), t(_cost_np(c, X, U))
        phic, _, _ = merit_np(dtype, Jc, mu, Rc)
        phi0, dinf0, _ = merit_np(dtype, J0, mu, X[1:] - F)
        pc = phic.reshape(na, B)
        arg = np.argmin(np.where(np.isfinite(pc), pc, np.inf), axis=0)
        imp = pc[arg, np.arange(B)] < phi0
        tr["J"].append(J0); tr["dinf"].append(dinf0); tr["arg"].append(np.where(imp, arg, -1)); tr["phic"].append(pc); tr["phi0"].append(phi0)
        tr["mu"].append(mu.copy())
        for b in np.flatnonzero(imp):
            X[:, :, b] = Xc[:, :, arg[b] * B + b]; U[:, :, b] = Uc[:, :, arg[b] * B + b]
    F = step(X, U)
    tr["J"].append(t(_cost_np(c, X, U))); tr["dinf"].append(np.abs(X[1:] - F).max(axis=(0, 1)))
    out = {k: np.stack(v) for k, v in tr.items()}
    out.update(X=X, U=U)
    return out
