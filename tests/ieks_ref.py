"""Float64 restatement of the iterated extended Kalman smoother (aircraft_amd/csrc/ac_ieks.hpp; include/aircraft_hip.h,
ac_ieks_pass_f32 .. ac_ieks_solve_f32) for the tests, on top of tests/ekf_ref.py and tests/rts_ref.py: the
linearised pass, the MAP cost, the candidates, the accept decision and the solve loop; the dense Gauss-Newton problem the pass
plus smoother is checked against; the gradient of the cost by central differences; the inputs of the tests; the host build's
entry points and the recorded worst float32 errors E32_WORST.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import ctypes as C

import numpy as np

from tests import ekf_ref as E
from tests import rts_ref as R

P0_NOT_PD, NONFINITE, QZERO_DEFECT, NO_DECREASE = 1, 2, 4, 8
LADDER = (1.0, 0.5, 0.25, 0.125)
CHUNK = 32

# e32: the host build (g++, -ffp-contract=off) against this restatement on identical float32-rounded inputs (prior, nominal, F, A,
# Z, Qd, Rd), worst instance over the chains of ekf_ref.MODELS (inputs()) and the lengths T = 1, 2, 5, 6.  tests/test_host_ieks.py measures them and fails if
# they are exceeded; DESIGN.md §4.20 quotes them.  The GPU tests check an instance when its e32 is within 2 x these and hold the
# device to 8 x the worst e32 of the checked instances of its batch.  Measures: x, P, S, nu, nis, ll, Ppred, Abar ekf_ref's, worst
# over the steps (xpred: err_state of Xpreds); J, Jprior, Jproc, Jmeas: |dJ| / (1 + |J64|).
E32_WORST = {"x": 6.4e-7, "xpred": 1.8e-6, "P": 5.7e-5, "S": 5.5e-6, "nu": 2.8e-5, "nis": 5.5e-6, "ll": 6.5e-6, "Ppred": 5.8e-6,
             "Abar": 2.8e-7, "J": 3.3e-6, "Jprior": 6.0e-7, "Jproc": 4.6e-6, "Jmeas": 6.9e-6}

mm, mv, tr, sym, f32x, c32 = E.mm, E.mv, E.tr, E.sym, E.f32x, E.c32
finite = R.finite


# ---- the linearised pass ---------------------------------------------------------------------------------------------------------
def linearise(orc, Xbar, U, dt=E.DT):
    """F_k, A_k at Xbar[k], U[k] for k = 0 .. T-1 -> (T, 13, n), (T, 13, 13, n)"""
    out = [orc.step_sens(Xbar[k], U[k], dt)[:2] for k in range(U.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def images(orc, Xt, U, dt=E.DT):
    """F(Xt[k], U[k]) for k = 0 .. T-1 -> (T, 13, cols)"""
    return np.stack([orc.state_update(Xt[k], U[k], dt) for k in range(U.shape[0])])


def _safe(x, ok):
    """x where ok, else a harmless flight state (ekf_ref.update's)"""
    xs = np.where(ok, x, 0.0)
    xs[9] = np.where(ok, x[9], 1.0)
    xs[3] = np.where(ok, x[3], 30.0)
    return xs


def _update(xb, dm, Pm, z, mask, Rd, ok0, mag, eps):
    """ekf_ref.update's fifteen scalar updates with nu and H at the nominal xb, from d = dm; ok0: the instances that are updated"""
    n = xb.shape[1]
    mask = np.full(n, E.ALL) if mask is None else np.asarray(mask).astype(np.int64)
    xs = _safe(xb, ok0)
    H = E.H_of(xs, mag, eps)
    nu0 = z - E.h(xs, mag, eps)
    P, d = np.where(ok0, Pm, 0.0), np.where(ok0, dm, 0.0)
    nu, S = np.zeros((E.ROWS, n)), np.zeros((E.ROWS, n))
    nis, ll = np.zeros(n), np.zeros(n)
    usedbits, rejected = np.zeros(n, np.int64), np.zeros(n, bool)
    for i in range(E.ROWS):
        hi = H[i]
        ph = np.einsum("rjn,jn->rn", P, hi)
        s = (hi * ph).sum(0) + Rd[i]
        rho = nu0[i] - (hi * d).sum(0)
        used = ok0 & (((mask >> i) & 1) == 1) & np.isfinite(z[i])
        ok = used & (s > 0) & np.isfinite(s)
        rejected |= used & ~ok
        w = np.where(ok, 1.0 / np.where(ok, s, 1.0), 0.0)
        r_ok, ph_ok = np.where(ok, rho, 0.0), np.where(ok, ph, 0.0)
        d = d + ph_ok * (r_ok * w)
        P = P - ph_ok[:, None] * ph_ok[None, :] * w
        nu[i], S[i] = np.where(used, rho, 0.0), np.where(used, s, 0.0)
        nis += r_ok * r_ok * w
        ll += np.where(ok, -0.5 * (np.log(2 * np.pi * np.where(ok, s, 1.0)) + r_ok * r_ok * w), 0.0)
        usedbits |= np.where(used, 1 << i, 0)
    return dict(d=d, P=P, nu=nu, S=S, nis=nis, ll=ll, used=usedbits, rejected=rejected, xs=xs)


def pass_(X0, P0, Xbar, F, A, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0, drop_c=False, at_prediction=False, no_q=False, d0_zero=False):
    """The forward recursion about Xbar (T+1, 13, n) through F (T, 13, n), A (T, 13, 13, n) -> dict of X, P, Xpred, Ppred, Abar, nu, S,
    nis, used, status stacked on a leading axis T, ll (n,), X0, P0.  The keyword flags are the mutations the tests must catch."""
    T_, n = Z.shape[0], X0.shape[1]
    out = {k: [] for k in ("X", "P", "Xpred", "Ppred", "Abar", "nu", "S", "nis", "used", "status")}
    with np.errstate(all="ignore"):
        d = np.zeros((12, n)) if d0_zero else E.boxminus(X0, Xbar[0])
        P, ll = P0, np.zeros(n)
        for k in range(T_):
            xb = Xbar[k + 1]
            Ab = E.abar(Xbar[k], F[k], A[k])
            c = E.boxminus(F[k], xb)
            dm = mv(Ab, d) + (0.0 if drop_c else c)
            Pm = sym(mm(mm(Ab, P), tr(Ab)))
            if not no_q:
                Pm[np.arange(12), np.arange(12)] += Qd
            pmfin = finite(Pm)
            ok = finite(Xbar[k], xb, F[k], A[k], dm) & pmfin
            xp = E.boxplus(xb, dm)
            u = _update(E.boxplus(xb, dm) if at_prediction else xb, dm, Pm, Z[k], None if masks is None else masks[k], Rd, ok, mag, eps)
            d = np.where(ok, u["d"], 0.0)
            P = np.where(ok, u["P"], np.where(pmfin, Pm, P0))
            out["X"].append(np.where(ok, E.boxplus(_safe(xb, ok), d), xb))
            out["P"].append(P)
            out["Xpred"].append(xp)
            out["Ppred"].append(Pm)
            out["Abar"].append(Ab)
            for key in ("nu", "S", "nis"):
                out[key].append(u[key])
            out["used"].append(np.where(ok, u["used"], 0))
            out["status"].append(u["rejected"] * 1 + (~ok) * 2)
            ll = ll + u["ll"]
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(ll=ll, X0=X0, P0=P0)
    return res


def smooth(rec):
    """rts_ref.smooth on the records of pass_ with the prior as node -1"""
    return R.smooth(rec["X"], rec["P"], rec["Xpred"], rec["Ppred"], rec["Abar"], rec["X0"], rec["P0"])


def nodes(sm):
    """the smoothed trajectory as (T+1, 13, n), the initial node first"""
    return np.concatenate([sm["X0"][None], sm["X"]])


# ---- the cost ------------------------------------------------------------------------------------------------------------------
def cost(X0, P0, Xt, Ft, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0):
    """J of the trajectories Xt (T+1, 13, cols) with Ft (T, 13, cols) = F(Xt[k], U[k]); the data of column c are those of instance
    c mod n -> dict of J, Jprior, Jproc, Jmeas, status (cols,)"""
    T_, n, cols = Z.shape[0], X0.shape[1], Xt.shape[2]
    ix = np.arange(cols) % n
    st = np.zeros(cols, np.int64)
    with np.errstate(all="ignore"):
        e0 = E.boxminus(Xt[0], X0[:, ix])
        jp, bad = np.zeros(cols), np.zeros(cols, bool)
        L, b = R.chol(P0)
        for c in range(cols):
            y = np.linalg.solve(L[:, :, ix[c]], e0[:, c]) if np.isfinite(L[:, :, ix[c]]).all() and np.isfinite(e0[:, c]).all() else np.full(12, np.nan)
            jp[c] = 0.5 * (y * y).sum()
        bad = b[ix]
        st |= np.where(bad, P0_NOT_PD, 0)
        st |= np.where(finite(Xt[0]) & finite(X0)[ix], 0, NONFINITE)
        jq, jm = np.zeros(cols), np.zeros(cols)
        for k in range(T_):
            w = E.boxminus(Xt[k + 1], Ft[k])
            st |= np.where(finite(Xt[k + 1], Ft[k]), 0, NONFINITE)
            q = Qd[:, ix]
            jq += 0.5 * np.where(q > 0, w * w / np.where(q > 0, q, 1.0), 0.0).sum(0)
            st |= np.where(((q <= 0) & (w != 0)).any(0), QZERO_DEFECT, 0)
            z = Z[k][:, ix]
            mk = np.full(cols, E.ALL) if masks is None else np.asarray(masks[k]).astype(np.int64)[ix]
            used = (((mk[None, :] >> np.arange(E.ROWS)[:, None]) & 1) == 1) & np.isfinite(z)
            v = np.where(used, z, 0.0) - np.where(used, E.h(Xt[k + 1], mag, eps), 0.0)
            jm += 0.5 * (v * v / Rd[:, ix]).sum(0)
        J = jp + jq + jm
        st |= np.where(np.isfinite(J), 0, NONFINITE)
    return dict(J=J, Jprior=jp, Jproc=jq, Jmeas=jm, status=st)


def candidates(Xbar, Xs, U, ladder=LADDER):
    """Xs (T+1, 13, n): the smoothed nodes -> Xc (T+1, 13, C n), Uc (T, 7, C n); candidate c of instance i at column c n + i"""
    Xc = np.concatenate([np.stack([E.boxplus(Xbar[k], a * E.boxminus(Xs[k], Xbar[k])) for k in range(Xbar.shape[0])]) for a in ladder], axis=2)
    return Xc, np.concatenate([U] * len(ladder), axis=2)


def accept(Jcur, Jc, stc, Xc, Xbar, status, ladder=LADDER):
    """-> Xbar, alpha, Jout, status, margin: |J(alpha) - J(0)| of the decision (the accepted candidate's, else the smallest)"""
    n = Jcur.shape[0]
    Jc, stc = Jc.reshape(len(ladder), n), stc.reshape(len(ladder), n)
    with np.errstate(all="ignore"):
        okc = (Jc < Jcur[None]) & ((stc & NONFINITE) == 0)
    sel = np.where(okc.any(0), okc.argmax(0), -1)
    pick = np.maximum(sel, 0)
    i = np.arange(n)
    Xn = np.where(sel >= 0, Xc.reshape(Xc.shape[0], 13, len(ladder), n)[:, :, pick, i], Xbar)
    alpha = np.where(sel >= 0, np.asarray(ladder)[pick], 0.0)
    Jout = np.where(sel >= 0, Jc[pick, i], Jcur)
    status = status | np.where(sel >= 0, stc[pick, i], NO_DECREASE)
    with np.errstate(all="ignore"):
        gap = np.abs(Jc - Jcur[None])
        # every comparison the decision made: the rejected candidates before the accepted one, and the accepted one
        seen = np.arange(len(ladder))[:, None] <= np.where(sel >= 0, sel, len(ladder))[None, :]
        margin = np.where(seen, gap, np.inf).min(0)
    return Xn, alpha, Jout, status, margin


def solve(orc, X0, P0, Xbar, U, Z, masks, Qd, Rd, iters, ladder=LADDER, mag=E.MAG, eps=0.0, dt=E.DT, **mut):
    """ac_ieks_solve_f32's loop in float64 -> dict of X, P, X0s, P0s (the final smoothed nodes), rec (the last pass), Xbar, cost
    (iters+1, n), alpha (iters, n), status, margin (iters, n), dirs: the Gauss-Newton steps' sizes"""
    Xbar = np.array(Xbar, dtype=np.float64)
    c0 = cost(X0, P0, Xbar, images(orc, Xbar, U, dt), Z, masks, Qd, Rd, mag, eps)
    costs, alphas, margins, status = [c0["J"]], [], [], c0["status"]
    for it in range(iters + 1):
        F, A = linearise(orc, Xbar, U, dt)
        rec = pass_(X0, P0, Xbar, F, A, Z, masks, Qd, Rd, mag, eps, **mut)
        sm = smooth(rec)
        if it == iters:
            break
        Xc, Uc = candidates(Xbar, nodes(sm), U, ladder)
        cc = cost(X0, P0, Xc, images(orc, Xc, Uc, dt), Z, masks, Qd, Rd, mag, eps)
        Xbar, a, J, status, mg = accept(costs[-1], cc["J"], cc["status"], Xc, Xbar, status, ladder)
        costs.append(J)
        alphas.append(a)
        margins.append(mg)
    n = X0.shape[1]
    return dict(X=sm["X"], P=sm["P"], X0s=sm["X0"], P0s=sm["P0"], rec=rec, Xbar=Xbar, cost=np.stack(costs), status=status,
                alpha=np.stack(alphas) if alphas else np.zeros((0, n)), margin=np.stack(margins) if margins else np.zeros((0, n)))


# ---- the dense Gauss-Newton problem and the gradient ------------------------------------------------------------------------------
def dense_step(X0, P0, Xbar, F, A, Z, masks, Qd, Rd, k, mag=E.MAG, eps=0.0):
    """The linearised least-squares problem of instance k in the deviations of all T+1 nodes about Xbar, solved densely:
    prior rows L0^-1 (d_0 - (x0 [-] Xbar[0])), process rows Q^-1/2 (d_{j+1} - Abar_j d_j - c_j), measurement rows
    R^-1/2 (nu_j - H_j d_{j+1}) over the used rows -> the minimiser (T+1, 12)"""
    T_ = Z.shape[0]
    col = lambda a: a[..., k:k + 1]  # noqa: E731
    N = 12 * (T_ + 1)
    rows, rhs = [], []
    Li = np.linalg.inv(np.linalg.cholesky(P0[:, :, k]))
    r = np.zeros((12, N))
    r[:, :12] = Li
    rows.append(r)
    rhs.append(Li @ E.boxminus(col(X0), col(Xbar[0]))[:, 0])
    for j in range(T_):
        Ab = E.abar(col(Xbar[j]), col(F[j]), col(A[j]))[:, :, 0]
        c = E.boxminus(col(F[j]), col(Xbar[j + 1]))[:, 0]
        qi = 1.0 / np.sqrt(Qd[:, k])
        r = np.zeros((12, N))
        r[:, 12 * (j + 1):12 * (j + 2)] = np.diag(qi)
        r[:, 12 * j:12 * (j + 1)] = -qi[:, None] * Ab
        rows.append(r)
        rhs.append(qi * c)
        H = E.H_of(col(Xbar[j + 1]), mag, eps)[:, :, 0]
        nu = (col(Z[j]) - E.h(col(Xbar[j + 1]), mag, eps))[:, 0]
        mk = E.ALL if masks is None else int(masks[j][k])
        used = np.array([((mk >> i) & 1) == 1 and np.isfinite(Z[j][i, k]) for i in range(E.ROWS)])
        ri = 1.0 / np.sqrt(Rd[:, k])
        r = np.zeros((int(used.sum()), N))
        r[:, 12 * (j + 1):12 * (j + 2)] = (ri[:, None] * H)[used]
        rows.append(r)
        rhs.append((ri * nu)[used])
    sol = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    return sol.reshape(T_ + 1, 12)


def grad_norm(orc, X0, P0, Xt, U, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0, dt=E.DT, step=1e-6):
    """|grad J| per instance at the trajectory Xt in the chart coordinates of its own nodes, by central differences, each
    coordinate scaled by sqrt of the prior variance of its kind (so that the norm has no units) -> (n,)"""
    T1, n = Xt.shape[0], Xt.shape[2]
    g2 = np.zeros(n)
    J = lambda X: cost(X0, P0, X, images(orc, X, U, dt), Z, masks, Qd, Rd, mag, eps)["J"]  # noqa: E731
    for k in range(T1):
        for j in range(12):
            s = E.SIG_P0[j]
            e = np.zeros((12, n))
            e[j] = step * s
            Xp, Xm = Xt.copy(), Xt.copy()
            Xp[k], Xm[k] = E.boxplus(Xt[k], e), E.boxplus(Xt[k], -e)
            g2 += ((J(Xp) - J(Xm)) / (2 * step)) ** 2
    return np.sqrt(g2)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
DESCENT_T = 6
P0_SCALE = 10.0
BATCH = 19  # the first 19 instances of a chain: the GPU tests' batch
_INPUTS = {}


def inputs(name, T_=DESCENT_T, sigmas=3.0, seed=0, scale=1.0):
    """The filter chain of ekf_ref.chain_inputs(name) with T_ steps, every row used at every step, the prior covariance
    (scale SIG_P0)^2 and the prior mean offset from the truth by `sigmas` standard deviations of P0 along a seeded direction.
    Everything the host build and the device read is float32-exact.  -> the chain's dict plus X0, U (T, 7, m), masks, Xekf
    (T+1, 13, m): the EKF + RTS trajectory from that prior, Xfilt (T+1, 13, m): the prior mean and the filtered nodes.
    scale = 1 (the parity tests): with ekf_ref's own P0 the EKF + RTS trajectory is the MAP trajectory to 1e-5 of J, and a line
    search from it is decided by rounding.  descent_inputs: scale = P0_SCALE (20 m, 5 m/s, 0.3 - 0.5 rad, 0.5 rad/s: the large
    initial error the iteration is for) and the solve starts from Xfilt: two iterations each lower J by more than 1e-3 of it."""
    key = (name, T_, sigmas, seed, scale)
    if key in _INPUTS:
        return _INPUTS[key]
    d = dict(E.chain_inputs(name, T_=T_, seed=seed))
    m = min(d["x"].shape[1], BATCH)
    for k in ("x", "u", "P", "z", "Qd", "Rd", "truth", "Z", "masks"):
        d[k] = d[k][..., :m]
    d["P"] = f32x(d["P"] * scale ** 2)
    rng = np.random.default_rng(300 + seed)
    off = np.zeros((12, m))
    for k in range(m):
        v = np.linalg.cholesky(d["P"][:, :, k]) @ rng.standard_normal(12)
        off[:, k] = sigmas * v / np.sqrt(v @ np.linalg.solve(d["P"][:, :, k], v))
    d["X0"] = f32x(E.boxplus(d["truth"], off))
    d["U"] = np.repeat(d["u"][None], T_, axis=0)
    d["masks"] = np.full((T_, m), E.ALL, np.int32)
    rec = R.filter_records(d["orc"].step_sens, d["X0"], d["P"], d["u"], d["Z"], d["masks"], d["Qd"], d["Rd"], E.MAG, d["eps"])
    sm = R.smooth(rec["X"], rec["P"], rec["Xpred"], rec["Ppred"], rec["Abar"], rec["X0"], rec["P0"])
    d["Xekf"] = f32x(nodes(sm))
    d["Xfilt"] = f32x(np.concatenate([d["X0"][None], rec["X"]]))
    _INPUTS[key] = d
    return d


DESCENT_ITERS = 2


def descent_inputs(name):
    return inputs(name, scale=P0_SCALE)


# ---- measures --------------------------------------------------------------------------------------------------------------------
def pass_errors(got, ref):
    """the measures of a pass `got` against `ref` (dicts of pass_), worst over the steps -> dict of (n,)"""
    T_ = ref["X"].shape[0]
    mx = lambda f: np.max([f(t) for t in range(T_)], axis=0)  # noqa: E731
    return {"x": mx(lambda t: E.err_state(got["X"][t], ref["X"][t])), "xpred": mx(lambda t: E.err_state(got["Xpred"][t], ref["Xpred"][t])),
            "P": mx(lambda t: E.err_P(got["P"][t], ref["P"][t])), "S": mx(lambda t: E.err_S(got["S"][t], ref["S"][t])),
            "nu": mx(lambda t: E.err_nu(got["nu"][t], ref["nu"][t], ref["S"][t])),
            "nis": mx(lambda t: E.err_scalar(got["nis"][t], ref["nis"][t])), "ll": E.err_scalar(got["ll"], ref["ll"]),
            "Ppred": mx(lambda t: E.err_P(got["Ppred"][t], ref["Ppred"][t])),
            "Abar": mx(lambda t: E.L.unit_max_rel(got["Abar"][t], ref["Abar"][t]))}


COST_KEYS = ("J", "Jprior", "Jproc", "Jmeas")


def cost_errors(got, ref):
    return {k: E.err_scalar(got[k], ref[k]) for k in COST_KEYS}


def checked(e32):
    keep = np.ones(len(next(iter(e32.values()))), bool)
    for k, v in e32.items():
        keep &= v <= 2 * E32_WORST[k]
    return keep


def hold(name, dev, e32, distinct):
    """ekf_ref.hold's rule with this file's E32_WORST.  Prints each figure before it asserts."""
    keep = checked(e32)
    left = int((~keep[:distinct]).sum())
    worst = {k: (float(dev[k][keep].max()), float(e32[k][keep].max())) for k in dev} if keep.any() else {}
    print(f"[ieks] {name}: left out {left}/{distinct}; " + ", ".join(f"{k} dev {d:.2e} e32 {e:.2e}" for k, (d, e) in worst.items()))
    assert left <= 0.05 * distinct, (name, "e32 condition: left out", left, "of", distinct, {k: float(v.max()) for k, v in e32.items()})
    for k, (d, e) in worst.items():
        assert d <= 8 * e, (name, k, d, e)


# ---- the host build's entry points (tests/host_ieks/ieks_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) ------------------------
_fp, _ip = E._fp, E._ip


def _lad(ladder):
    return (C.c_float * len(ladder))(*[float(a) for a in ladder])


def host_pass(X0, P0, Xbar, F, A, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0, header=None):
    """the float32 host build on float32-rounded inputs -> the dict of pass_ (float64 / int arrays; P32, Ppred32: the float32 ones)"""
    from tests.test_host_ieks import lib_host

    T_, n = Z.shape[0], X0.shape[1]
    a = [c32(X0), c32(np.reshape(P0, (144, n))), c32(Xbar), c32(F), c32(np.reshape(A, (T_, 169, n))), c32(Z)]
    mk = None if masks is None else np.ascontiguousarray(masks, dtype=np.int32)
    q, r = c32(Qd), c32(Rd)
    f = lambda *s: np.full(s, 12345.0, np.float32)  # noqa: E731
    Xs, Ps, ll, nu, S, nis = f(T_, 13, n), f(T_, 12, 12, n), f(n), f(T_, E.ROWS, n), f(T_, E.ROWS, n), f(T_, n)
    used, st = np.full((T_, n), -1, np.int32), np.full((T_, n), -1, np.int32)
    Xp, Pp, Ab = f(T_, 13, n), f(T_, 12, 12, n), f(T_, 12, 12, n)
    o = E.ekf_opts(mag)
    assert lib_host(header).host_ieks_pass(C.byref(o), C.c_float(eps), *[_fp(v) for v in a], _ip(mk), _fp(q), _fp(r), n, T_, _fp(Xs), _fp(Ps),
                                           _fp(ll), _fp(nu), _fp(S), _fp(nis), _ip(used), _ip(st), _fp(Xp), _fp(Pp), _fp(Ab)) == 0
    d64 = lambda v: v.astype(np.float64)  # noqa: E731
    return dict(X=d64(Xs), P=d64(Ps), Xpred=d64(Xp), Ppred=d64(Pp), Abar=d64(Ab), nu=d64(nu), S=d64(S), nis=d64(nis), used=used, status=st,
                ll=d64(ll), X0=np.asarray(X0, dtype=np.float64), P0=np.asarray(P0, dtype=np.float64), P32=Ps, Ppred32=Pp, Abar32=Ab,
                X32=Xs, raw=dict(X=Xs, P=Ps, Xpred=Xp, Ppred=Pp, Abar=Ab, nu=nu, S=S, nis=nis, used=used, status=st, ll=ll))


def host_cost(X0, P0, Xt, Ft, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0, header=None):
    from tests.test_host_ieks import lib_host

    T_, n, cols = Z.shape[0], X0.shape[1], Xt.shape[2]
    assert cols % n == 0
    a = [c32(X0), c32(np.reshape(P0, (144, n))), c32(Xt), c32(Ft), c32(Z)]
    mk = None if masks is None else np.ascontiguousarray(masks, dtype=np.int32)
    q, r = c32(Qd), c32(Rd)
    J, Jp, Jq, Jm = (np.full(cols, 12345.0, np.float32) for _ in range(4))
    st = np.full(cols, -1, np.int32)
    o = E.ekf_opts(mag)
    assert lib_host(header).host_ieks_cost(C.byref(o), C.c_float(eps), *[_fp(v) for v in a], _ip(mk), _fp(q), _fp(r), n, cols // n, T_, _fp(J),
                                           _fp(Jp), _fp(Jq), _fp(Jm), _ip(st)) == 0
    return dict(J=J.astype(np.float64), Jprior=Jp.astype(np.float64), Jproc=Jq.astype(np.float64), Jmeas=Jm.astype(np.float64), status=st,
                raw=dict(J=J, Jprior=Jp, Jproc=Jq, Jmeas=Jm, status=st))


def host_candidates(Xbar, Xs, U, ladder=LADDER):
    from tests.test_host_ieks import lib_host

    T_, n, Cn = U.shape[0], U.shape[2], len(ladder)
    Xc, Uc = np.zeros((T_ + 1, 13, Cn * n), np.float32), np.zeros((T_, 7, Cn * n), np.float32)
    assert lib_host().host_ieks_candidates(_fp(c32(Xbar)), _fp(c32(Xs[0])), _fp(c32(Xs[1:])), _fp(c32(U)), _lad(ladder), Cn, n, T_, _fp(Xc),
                                           _fp(Uc)) == 0
    return Xc, Uc


def host_accept(Jcur, Jc, stc, Xc, Xbar, status, ladder=LADDER):
    from tests.test_host_ieks import lib_host

    T_, n = Xbar.shape[0] - 1, Xbar.shape[2]
    Xb, st = c32(Xbar).copy(), np.ascontiguousarray(status, dtype=np.int32).copy()
    alpha, Jout = np.zeros(n, np.float32), np.zeros(n, np.float32)
    assert lib_host().host_ieks_accept(_fp(c32(Jcur)), _fp(c32(Jc)), _ip(np.ascontiguousarray(stc, dtype=np.int32)), _fp(c32(Xc)), _lad(ladder),
                                       len(ladder), n, T_, _fp(Xb), _fp(alpha), _fp(Jout), _ip(st)) == 0
    return Xb, alpha, Jout, st


# ---- the Gauss-Newton property --------------------------------------------------------------------------------------------------
def gn_case(name, s, T_=3, m=4, seed=0):
    """A log of T_ steps whose deviations from the nominal all scale with s: the truth is driven by s x the process noise, measured
    with s x the sensor noise; the prior mean is the truth [+] s N(0, P0) and the nominal the truth [+] s/2 N(0, diag SIG_P0^2) node
    by node.  The weights P0, Qd, Rd are not scaled.  Float32-exact.  The same seed draws the same directions for every s."""
    d = E.chain_inputs(name, T_=T_)
    rng = np.random.default_rng(400 + seed)
    cut = lambda a: a[..., :m]  # noqa: E731
    orc, u, P0, Qd, Rd, eps = d["orc"], cut(d["u"]), cut(d["P"]), cut(d["Qd"]), cut(d["Rd"]), d["eps"]
    Xt, Z = [cut(d["truth"])], []
    for _ in range(T_):
        Xt.append(E.boxplus(orc.state_update(Xt[-1], u, E.DT), s * np.sqrt(Qd) * rng.standard_normal((12, m))))
        Z.append(f32x(E.h(Xt[-1], E.MAG, eps) + s * np.sqrt(Rd) * rng.standard_normal((E.ROWS, m))))
    off = np.stack([np.linalg.cholesky(P0[:, :, k]) @ rng.standard_normal(12) for k in range(m)], axis=1)
    X0 = f32x(E.boxplus(Xt[0], s * off))
    Xbar = f32x(np.stack([E.boxplus(x, 0.5 * s * E.SIG_P0[:, None] * rng.standard_normal((12, m))) for x in Xt]))
    return dict(orc=orc, eps=eps, X0=X0, P0=P0, Xbar=Xbar, U=np.repeat(u[None], T_, axis=0), Z=np.stack(Z), masks=None, Qd=Qd, Rd=Rd)


def gn_mismatch(pass_fn, c):
    """|(X^s [-] Xbar) - dense| / |dense| per instance, every coordinate in units of SIG_P0; pass_fn: pass_ or host_pass"""
    F, A = linearise(c["orc"], c["Xbar"], c["U"])
    F, A = f32x(F), f32x(A)
    rec = pass_fn(c["X0"], c["P0"], c["Xbar"], F, A, c["Z"], c["masks"], c["Qd"], c["Rd"], E.MAG, c["eps"])
    Xs = nodes(smooth(rec))
    T1, m = Xs.shape[0], Xs.shape[2]
    delta = np.stack([E.boxminus(Xs[k], c["Xbar"][k]) for k in range(T1)])
    dense = np.stack([dense_step(c["X0"], c["P0"], c["Xbar"], F, A, c["Z"], c["masks"], c["Qd"], c["Rd"], k, E.MAG, c["eps"]) for k in range(m)], axis=2)
    sg = E.SIG_P0[None, :, None]
    return np.sqrt((((delta - dense) / sg) ** 2).sum((0, 1)) / ((dense / sg) ** 2).sum((0, 1)))


def host_solve(orc, X0, P0, Xbar, U, Z, masks, Qd, Rd, iters, ladder=LADDER, mag=E.MAG, eps=0.0, dt=E.DT):
    """solve()'s loop made of the host build's pieces (the float64 oracle's F and A, rounded to float32) -> dict of cost, alpha, status"""
    Xbar = f32x(Xbar)
    data = (Z, masks, Qd, Rd, mag, eps)
    c0 = host_cost(X0, P0, Xbar, f32x(images(orc, Xbar, U, dt)), *data)
    costs, alphas, status = [c0["raw"]["J"]], [], c0["status"]
    for _ in range(iters):
        F, A = linearise(orc, Xbar, U, dt)
        rec = host_pass(X0, P0, Xbar, f32x(F), f32x(A), *data)
        sm = R.host_smooth(rec["X"], rec["P"], rec["Xpred"], rec["Ppred"], rec["Abar"], rec["X0"], rec["P0"], gains=False)
        Xc, Uc = host_candidates(Xbar, nodes(sm), U, ladder)
        cc = host_cost(X0, P0, Xc.astype(np.float64), f32x(images(orc, Xc.astype(np.float64), Uc.astype(np.float64), dt)), *data)
        Xb, a, J, status = host_accept(costs[-1], cc["raw"]["J"], cc["status"], Xc, Xbar, status, ladder)
        Xbar = Xb.astype(np.float64)
        costs.append(J)
        alphas.append(a)
    return dict(cost=np.stack(costs).astype(np.float64), alpha=np.stack(alphas).astype(np.float64), status=status, Xbar=Xbar)
