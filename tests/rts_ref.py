"""Float64 restatement of the Rauch-Tung-Striebel smoother over the trace of the extended Kalman filter
(aircraft_amd/csrc/ac_rts.hpp; include/aircraft_hip.h, ac_ekf_smooth_f32) for the tests, on top of
tests/ekf_ref.py: the backward recursion, the block-tridiagonal joint information matrix it is checked against, the filter
chain that records what the smoother reads, the error measures, the host build's entry point and the recorded worst float32
errors E32_WORST.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import numpy as np

from tests import ekf_ref as E

NOT_PD, NONFINITE = 1, 2

# e32: the host build (g++, -ffp-contract=off) against this restatement on identical float32-rounded records (those of the
# float64 filter chain of ekf_ref.chain_inputs), worst instance and node over ekf_ref.MODELS, with and without the initial node.
# tests/test_host_rts.py measures them and fails if they are exceeded; DESIGN.md §4.15 quotes them.  The GPU tests check an
# instance when its e32 is within 2 x these and hold the device to 8 x the worst e32 of the checked instances of its batch.
# Measures: x err_state, P err_P (both worst over the nodes), C err_C (worst over the links).  The worst node is the initial one
# (link 0 factors Abar_0 P0 Abar_0' + Q with the wide P0 of ekf_ref.inputs); without it the chains give x 3.9e-7, P 9.7e-6, C 2.5e-6.
E32_WORST = {"x": 6.0e-6, "P": 7.5e-5, "C": 2.9e-5}

mm, mv, tr, sym, f32x, c32 = E.mm, E.mv, E.tr, E.sym, E.f32x, E.c32


# ---- the recursion ------------------------------------------------------------------------------------------------------------
def chol(A):
    """plain Cholesky of A (12, 12, n), column by column -> L, bad (n,): a pivot was <= 0 or not finite (the pivot is then
    taken as 1 and the factor is meaningless)"""
    n = A.shape[2]
    L, bad = np.zeros_like(A), np.zeros(n, bool)
    for j in range(12):
        d = A[j, j] - (L[j, :j] ** 2).sum(0)
        b = ~((d > 0) & np.isfinite(d))
        bad |= b
        L[j, j] = np.sqrt(np.where(b, 1.0, d))
        for r in range(j + 1, 12):
            L[r, j] = (A[r, j] - (L[r, :j] * L[j, :j]).sum(0)) / L[j, j]
    return L, bad


def solve_right(M, L):
    """M (L L')^-1, row by row: two triangular solves"""
    Y = np.zeros_like(M)
    for j in range(12):
        Y[:, j] = (M[:, j] - np.einsum("rcn,cn->rn", Y[:, :j], L[j, :j])) / L[j, j]
    X = np.zeros_like(M)
    for j in range(11, -1, -1):
        X[:, j] = (Y[:, j] - np.einsum("rcn,cn->rn", X[:, j + 1:], L[j + 1:, j])) / L[j, j]
    return X


def finite(*arrays):
    n = arrays[0].shape[-1]
    return np.all([np.isfinite(a).reshape(-1, n).all(axis=0) for a in arrays], axis=0)


def smooth(Xf, Pf, Xpred, Ppred, Abar, X0=None, P0=None):
    """The backward recursion over the records of a filter run (leading axis T; X0 (13, n), P0 (12, 12, n): node -1 or None)
    -> dict of X (T, 13, n), P (T, 12, 12, n), X0, P0 (None without node -1), C (T, 12, 12, n), status (T, n)"""
    T_, n = Xf.shape[0], Xf.shape[2]
    Xs, Ps, Cg = np.zeros((T_, 13, n)), np.zeros((T_, 12, 12, n)), np.zeros((T_, 12, 12, n))
    status = np.zeros((T_, n), np.int32)
    xs, ps = Xf[-1].copy(), Pf[-1].copy()
    Xs[-1], Ps[-1] = xs, ps
    Xs0 = Ps0 = None
    for k in range(T_ - 1, -1 if X0 is not None else 0, -1):
        xh, ph = (Xf[k - 1], Pf[k - 1]) if k > 0 else (X0, P0)
        with np.errstate(all="ignore"):
            fin = finite(xh, ph, Xpred[k], Ppred[k], Abar[k], xs, ps)
            L, bad = chol(np.where(fin, Ppred[k], np.eye(12)[:, :, None]))
            ok = fin & ~bad
            Ck = np.where(ok, solve_right(mm(ph, tr(Abar[k])), L), 0.0)
            d = mv(Ck, np.where(ok, E.boxminus(xs, Xpred[k]), 0.0))
            xn = np.where(ok, E.boxplus(np.where(ok, xh, Xf[-1]), d), xh)
            pn = np.where(ok, sym(ph + mm(mm(Ck, np.where(ok, ps - Ppred[k], 0.0)), tr(Ck))), ph)
        Cg[k] = Ck
        status[k] = np.where(fin, bad * NOT_PD, NONFINITE)
        xs, ps = xn, pn
        if k > 0:
            Xs[k - 1], Ps[k - 1] = xs, ps
        else:
            Xs0, Ps0 = xs, ps
    return dict(X=Xs, P=Ps, X0=Xs0, P0=Ps0, C=Cg, status=status)


def joint_marginals(Pf, Ppred, Abar, P0=None):
    """The smoothed covariances of ONE instance (Pf, Ppred, Abar (T, 12, 12)) from the records alone, without the recursion:
    the diagonal blocks of the inverse of the block-tridiagonal joint information matrix with the prior P_0^-1 on node 0 (with
    P0: P0^-1 on node -1, link 0 and node 0's measurements as well), per link Q_k = P-_k - Abar_k P_{k-1} Abar_k', per node the
    measurement information P_k^-1 - (P-_k)^-1 -> (T, 12, 12) (with P0: (T + 1, 12, 12), node -1 first)"""
    T_ = Pf.shape[0]
    first = 0 if P0 is not None else 1  # the first link
    N = T_ + (1 if P0 is not None else 0)
    at = (lambda k: k + 1) if P0 is not None else (lambda k: k)  # block index of node k
    J = np.zeros((12 * N, 12 * N))
    blk = lambda a, b: (slice(12 * a, 12 * a + 12), slice(12 * b, 12 * b + 12))  # noqa: E731
    J[blk(0, 0)] += np.linalg.inv(P0 if P0 is not None else Pf[0])
    for k in range(first, T_):
        Pprev = Pf[k - 1] if k > 0 else P0
        A = Abar[k]
        Qi = np.linalg.inv(Ppred[k] - A @ Pprev @ A.T)
        a, b = at(k - 1), at(k)
        J[blk(a, a)] += A.T @ Qi @ A
        J[blk(a, b)] -= A.T @ Qi
        J[blk(b, a)] -= Qi @ A
        J[blk(b, b)] += Qi + np.linalg.inv(Pf[k]) - np.linalg.inv(Ppred[k])
    S = np.linalg.inv(J)
    return np.stack([S[blk(a, a)] for a in range(N)])


# ---- the filter chain that records what the smoother reads --------------------------------------------------------------------
def filter_records(sens_fn, x, P, u, Z, masks, Qd, Rd, mag=E.MAG, eps=0.0, dt=E.DT):
    """T steps of the float64 filter (ekf_ref.step) from (x, P) -> dict of X, P, Xpred, Ppred, Abar, status stacked on a leading
    axis, and X0, P0"""
    out = {k: [] for k in ("X", "P", "Xpred", "Ppred", "Abar", "status")}
    x0, P0 = x, P
    for t in range(Z.shape[0]):
        xp, A = sens_fn(x, u, dt)[:2]
        o = E.step(x, P, xp, A, Z[t], None if masks is None else masks[t], Qd, Rd, mag, eps)
        for k in out:
            out[k].append(o[k])
        x, P = o["X"], o["P"]
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(X0=x0, P0=P0)
    return res


_RECORDS = {}


def chain_records(name):
    """the records of the float64 filter on ekf_ref.chain_inputs(name), rounded to float32 (so that every reader of them sees
    identical inputs; P, Ppred stay symmetric) -> dict of X, P, Xpred, Ppred, Abar (T, .., m), X0, P0"""
    if name not in _RECORDS:
        c = E.chain_inputs(name)
        r = filter_records(c["orc"].step_sens, c["x"], c["P"], c["u"], c["Z"], c["masks"], c["Qd"], c["Rd"], E.MAG, c["eps"])
        assert (r["status"] == 0).all()
        _RECORDS[name] = {k: f32x(r[k]) for k in ("X", "P", "Xpred", "Ppred", "Abar", "X0", "P0")}
    return _RECORDS[name]


# ---- measures (per instance, (n,)) --------------------------------------------------------------------------------------------
def err_C(a, ref, Pprev, Ppred):
    """max |dC_ij| sqrt(P-_jj / P_ii) with the link's own P_{k-1} and P-_k"""
    i = np.arange(12)
    with np.errstate(all="ignore"):
        s = np.sqrt(Ppred[i, i])[None, :] / np.sqrt(Pprev[i, i])[:, None]
        return (np.abs(a - ref) * s).reshape(144, -1).max(axis=0)


def errors(got, ref, rec, initial):
    """the measures of a smoother run `got` against `ref` (dicts of smooth()) on the records `rec` (dict with P, Ppred, P0),
    worst over nodes and links -> dict of (n,): x, P and, when got has gains, C"""
    T_ = ref["X"].shape[0]
    ex = [E.err_state(got["X"][t], ref["X"][t]) for t in range(T_)]
    eP = [E.err_P(got["P"][t], ref["P"][t]) for t in range(T_)]
    if initial:
        ex.append(E.err_state(got["X0"], ref["X0"]))
        eP.append(E.err_P(got["P0"], ref["P0"]))
    e = {"x": np.max(ex, axis=0), "P": np.max(eP, axis=0)}
    if got.get("C") is not None:
        eC = [np.zeros_like(e["x"])]
        for k in range(0 if initial else 1, T_):
            Pprev = rec["P"][k - 1] if k > 0 else rec["P0"]
            eC.append(err_C(got["C"][k], ref["C"][k], Pprev, rec["Ppred"][k]))
        e["C"] = np.max(eC, axis=0)
    return e


def checked(e32):
    """instances whose host/float64 pair is within 2 x the recorded worst in every measure"""
    keep = np.ones(len(e32["x"]), bool)
    for k, v in e32.items():
        keep &= v <= 2 * E32_WORST[k]
    return keep


def hold(name, dev, e32, distinct):
    """ekf_ref.hold's rule with this file's E32_WORST: at most 5 % of the batch's distinct instances left out; the device
    within 8 x the worst e32 of the checked instances, measure by measure.  Prints each figure before it asserts."""
    keep = checked(e32)
    left = int((~keep[:distinct]).sum())
    worst = {k: (float(dev[k][keep].max()), float(e32[k][keep].max())) for k in dev} if keep.any() else {}
    print(f"[rts] {name}: left out {left}/{distinct}; " + ", ".join(f"{k} dev {d:.2e} e32 {e:.2e}" for k, (d, e) in worst.items()))
    assert left <= 0.05 * distinct, (name, "e32 condition: left out", left, "of", distinct, {k: float(v.max()) for k, v in e32.items()})
    for k, (d, e) in worst.items():
        assert d <= 8 * e, (name, k, d, e)


# ---- the host build's entry point (tests/host_rts/rts_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) -----------------------
def host_smooth(Xf, Pf, Xpred, Ppred, Abar, X0=None, P0=None, gains=True, header=None):
    """the float32 host build on float32-rounded records -> the dict of smooth() (float64 / int arrays; P32: the float32 P)"""
    from tests.test_host_rts import lib_host

    T_, n = Xf.shape[0], Xf.shape[2]
    a = [None if v is None else c32(v) for v in (X0, P0, Xf, Pf, Xpred, Ppred, Abar)]
    f = lambda *s: np.full(s, 12345.0, np.float32)  # noqa: E731
    Xs, Ps, Cg = f(T_, 13, n), f(T_, 12, 12, n), f(T_, 12, 12, n) if gains else None
    Xs0, Ps0 = (f(13, n), f(12, 12, n)) if X0 is not None else (None, None)
    st = np.full((T_, n), -1, np.int32)
    assert lib_host(header).host_rts_smooth(*[E._fp(v) for v in a], n, T_, E._fp(Xs), E._fp(Ps), E._fp(Xs0), E._fp(Ps0), E._fp(Cg),
                                            E._ip(st)) == 0
    d64 = lambda v: None if v is None else v.astype(np.float64)  # noqa: E731
    return dict(X=d64(Xs), P=d64(Ps), X0=d64(Xs0), P0=d64(Ps0), C=d64(Cg), status=st, P32=Ps, P032=Ps0, X32=Xs)
