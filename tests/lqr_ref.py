"""Float64 restatement of the LQR stabiliser about steady-flight trims (aircraft_amd/csrc/ac_lqr.hpp; include/aircraft_hip.h,
ac_lqr_f32) for the tests: the 12-coordinate steady-flight chart and its inverse, the analytic T = dx/dxi
and E = dxi/dx, the projection A_xi = E(x+) A T(x), B_xi = E(x+) B, the structured doubling solve of the discrete Riccati
equation, the gain, its expansion to raw-state gains, the closed loop through the oracle, the error measures, the host
build's entry points and the grid.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import numpy as np

from tests import trim_ref as T

IGNORABLE = (0, 1, 2, 8)          # along-track, cross-track, down, heading: they feed no other coordinate
Q8 = np.array([0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1], dtype=np.float64)    # the default: stability augmentation
Q11 = np.array([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], dtype=np.float64)   # path holding without along-track
Q12 = np.ones(12)
SELECTIONS = {"8": Q8, "11": Q11, "12": Q12}
R1 = np.ones(7)
DT = 0.01
ITERS = 24
TOL = 1e-6
SIZES = (1, 3, 4, 5, 63, 64, 65, 257)

# e32: the host build (g++, -ffp-contract=off) against float64 on identical float32-rounded inputs, worst instance over
# the cubic-fit and default models on the grid, the 8, 11 and 12 coordinate selections (tests/test_host_lqr.py measures
# them and fails if they are exceeded; DESIGN.md §4.13 quotes them).  The GPU tests assert the host/float64 pair within
# 2 x these first, then the device within 8 x the instance's own e32.
# proj: max |d A_xi|, |d B_xi| (absolute; max |A_xi| is about 1: the 70 m/s terms of T and E cancel to g dt);
# P: max |dP| / max |P|;  K: max |dK| / max |K|;  gains: max |dK_x| / max |K_x| per node;
# xi: max |d xi| / max(|xi|, 1) for errors of up to 5 m, 1 m/s, 0.05 rad, 0.05 rad/s.
E32_WORST = {"proj": 3.0e-5, "P": 1.0e-4, "K": 4.0e-5, "gains": 1.8e-6, "xi": 9.0e-6}


def f32x(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- rotations ---------------------------------------------------------------------------------------------------------------
def unit(q):
    return q / np.sqrt((q * q).sum(0))


def yaw(q):
    """yaw of a unit xyzw quaternion (4, n)"""
    x, y, z, w = q
    return np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))


def rotmat(q):
    """R(q) (3, 3, n): body -> NED for a unit xyzw quaternion"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def heading(q):
    """Z = R_z(yaw(q)) (3, 3, n)"""
    psi = yaw(q)
    c, s, o, e = np.cos(psi), np.sin(psi), np.zeros_like(psi), np.ones_like(psi)
    return np.array([[c, -s, o], [s, c, o], [o, o, e]])


def skew(v):
    o = np.zeros_like(v[0])
    return np.array([[o, -v[2], v[1]], [v[2], o, -v[0]], [-v[1], v[0], o]])


def mv(M, v):
    return np.einsum("ijn,jn->in", M, v)


def mtv(M, v):
    return np.einsum("jin,jn->in", M, v)


def mm(A, B):
    return np.einsum("ikn,kjn->ijn", A, B)


def tr(A):
    return np.swapaxes(A, 0, 1)


# ---- the chart ---------------------------------------------------------------------------------------------------------------
def chart(x, xb):
    """xi (12, n) of the state x (13, n) about the nominal xb (13, n)"""
    q, qb = unit(x[6:10]), unit(xb[6:10])
    Z = heading(qb)
    d = T.qmul(q, T.qconj(qb))
    d = np.where(d[3] < 0, -d, d)
    return np.concatenate([mtv(Z, x[0:3] - xb[0:3]), mtv(rotmat(q), x[3:6]) - mtv(rotmat(qb), xb[3:6]),
                           mtv(Z, 2 * d[:3]), x[10:13] - xb[10:13]])


def unchart(xi, xb):
    """the state x with chart(x, xb) = xi (its attitude has the norm of xb's; |xi[6:9]| < 2)"""
    qb = unit(xb[6:10])
    Z = heading(qb)
    dv = 0.5 * mv(Z, xi[6:9])
    d = np.concatenate([dv, np.sqrt(1 - (dv * dv).sum(0))[None]])
    q = T.qmul(d, xb[6:10])  # (xi = 0 gives xb itself, whatever the norm of its attitude)
    vb = mtv(rotmat(qb), xb[3:6]) + xi[3:6]
    return np.concatenate([xb[0:3] + mv(Z, xi[0:3]), mv(rotmat(unit(q)), vb), q, xb[10:13] + xi[9:12]])


def T_of(xb):
    """T = dx/dxi at xi = 0 (13, 12, n)"""
    n = xb.shape[1]
    qb = unit(xb[6:10])
    Z, R = heading(qb), rotmat(qb)
    Tm = np.zeros((13, 12, n))
    Tm[0:3, 0:3] = Z
    Tm[3:6, 3:6] = R
    Tm[3:6, 6:9] = -mm(skew(xb[3:6]), Z)
    M = np.zeros((4, 3, n))
    qr = xb[6:10]  # not normalised: the tangent of d (x) q_b at xb itself (a norm error of 1e-7 times |v| would show in A_xi)
    M[0:3] = qr[3] * np.eye(3)[:, :, None] - skew(qr[0:3])
    M[3] = -qr[0:3]
    Tm[6:10, 6:9] = 0.5 * mm(M, Z)
    Tm[10:13, 9:12] = np.eye(3)[:, :, None]
    return Tm


def E_of(xb):
    """E = dxi/dx at x = xb (12, 13, n); it annihilates the quaternion-norm direction"""
    n = xb.shape[1]
    nq = np.sqrt((xb[6:10] ** 2).sum(0))
    qb = xb[6:10] / nq
    Z, R = heading(qb), rotmat(qb)
    N = np.zeros((3, 4, n))
    N[:, 0:3] = qb[3] * np.eye(3)[:, :, None] + skew(qb[0:3])
    N[:, 3] = -qb[0:3]
    N2 = 2 * N / nq
    Em = np.zeros((12, 13, n))
    Em[0:3, 0:3] = tr(Z)
    Em[3:6, 3:6] = tr(R)
    Em[3:6, 6:10] = mm(mm(tr(R), skew(xb[3:6])), N2)
    Em[6:9, 6:10] = mm(tr(Z), N2)
    Em[9:12, 10:13] = np.eye(3)[:, :, None]
    return Em


def project(xb, xbp, A, B):
    """A_xi = E(x+) A T(x) (12, 12, n), B_xi = E(x+) B (12, 7, n)"""
    E = E_of(xbp)
    return mm(mm(E, A), T_of(xb)), mm(E, B)


def oracle_projection(orc, x, u, dt=DT):
    xp, A, B, _ = orc.step_sens(x, u, dt)
    return project(x, xp, A, B)


# ---- the Riccati solve -------------------------------------------------------------------------------------------------------
def dropped(q):
    return [i for i in IGNORABLE if q[i] == 0]


def reduce(A, B, q):
    """rows and columns of the dropped coordinates zeroed (copies)"""
    A, B = np.array(A, dtype=np.float64), np.array(B, dtype=np.float64)
    d = dropped(q)
    A[d] = 0
    A[:, d] = 0
    B[d] = 0
    return A, B


def sda(A, B, q, r, iters=ITERS, tol=TOL):
    """One instance: structured doubling on the reduced (A, B) -> P, K, residual, status, iterations used.
    status 0 converged, 1 not within iters, 2 breakdown, 3 non-finite input"""
    nan = (np.full((12, 12), np.nan), np.full((7, 12), np.nan), np.nan)
    if not (np.isfinite(A).all() and np.isfinite(B).all()):
        return (*nan, 3, 0)
    A0, B0 = reduce(A, B, q)
    Ak, G, H = A0.copy(), (B0 / r) @ B0.T, np.diag(np.asarray(q, dtype=np.float64))
    status, used = 1, iters
    with np.errstate(all="ignore"):
        for k in range(iters):
            W = np.eye(12) + G @ H
            try:
                X = np.linalg.solve(W, np.concatenate([Ak, G], axis=1))
            except np.linalg.LinAlgError:
                return (*nan, 2, k + 1)
            X1, X2 = X[:, :12], X[:, 12:]
            An = Ak @ X1
            Gn = G + Ak @ X2 @ Ak.T
            Hn = H + Ak.T @ (H @ X1)
            Gn, Hn = 0.5 * (Gn + Gn.T), 0.5 * (Hn + Hn.T)
            if not (np.isfinite(An).all() and np.isfinite(Gn).all() and np.isfinite(Hn).all()):
                return (*nan, 2, k + 1)
            conv = np.abs(Hn - H).max() < tol * np.abs(Hn).max()
            Ak, G, H = An, Gn, Hn
            if conv:
                status, used = 0, k + 1
                break
    K = gain(A0, B0, H, r)
    return H, K, residual(A0, B0, H, K, q), status, used


def sda32(A, B, q, r, iters=ITERS, tol=TOL):
    """The same iteration in NumPy/LAPACK float32 (one instance) -> P, K as float64: where a float32 solve lands."""
    f = np.float32
    A0, B0 = (m.astype(f) for m in reduce(A, B, q))
    r = np.asarray(r, dtype=f)
    Ak, G, H = A0.copy(), (B0 / r) @ B0.T, np.diag(np.asarray(q, dtype=f))
    for _ in range(iters):
        X = np.linalg.solve(np.eye(12, dtype=f) + G @ H, np.concatenate([Ak, G], axis=1))
        An, Gn, Hn = Ak @ X[:, :12], G + Ak @ X[:, 12:] @ Ak.T, H + Ak.T @ (H @ X[:, :12])
        Gn, Hn = f(0.5) * (Gn + Gn.T), f(0.5) * (Hn + Hn.T)
        conv = np.abs(Hn - H).max() < f(tol) * np.abs(Hn).max()
        Ak, G, H = An, Gn, Hn
        if conv:
            break
    K = np.linalg.solve(np.diag(r) + B0.T @ H @ B0, B0.T @ H @ A0)
    return H.astype(np.float64), K.astype(np.float64)


def gain(A, B, P, r):
    return np.linalg.solve(np.diag(r) + B.T @ P @ B, B.T @ P @ A)


def residual(A, B, P, K, q):
    """max |Q + A'PA - A'PB K - P| / max |P|"""
    return np.abs(np.diag(q) + A.T @ P @ A - A.T @ P @ B @ K - P).max() / np.abs(P).max()


def solve(A, B, q=Q8, r=R1, iters=ITERS, tol=TOL):
    """every instance of A (12, 12, n), B (12, 7, n) -> P (12, 12, n), K (7, 12, n), residual, status, iterations (n,)"""
    n = A.shape[2]
    P, K = np.zeros((12, 12, n)), np.zeros((7, 12, n))
    res, st, it = np.zeros(n), np.zeros(n, int), np.zeros(n, int)
    for i in range(n):
        P[:, :, i], K[:, :, i], res[i], st[i], it[i] = sda(A[:, :, i], B[:, :, i], q, r, iters, tol)
    return P, K, res, st, it


def expand(Xnom, K):
    """K_x,k = -K E(x_k): Xnom (H+1, 13, n), K (7, 12, n) -> (H, 7, 13, n)"""
    return np.stack([-mm(K, E_of(Xnom[k])) for k in range(Xnom.shape[0] - 1)])


def closed_loop(orc, x0, xb, ub, Kx, dt=DT, u_min=None, u_max=None, Xnom=None):
    """u_k = clip(ub + Kx_k (x_k - Xnom_k)) through the oracle; Xnom: given, or the oracle's rollout of (xb, ub).
    -> X (H+1, 13, n), U (H, 7, n), Xnom"""
    H = Kx.shape[0]
    if Xnom is None:
        Xnom = orc.rollout(xb, np.repeat(ub[None], H, axis=0), dt)
    X, U = [np.array(x0, dtype=np.float64)], []
    for k in range(H):
        u = ub + mv(Kx[k], X[-1] - Xnom[k])
        if u_min is not None:
            u = np.clip(u, np.asarray(u_min)[:, None], np.asarray(u_max)[:, None])
        U.append(u)
        X.append(orc.state_update(X[-1], u, dt))
    return np.stack(X), np.stack(U), Xnom


XI0_SIZE = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02])  # m, m/s, rad, rad/s
H_LOOP = 200


def closed_loop_start(n, seed=11):
    """xi_0 (12, n) of the closed-loop tests: XI0_SIZE per coordinate with random signs, along-track 0 (selection 11)"""
    xi = XI0_SIZE[:, None] * np.random.default_rng(seed).choice([-1.0, 1.0], (12, n))
    xi[0] = 0.0
    return xi


def cost_to_go(x, xb, P):
    xi = chart(x, xb)
    return np.einsum("in,ijn,jn->n", xi, P, xi)


# ---- measures ----------------------------------------------------------------------------------------------------------------
def rho(A, B, K, q):
    """spectral radius of the reduced closed loop A - B K per instance"""
    out = np.zeros(A.shape[2])
    for i in range(A.shape[2]):
        a, b = reduce(A[:, :, i], B[:, :, i], q)
        with np.errstate(all="ignore"):
            out[i] = np.abs(np.linalg.eigvals(a - b @ K[:, :, i])).max() if np.isfinite(K[:, :, i]).all() else np.inf
    return out


def loop_cost(A, B, K, q, r):
    """trace of P_K = Q + K'RK + (A - BK)' P_K (A - BK) (the cost of flying the gain K from a unit-covariance start)"""
    a, b = reduce(A, B, q)
    F = a - b @ K
    M = np.diag(q) + K.T @ np.diag(r) @ K
    n = 12
    vec = np.linalg.solve(np.eye(n * n) - np.kron(F.T, F.T), M.reshape(-1))
    return float(np.trace(vec.reshape(n, n)))


def excess_cost(A, B, K, P, q, r):
    """trace(P_K) / trace(P*) - 1 per instance (P*: the float64 solution)"""
    return np.array([loop_cost(A[:, :, i], B[:, :, i], K[:, :, i], q, r) / np.trace(P[:, :, i]) - 1 for i in range(A.shape[2])])


def unit_max_rel(a, ref):
    from tests.helpers import unit_max_rel as f

    return f(a, ref)


def unit_max_abs(a, ref):
    n = ref.shape[-1]
    return np.abs(np.asarray(a, dtype=np.float64) - ref).reshape(-1, n).max(axis=0)


# ---- the grid ----------------------------------------------------------------------------------------------------------------
_GRID = {}


def grid(name, seed=0):
    """The instances of trim_ref.grid(seed) that trim in float64 for the model `name` (a key of tests.test_gpu_trim.MODELS):
    -> (ac, orc, x (13, m), u (7, m)) with x, u float32-exact.  The linear model trims its turns with the rudder held; the
    synthetic wide net is linearised about the cubic fits' trims."""
    if (name, seed) in _GRID:
        return _GRID[(name, seed)]
    from tests.helpers import make_aircraft, make_oracle

    models = {"default": dict(model="default"), "linear": dict(model="linear"), "poly": dict(model="poly"),
              "real_net": dict(model="nn"), "net_4x128": dict(model="nn", hidden=(128, 128, 128, 128))}
    ac = make_aircraft(**models[name])
    orc = make_oracle(ac)
    if name == "net_4x128":  # a random function, not an airframe: it has no steady flight; design about the cubic fits' trims
        out = (ac, orc) + grid("poly", seed)[2:]
        _GRID[(name, seed)] = out
        return out
    cases = T.grid(seed=seed)
    xs, us = [], []
    for lateral in (0, 1):
        sel = [c for c in cases if (name == "linear" and c[1] != 0.0) == (lateral == 1)]
        if not sel:
            continue
        V, psid, beta, fl, psi = (np.array(v) for v in zip(*sel))
        n = len(sel)
        tg = f32x(np.stack([np.zeros(n), np.zeros(n), np.full(n, -200.0), V, psi, psid, np.zeros(n) if lateral else beta]))
        uh = np.zeros((7, n))
        uh[6] = fl
        uh = f32x(uh)
        lo, hi = ac.trim_bounds(lateral)
        z0 = f32x(T.default_guess(tg[3], tg[5], ac.opts.aircraft_config.glide_ratio))
        z, _, ok = T.lm(orc, z0, tg, uh, lateral, lo, hi, iters=200)
        x, u = T.assemble(z[:, ok], tg[:, ok], uh[:, ok], lateral)
        xs.append(x)
        us.append(u)
    out = (ac, orc, f32x(np.concatenate(xs, axis=1)), f32x(np.concatenate(us, axis=1)))
    _GRID[(name, seed)] = out
    return out


def cycle(a, n):
    """n columns of a (.., m), cycling"""
    return a[..., np.arange(n) % a.shape[-1]]


# ---- the host build's entry points (tests/host_lqr/lqr_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) ---------------------
def _host(header=None):
    from tests.test_host_lqr import lib_host

    return lib_host(header)


def _fp(a):
    import ctypes as C

    return a.ctypes.data_as(C.POINTER(C.c_float))


def lqr_opts(q=Q8, r=R1, tol=TOL):
    from aircraft_amd import _lib

    o = _lib.LqrOpts()
    o.q[:] = [float(v) for v in q]
    o.r[:] = [float(v) for v in r]
    o.tol = float(tol)
    return o


def host_project(xb, xbp, A, B, header=None):
    n = xb.shape[1]
    a = [c32(v) for v in (xb, xbp, np.reshape(A, (169, n)), np.reshape(B, (91, n)))]
    Ax, Bx = np.zeros((144, n), np.float32), np.zeros((84, n), np.float32)
    assert _host(header).host_lqr_project(*[_fp(v) for v in a], n, _fp(Ax), _fp(Bx)) == 0
    return Ax.reshape(12, 12, n).astype(np.float64), Bx.reshape(12, 7, n).astype(np.float64)


def host_dare(A, B, q=Q8, r=R1, iters=ITERS, tol=TOL, header=None):
    """-> P, K, residual, status, iterations of the float32 host build on float32-rounded A_xi, B_xi"""
    import ctypes as C

    n = A.shape[2]
    a = [c32(np.reshape(A, (144, n))), c32(np.reshape(B, (84, n)))]
    P, K = np.zeros((144, n), np.float32), np.zeros((84, n), np.float32)
    res, st, it = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    IP = C.POINTER(C.c_int)
    o = lqr_opts(q, r, tol)
    assert _host(header).host_lqr_dare(C.byref(o), *[_fp(v) for v in a], int(iters), n, _fp(P), _fp(K), _fp(res),
                                       st.ctypes.data_as(IP), it.ctypes.data_as(IP)) == 0
    return P.reshape(12, 12, n).astype(np.float64), K.reshape(7, 12, n).astype(np.float64), res.astype(np.float64), st, it


def host_gains(Xnom, K, header=None):
    Hn, n = Xnom.shape[0] - 1, Xnom.shape[2]
    a = [c32(Xnom), c32(np.reshape(K, (84, n)))]
    Kx = np.zeros((Hn, 7, 13, n), np.float32)
    assert _host(header).host_lqr_gains(*[_fp(v) for v in a], n, Hn, _fp(Kx)) == 0
    return Kx.astype(np.float64)


def host_error(x, xb, header=None):
    n = x.shape[1]
    a = [c32(x), c32(xb)]
    xi = np.zeros((12, n), np.float32)
    assert _host(header).host_steady_error(*[_fp(v) for v in a], n, _fp(xi)) == 0
    return xi.astype(np.float64)


def host_gj(W, rhs, header=None):
    """the group elimination alone: W (12, 12), rhs (12, 24) -> X (12, 24), breakdown flag"""
    import ctypes as C

    w, b = c32(W), c32(rhs)
    X = np.zeros((12, 24), np.float32)
    bad = C.c_int(0)
    assert _host(header).host_lqr_gj(_fp(w), _fp(b), _fp(X), C.byref(bad)) == 0
    return X.astype(np.float64), bad.value
