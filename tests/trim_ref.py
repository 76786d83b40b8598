"""Float64 restatement of the trim problem (aircraft_amd/csrc/ac_trim.hpp; include/aircraft_hip.h, ac_trim_f32) for the tests:
the map z -> (x, u), the residual r from the oracle's state_derivative, its exact Jacobian (the oracle's df/dx, df/du
chained with dx/dz, plus the rotation terms) and the same Levenberg-Marquardt iteration in float64.

For the step-by-step tests (second half): `chain` (r, J_z from GIVEN f, df/dx, df/du), `step`, `final_status`, `transition`,
the workspace and state-word layout, the error measures, the host build's entry points, the cases with their e32 (the g++
build against float64 on identical inputs) and the per-call checks that the host build (tests/test_trim_steps_ref.py) and the
device (tests/test_gpu_trim_steps.py) both go through.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import numpy as np

from aircraft_amd.synthetic import quat_from_euler

DEG = np.pi / 180.0
LAM0, LAM_MIN, LAM_MAX = 1e-3, 1e-8, 1e8


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.stack([aw * bx + bw * ax + ay * bz - az * by, aw * by + bw * ay + az * bx - ax * bz,
                     aw * bz + bw * az + ax * by - ay * bx, aw * bw - (ax * bx + ay * by + az * bz)])


def qconj(q):
    return np.stack([-q[0], -q[1], -q[2], q[3]])


def rot(q, v):
    """q (v, 0) q^-1 (unit q), v (3, n)"""
    return qmul(qmul(q, np.concatenate([v, np.zeros((1, v.shape[1]))])), qconj(q))[:3]


def kinematics(z, target, lateral):
    """z (6, n), target (7, n) -> q (4, n), v_b, v_ned, omega_b (3, n)"""
    al, th, ph = z[0], z[1], z[2]
    be = z[5] if lateral else target[6]
    V, psi, psid = target[3], target[4], target[5]
    q = quat_from_euler(ph, th, psi)
    vb = V * np.stack([np.cos(al) * np.cos(be), np.sin(be), np.sin(al) * np.cos(be)])
    vn = rot(q, vb)
    wb = rot(qconj(q), np.stack([0 * V, 0 * V, psid]))
    return q, vb, vn, wb


def assemble(z, target, uhold, lateral):
    """z -> x (13, n), u (7, n)"""
    q, vb, vn, wb = kinematics(z, target, lateral)
    x = np.concatenate([target[0:3], vn, q, wb])
    u = np.array(uhold, dtype=np.float64, copy=True)
    u[0], u[1] = z[3], z[4]
    u[2] = target[6] if lateral else z[5]
    return x, u


def transform(z, target, lateral, fv, fw):
    """r = (q^-1 f_v q - w_b x v_b, f_w)"""
    q, vb, vn, wb = kinematics(z, target, lateral)
    rv = rot(qconj(q), fv) - np.cross(wb, vb, axis=0)
    return np.concatenate([rv, fw])


def residual(orc, z, target, uhold, lateral):
    x, u = assemble(z, target, uhold, lateral)
    f = orc.state_derivative(x, u)
    return transform(z, target, lateral, f[3:6], f[10:13])


def residual_at(orc, x, u, z, target, lateral):
    """r from the oracle at a given (x, u) (the GPU's returned fp32 state), with the frame of z"""
    f = orc.state_derivative(x, u)
    return transform(z, target, lateral, f[3:6], f[10:13])


def chain(z, target, lateral, xd, Fx, Fu, h=1e-6):
    """(r (6, n), J (6, 6, n)) from GIVEN f = xd (13, n), df/dx = Fx (13, 13, n), df/du = Fu (13, 7, n) at the assembled
    (x(z), u(z)): trim_residual_jacobian in float64.  df/dx, df/du are chained with dx/dz, du/dz, plus the explicit
    z-dependence of the transform.  The two elementary smooth maps (z -> x and the transform at fixed f) are differentiated
    by central differences (error ~h^2, far below the test bars).  The held control rows do not depend on z."""
    n = z.shape[1]
    f = xd
    uhold = np.zeros((7, n))
    q = kinematics(z, target, lateral)[0]
    r = transform(z, target, lateral, f[3:6], f[10:13])
    J = np.zeros((6, 6, n))
    for j in range(6):
        e = np.zeros((6, 1))
        e[j] = h
        xp, up = assemble(z + e, target, uhold, lateral)
        xm, um = assemble(z - e, target, uhold, lateral)
        dx, du = (xp - xm) / (2 * h), (up - um) / (2 * h)
        df = np.einsum("icn,cn->in", Fx, dx) + np.einsum("icn,cn->in", Fu, du)
        rp = transform(z + e, target, lateral, f[3:6], f[10:13])
        rm = transform(z - e, target, lateral, f[3:6], f[10:13])
        dT = (rp - rm) / (2 * h)
        # r is linear in f: its f-part is the rotation of df_v into the body frame, and df_w
        lin = np.concatenate([rot(qconj(q), df[3:6]), df[10:13]])
        J[:, j] = dT + lin
    return r, J


def jacobian(orc, z, target, uhold, lateral, h=1e-6):
    """(r (6, n), J (6, 6, n)): `chain` fed with the oracle's exact f, df/dx, df/du at the assembled (x, u)."""
    x, u = assemble(z, target, uhold, lateral)
    f, Fx, Fu = orc.state_derivative_sens(x, u)
    return chain(z, target, lateral, f, Fx, Fu, h)


def row_weights(tol):
    """(6, 1): the residual rows are scaled by 1 / tol_v (r_v) and 1 / tol_w (r_w)"""
    return np.array([1 / tol[0]] * 3 + [1 / tol[1]] * 3)[:, None]


def gradient(r, J, tol):
    """g = J' W^2 r (6, n), and sum_i |J_ij w_i^2 r_i| (6, n): the size of the terms that add up to g_j"""
    w2 = row_weights(tol) ** 2
    t = J * (w2 * r)[:, None, :]
    return t.sum(0), np.abs(t).sum(0)


def step(z, r, J, lam, lo, hi, tol=(1e-4, 1e-4), raw=False):
    """trim_step in float64, per instance: (H + lam diag H + mu I) dz = -g with H = J' W^2 J, g = J' W^2 r,
    mu = 1e-7 max diag H + 1e-30, then z + dz clipped to [lo, hi]; a non-finite step leaves z where it is.
    z, r (6, n), J (6, 6, n), lam (n,) -> z_next (6, n) (raw: and the unclipped z + dz)."""
    lo, hi = np.asarray(lo, dtype=np.float64).ravel(), np.asarray(hi, dtype=np.float64).ravel()
    w = row_weights(tol)
    n = z.shape[1]
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,))
    zn, free = np.array(z, dtype=np.float64, copy=True), np.array(z, dtype=np.float64, copy=True)
    for i in range(n):
        Jw = w * J[:, :, i]
        H = Jw.T @ Jw
        g = Jw.T @ (w[:, 0] * r[:, i])
        M = H + lam[i] * np.diag(np.diag(H)) + (1e-7 * np.diag(H).max() + 1e-30) * np.eye(6)
        try:
            with np.errstate(all="ignore"):
                t = z[:, i] + np.linalg.solve(M, -g)
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(t).all():
            free[:, i] = t
            zn[:, i] = np.clip(t, lo, hi)
    return (zn, free) if raw else zn


def converged(r, tol):
    """trim_converged (false for NaN): (n,)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(r[:3]) <= tol[0]).all(0) & (np.abs(r[3:]) <= tol[1]).all(0)


def lm_states(orc, z0, target, uhold, lateral, lo, hi, tol=(1e-4, 1e-4), iters=200):
    """The kernel's iteration in float64, one state per evaluation: yields after evaluation k = 1, 2, ... a dict of copies
    zc (the NEXT candidate), zb, rb, Jb, lam, cost, active, conv, and what the evaluation did per instance:
    kind (n,) in {"accept", "reject", "frozen"} (frozen: the instance was no longer active when it started)."""
    lo, hi = np.asarray(lo)[:, None], np.asarray(hi)[:, None]
    w = row_weights(tol)
    n = z0.shape[1]
    zc = np.clip(z0, lo, hi)
    zb, rb, Jb = zc.copy(), np.full((6, n), np.nan), np.zeros((6, 6, n))
    cost_b = np.full(n, np.inf)
    lam = np.full(n, LAM0)
    active = np.ones(n, bool)
    conv = np.zeros(n, bool)
    for k in range(iters):
        idx = np.where(active)[0]
        if not len(idx):
            break
        r, J = jacobian(orc, zc[:, idx], target[:, idx], uhold[:, idx], lateral)
        cost = ((w * r) ** 2).sum(0)
        better = cost < cost_b[idx]
        a, b = idx[better], idx[~better]
        kind = np.full(n, "frozen", dtype=object)
        kind[a], kind[b] = "accept", "reject"
        zb[:, a], rb[:, a], Jb[:, :, a], cost_b[a] = zc[:, a], r[:, better], J[:, :, better], cost[better]
        lam[a] = np.maximum(lam[a] / 3, LAM_MIN)
        lam[b] = np.minimum(lam[b] * 4, LAM_MAX)
        ok = converged(rb, tol)
        conv |= ok & active
        active &= ~ok & np.isfinite(cost_b)
        act = np.where(active)[0]
        zc[:, act] = step(zb[:, act], rb[:, act], Jb[:, :, act], lam[act], lo, hi, tol)
        yield dict(k=k + 1, zc=zc.copy(), zb=zb.copy(), rb=rb.copy(), Jb=Jb.copy(), lam=lam.copy(), cost=cost_b.copy(),
                   active=active.copy(), conv=conv.copy(), kind=kind)


def lm(orc, z0, target, uhold, lateral, lo, hi, tol=(1e-4, 1e-4), iters=200):
    """The kernel's iteration in float64 -> (z, r, converged mask)."""
    lo_, hi_ = np.asarray(lo)[:, None], np.asarray(hi)[:, None]
    n = z0.shape[1]
    s = dict(zb=np.clip(z0, lo_, hi_), rb=np.full((6, n), np.nan), conv=np.zeros(n, bool))
    for s in lm_states(orc, z0, target, uhold, lateral, lo, hi, tol, iters):
        pass
    return s["zb"], s["rb"], s["conv"]


def default_guess(V, psid, glide_ratio, g=9.81):
    V, psid = np.broadcast_arrays(np.asarray(V, float), np.asarray(psid, float))
    z = np.zeros((6, V.size))
    z[0] = 4 * DEG
    z[1] = 4 * DEG - np.arctan(1.0 / glide_ratio)
    z[2] = np.arctan(V.ravel() * psid.ravel() / g)
    return z


def grid(seed=0, flaps=(0.0, 0.5)):
    """The test grid: V in {25, 35, 50, 70}, turn rate in {0, +-0.15}, beta in {0, 2 deg}, flaps, random psi
    -> list of (V, psid, beta, flaps, psi)."""
    rng = np.random.default_rng(seed)
    out = []
    for V in (25.0, 35.0, 50.0, 70.0):
        for psid in (0.0, 0.15, -0.15):
            for beta in (0.0, 2 * DEG):
                for fl in flaps:
                    out.append((V, psid, beta, fl, rng.uniform(-np.pi, np.pi)))
    return out


# ---- the LM iteration step by step (tests/test_trim_steps_ref.py, tests/test_gpu_trim_steps.py) -------------------------------
# The layout of ac_trim_f32's workspace and of the LM state column, restated from aircraft_amd/csrc/ac_trim.hpp and
# ac_trim_f32 (tests/test_trim_steps_ref.py reads the header and fails if they part).
WS_ROWS = (("X", 13), ("U", 7), ("Xd", 13), ("Fx", 169), ("Fu", 91), ("St", 57))   # rows of n floats, in this order
WS_FLOATS = 350          # kTrimWsFloats
WS_PAD = 6 * 64          # kTrimWsPad: each of the six arrays starts on a 256-byte boundary
WORDS = dict(zc=0, zb=6, rb=12, Jb=18, lam=54, cost=55, flag=56)   # kTzc ... kTflag
STATE_WORDS = 57
ACTIVE = -1.0            # kTrimActive
BLOCK = 256              # kTrimBlock
SIZES = (1, 63, 64, 65, 257)
POINTS = (0, 1, 3, 6)    # starting points: the float64 LM's best iterate after this many steps (k + 1 evaluations)
K = 6                    # evaluations of the chain
TOL32 = float(np.float32(1e-4))
F32 = np.float32
LAM_ACCEPT = F32(1.0) / F32(3.0)


def f32x(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def ws_layout(addr, n):
    """Float offsets from `ws` (a byte address) of the six arrays, and of the end of the last one: the first starts at the
    first 256-byte boundary at or after ws, each next one at the first boundary at or after the end of the one before."""
    off, p = {}, int(addr)
    for name, rows in WS_ROWS:
        p = (p + 255) & ~255
        assert (p - addr) % 4 == 0
        off[name] = (p - addr) // 4
        p += 4 * rows * n
    return off, (p - addr) // 4


def unpack(st):
    """(57, n) LM state -> dict zc, zb, rb (6, n), Jb (6, 6, n), lam, cost, flag (n,), dtype kept"""
    W = WORDS
    return dict(zc=st[W["zc"]:W["zc"] + 6], zb=st[W["zb"]:W["zb"] + 6], rb=st[W["rb"]:W["rb"] + 6],
                Jb=st[W["Jb"]:W["Jb"] + 36].reshape(6, 6, -1), lam=st[W["lam"]], cost=st[W["cost"]], flag=st[W["flag"]])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def z_err(z, ref, lo, hi):
    """per instance: max_j |z_j - ref_j| / (hi_j - lo_j)"""
    return (np.abs(z - ref) / (np.asarray(hi) - np.asarray(lo))[:, None]).max(0)


def r_scale(z, target, lateral, xd):
    """s_i = max(max_rows(|q^-1 f_v q| + |w_b x v_b|), max |f_w|): the size of the terms that cancel in r"""
    q, vb, vn, wb = kinematics(z, target, lateral)
    a = np.abs(rot(qconj(q), xd[3:6])) + np.abs(np.cross(wb, vb, axis=0))
    return np.maximum(a.max(0), np.abs(xd[10:13]).max(0))


def r_err(r, ref, s):
    return (np.abs(r - ref) / s).max(0)


def final_status(z, r, J, lo, hi, tol):
    """trim_final_status -> (status (n,): 2 when some z_j sits on a bound and -g points out of the box there, else 1;
    decisiveness (n,): min over the on-bound components of |g_j| / sum_i |J_ij w_i^2 r_i|, inf without one)."""
    lo, hi = np.asarray(lo)[:, None], np.asarray(hi)[:, None]
    g, size = gradient(r, J, tol)
    stuck = ((z >= hi) & (g < 0)) | ((z <= lo) & (g > 0))
    on = (z >= hi) | (z <= lo)
    with np.errstate(all="ignore"):
        dec = np.where(on, np.abs(g) / size, np.inf).min(0)
    return np.where(stuck.any(0), 2, 1), dec


def transition(prev, cost_c):
    """The accept / reject rule of trim_update_unit in the device's arithmetic.  prev: the unpacked fp32 state before the
    evaluation, cost_c (n,): the candidate's cost -> kind (n,) in {"accept", "reject", "frozen"}, lambda after it (fp32,
    bit for bit), nonfinite (n,): a reject without one finite evaluation behind it (status 3)."""
    cost_b, lam = np.asarray(prev["cost"]), np.asarray(prev["lam"], dtype=np.float32)
    active = np.asarray(prev["flag"]) == ACTIVE
    with np.errstate(invalid="ignore"):
        accept = active & (np.asarray(cost_c) < cost_b)
        reject = active & ~accept
        nonfinite = reject & ~(cost_b <= 3.0e38)
    kind = np.where(accept, "accept", np.where(reject, "reject", "frozen"))
    with np.errstate(over="ignore"):
        lam_n = np.where(accept, np.maximum(lam * LAM_ACCEPT, F32(LAM_MIN)), np.where(reject, np.minimum(lam * F32(4.0), F32(LAM_MAX)), lam))
    return kind, lam_n.astype(np.float32), nonfinite


def cost_of(r, tol):
    return ((row_weights(tol) * r) ** 2).sum(0)


# ---- the host build's entry points (tests/host_trim/trim_host.cpp: g++, -ffp-contract=off) -----------------------------------
def _host():
    from tests.test_host_trim import _lib_host

    return _lib_host()


def _fp(a):
    import ctypes as C

    return a.ctypes.data_as(C.POINTER(C.c_float))


def trim_opts(lateral, lo, hi, tol):
    from aircraft_amd import _lib

    o = _lib.TrimOpts()
    o.lateral = int(lateral)
    o.tol_v, o.tol_w = tol
    o.lo[:] = [float(v) for v in lo]
    o.hi[:] = [float(v) for v in hi]
    return o


def c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host_chain(z, target, lateral, xd, Fx, Fu):
    """fp32 trim_residual_jacobian on given sensitivities -> r (6, n), J (6, 6, n) as float64"""
    n = z.shape[1]
    a = [c32(v) for v in (target, z, xd, Fx, Fu)]
    R, J = np.zeros((6, n), np.float32), np.zeros((36, n), np.float32)
    assert _host().host_trim_chain(int(lateral), *[_fp(v) for v in a], n, _fp(R), _fp(J)) == 0
    return R.astype(np.float64), J.reshape(6, 6, n).astype(np.float64)


def host_step(z, r, J, lam, lateral, lo, hi, tol):
    import ctypes as C

    n = z.shape[1]
    a = [c32(v) for v in (z, r, np.reshape(J, (36, n)), np.broadcast_to(lam, (n,)))]
    Zn = np.zeros((6, n), np.float32)
    o = trim_opts(lateral, lo, hi, tol)
    assert _host().host_trim_step(C.byref(o), *[_fp(v) for v in a], n, _fp(Zn)) == 0
    return Zn.astype(np.float64)


def host_final_status(z, r, J, lateral, lo, hi, tol):
    import ctypes as C

    n = z.shape[1]
    a = [c32(v) for v in (z, r, np.reshape(J, (36, n)))]
    S = np.zeros(n, np.int32)
    o = trim_opts(lateral, lo, hi, tol)
    assert _host().host_trim_final_status(C.byref(o), *[_fp(v) for v in a], n, S.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return S


def host_trace(ac, target, uhold, z0, lateral, iters, lo, hi, tol):
    """The host build's whole solve (analytic models) and what the device's workspace would hold after it -> snapshot"""
    import ctypes as C

    from tests.test_host_trim import _model_args

    n = target.shape[1]
    keep, ptr = _model_args(ac)
    o = trim_opts(lateral, lo, hi, tol)
    t, u, z = c32(target), c32(uhold), c32(z0)
    out = dict(Xo=(13, n), Uo=(7, n), Z=(6, n), R=(6, n))
    ws = dict(X=(13, n), U=(7, n), Xd=(13, n), Fx=(169, n), Fu=(91, n), st=(STATE_WORDS, n))
    s = {k: np.full(v, np.nan, np.float32) for k, v in {**out, **ws}.items()}
    s["S"] = np.full(n, -1, np.int32)
    rc = _host().host_trim_trace(C.byref(ac._param_struct()), *ptr, C.byref(o), _fp(t), _fp(u), _fp(z), int(iters), n,
                                 *[_fp(s[k]) for k in out], s["S"].ctypes.data_as(C.POINTER(C.c_int)), *[_fp(s[k]) for k in ws])
    assert rc == 0
    s["Fx"], s["Fu"] = s["Fx"].reshape(13, 13, n), s["Fu"].reshape(13, 7, n)
    return s


# ---- the cases and their e32 ---------------------------------------------------------------------------------------------------
class Case:
    """One (model, lateral mode): the 48 instances of grid(seed=0), the float64 LM's trajectory from the default guess
    (8 evaluations) and the starting points taken from it, all inputs fp32-exact."""

    def __init__(self, name, lateral):
        from tests.helpers import make_aircraft, make_oracle
        from tests.test_gpu_trim import MODELS

        self.name, self.lateral = name, lateral
        self.ac = make_aircraft(**MODELS[name])
        self.orc = make_oracle(self.ac)
        V, psid, beta, fl, psi = (np.array(v) for v in zip(*grid(seed=0)))
        n = len(V)
        tg = np.stack([np.zeros(n), np.zeros(n), np.full(n, -200.0), V, psi, psid, np.zeros(n) if lateral else beta])
        uh = np.zeros((7, n))
        uh[6] = fl
        self.tg, self.uh = f32x(tg), f32x(uh)
        self.lo, self.hi = (f32x(b) for b in self.ac.trim_bounds(lateral))
        self.tol = (TOL32, TOL32)
        self.z0 = f32x(default_guess(self.tg[3], self.tg[5], self.ac.opts.aircraft_config.glide_ratio))
        self.traj = list(lm_states(self.orc, self.z0, self.tg, self.uh, lateral, self.lo, self.hi, self.tol, iters=8))
        assert len(self.traj) > max(K, *POINTS), "some instance is is still active"
        self.points = {0: self.z0, **{k: f32x(self.traj[k]["zb"]) for k in POINTS if k}}

    def pool(self, points=POINTS):
        """every instance at every starting point: target, uhold, z0 (.., 48 len(points)) and the point of each column"""
        m = len(points)
        return (np.tile(self.tg, (1, m)), np.tile(self.uh, (1, m)), np.concatenate([self.points[k] for k in points], axis=1),
                np.repeat(points, self.tg.shape[1]))

    def sens(self, z, tg, uh):
        """the oracle's f, df/dx, df/du at the assembled (x(z), u(z)), rounded to fp32"""
        x, u = assemble(z, tg, uh, self.lateral)
        return tuple(f32x(a) for a in self.orc.state_derivative_sens(x, u))

    # e32: the host build against float64 on identical (fp32-exact) inputs, in the measures of the tests
    def e32_chain(self):
        """-> (e32 of r, e32 of J), worst instance over every starting point"""
        if not hasattr(self, "_e32_chain"):
            tg, uh, z, _ = self.pool()
            xd, Fx, Fu = self.sens(z, tg, uh)
            r64, J64 = chain(z, tg, self.lateral, xd, Fx, Fu)
            r32, J32 = host_chain(z, tg, self.lateral, xd, Fx, Fu)
            from tests.helpers import unit_max_rel

            self._e32_chain = (float(r_err(r32, r64, r_scale(z, tg, self.lateral, xd)).max()), float(unit_max_rel(J32, J64).max()))
        return self._e32_chain

    def _e32_step(self, z, r, J, lam):
        z, r, J, lam = f32x(z), f32x(r), f32x(J), f32x(lam)
        want = step(z, r, J, lam, self.lo, self.hi, self.tol)
        got = host_step(z, r, J, lam, self.lateral, self.lo, self.hi, self.tol)
        return z_err(got, want, self.lo, self.hi)

    def e32_step_point(self, k):
        """the step after the first evaluation at starting point k (the oracle's r, J there, lambda = 1e-3f / 3)"""
        if not hasattr(self, "_e32_pt"):
            self._e32_pt = {}
        if k not in self._e32_pt:
            r, J = jacobian(self.orc, self.points[k], self.tg, self.uh, self.lateral)
            self._e32_pt[k] = float(self._e32_step(self.points[k], r, J, F32(LAM0) * LAM_ACCEPT).max())
        return self._e32_pt[k]

    def e32_step_chain(self):
        """every step of the float64 trajectory's first K - 1 evaluations (active instances, their lambda)"""
        if not hasattr(self, "_e32_ch"):
            worst = 0.0
            for s in self.traj[:K - 1]:
                a = s["active"]
                if a.any():
                    worst = max(worst, float(self._e32_step(s["zb"][:, a], s["rb"][:, a], s["Jb"][:, :, a], s["lam"][a]).max()))
            self._e32_ch = worst
        return self._e32_ch


_CASES = {}


def case(name, lateral):
    if (name, lateral) not in _CASES:
        _CASES[(name, lateral)] = Case(name, lateral)
    return _CASES[(name, lateral)]


def columns(pool, n, offset=0):
    """n columns of a pool, cycling from `offset`"""
    return (offset + np.arange(n)) % pool


# ---- the checks, shared by the host build (CPU) and the device ------------------------------------------------------------------
# A snapshot is what one call left behind, as float32 arrays: the workspace X (13, n), U (7, n), Xd (13, n), Fx (13, 13, n),
# Fu (13, 7, n), st (57, n), and the outputs Xo, Uo, Z, R, S.
def check_evaluation(snap, tg, uh, z0, lateral, lo, hi, tol, bar_r, bar_J):
    """After iters = 1 from z0 (inside the bounds): every instance's assembly, stored r_b, J_b against `chain` fed with the
    snapshot's own sensitivities, cost, lambda, outputs and status.  -> dict of the worst figures."""
    from tests.helpers import unit_max_rel

    n = tg.shape[1]
    st = unpack(snap["st"])
    assert same_bits(st["zc"], c32(z0)) and same_bits(st["zb"], c32(z0)), "z_c, z_b are the starting point"
    x, u = assemble(z0, tg, uh, lateral)
    X, U = snap["X"].astype(np.float64), snap["U"]
    fig = dict(p=np.abs(X[0:3] - x[0:3]).max(), v=np.abs(X[3:6] - x[3:6]).max(), q=np.abs(X[6:10] - x[6:10]).max(),
               w=np.abs(X[10:13] - x[10:13]).max())
    assert fig["p"] <= 1e-7 * np.abs(x[0:3]).max() and fig["v"] < 1e-5 * 70 and fig["q"] < 1e-6 and fig["w"] < 1e-7, fig
    assert np.array_equal(U, c32(u)), "U is copied, not computed"
    xd, Fx, Fu = (snap[k].astype(np.float64) for k in ("Xd", "Fx", "Fu"))
    assert np.isfinite(xd).all() and np.isfinite(Fx).all() and np.isfinite(Fu).all()
    r64, J64 = chain(z0, tg, lateral, xd, Fx, Fu)
    rb, Jb = st["rb"].astype(np.float64), st["Jb"].astype(np.float64)
    er, eJ = r_err(rb, r64, r_scale(z0, tg, lateral, xd)), unit_max_rel(Jb, J64)
    fig.update(r=float(er.max()), J=float(eJ.max()), bar_r=bar_r, bar_J=bar_J)
    assert (er <= bar_r).all(), ("r_b", fig, np.where(er > bar_r)[0])
    assert (eJ <= bar_J).all(), ("J_b", fig, np.where(eJ > bar_J)[0])
    c64 = cost_of(rb, tol)
    ulp = np.abs(st["cost"].astype(np.float64) - c64) / np.spacing(c64.astype(np.float32)).astype(np.float64)
    fig["cost_ulp"] = float(ulp.max())
    assert (ulp <= 4).all(), ("cost", fig)
    assert same_bits(st["lam"], np.full(n, F32(LAM0) * LAM_ACCEPT, np.float32)), "lambda after the first accept"
    assert same_bits(snap["Z"], st["zb"]) and same_bits(snap["R"], st["rb"]), "Z, R are the stored best"
    assert same_bits(snap["Xo"], snap["X"]) and same_bits(snap["Uo"], snap["U"]), "X, U are the assembly of the stored best"
    conv = converged(st["rb"], tuple(F32(t) for t in tol))
    fs, dec = final_status(st["zb"].astype(np.float64), rb, Jb, lo, hi, tol)
    assert np.array_equal(st["flag"], np.where(conv, F32(0), F32(ACTIVE))), "frozen exactly where r_b meets the tolerances"
    want = np.where(conv, 0, fs)
    assert np.array_equal(snap["S"], want), ("status", snap["S"], want)
    fig.update(converged=int(conv.sum()), status1=int((want == 1).sum()), status2=int((want == 2).sum()),
               decisive=float(dec[~conv].min(initial=np.inf)))
    return fig


def check_step(prev, new, lo, hi, tol, bar):
    """z_c of the iters = k + 1 call against `step` fed with the stored z_b, r_b, J_b, lambda of the iters = k call: every
    active instance within `bar` ((n,) or a scalar) in the z measure, clipped components on the bound bit for bit; the z_c
    of a frozen instance unchanged.  -> (worst error, clipped components)"""
    a, b = unpack(prev["st"]), unpack(new["st"])
    act = a["flag"] == ACTIVE
    want, free = step(*(a[k].astype(np.float64) for k in ("zb", "rb", "Jb", "lam")), lo, hi, tol, raw=True)
    got = b["zc"].astype(np.float64)
    err = np.where(act, z_err(got, want, lo, hi), 0.0)
    assert (err <= bar).all(), ("step", float(err.max()), np.where(err > bar)[0])
    clip_hi = (free > np.asarray(hi)[:, None]) & act
    clip_lo = (free < np.asarray(lo)[:, None]) & act
    assert same_bits(b["zc"][clip_hi], np.broadcast_to(c32(hi)[:, None], got.shape)[clip_hi]), "clipped to hi"
    assert same_bits(b["zc"][clip_lo], np.broadcast_to(c32(lo)[:, None], got.shape)[clip_lo]), "clipped to lo"
    assert same_bits(b["zc"][:, ~act], a["zc"][:, ~act]), "a frozen instance keeps its z_c"
    return float(err.max(initial=0.0)), int(clip_hi.sum() + clip_lo.sum())


def check_transition(prev, new, tg, lateral, tol, bar_r):
    """The state after k + 1 evaluations from the state after k: accept, reject, freeze (trim_update_unit), every word.
    The kind is read off the stored cost (an accept lowers it strictly) and must be the one `transition` names for the
    candidate's float64 cost from `chain` at the new snapshot's sensitivities, unless that cost is within what an error of
    bar_r in r moves it of the stored best.  -> counts dict(accept, reject, freeze, frozen, undecided)"""
    a, b = unpack(prev["st"]), unpack(new["st"])
    tol32 = tuple(F32(t) for t in tol)
    act = a["flag"] == ACTIVE
    idle = ~act
    assert same_bits(new["st"][:, idle], prev["st"][:, idle]), "a frozen instance keeps every word"
    assert np.array_equal(new["S"][idle], prev["S"][idle]) and same_bits(new["Z"][:, idle], prev["Z"][:, idle]) \
        and same_bits(new["R"][:, idle], prev["R"][:, idle]), "a frozen instance keeps its outputs"
    with np.errstate(invalid="ignore"):
        acc = act & (b["cost"] < a["cost"])
    rej = act & ~acc
    _, lam, nonfinite = transition(a, np.where(acc, b["cost"], a["cost"]))
    assert same_bits(b["lam"], lam), ("lambda", b["lam"][bits(b["lam"]) != bits(lam)], lam[bits(b["lam"]) != bits(lam)])
    assert same_bits(b["zb"][:, acc], b["zc"][:, acc]), "accept: z_b is the candidate (the last evaluation forms no new one)"
    for k in ("zb", "rb", "Jb"):
        assert same_bits(b[k][..., rej], a[k][..., rej]), ("reject restores", k)
    assert same_bits(b["cost"][rej], a["cost"][rej]), "reject keeps the cost"
    # the decision itself, against float64 on the device's own sensitivities
    zc = b["zc"].astype(np.float64)
    xd, Fx, Fu = (new[k].astype(np.float64) for k in ("Xd", "Fx", "Fu"))
    with np.errstate(all="ignore"):
        r64, _ = chain(zc, tg, lateral, xd, Fx, Fu)
        c64 = cost_of(r64, tol)
        d = bar_r * r_scale(zc, tg, lateral, xd)
        margin = ((row_weights(tol) ** 2) * (2 * np.abs(r64) * d + d * d)).sum(0)
        clear = act & (np.abs(c64 - a["cost"].astype(np.float64)) > margin)
        want_acc = c64 < a["cost"].astype(np.float64)
    assert np.array_equal(acc[clear], want_acc[clear]), ("accept / reject against float64", np.where(clear & (acc != want_acc))[0])
    # freeze: exactly where the stored r_b meets the tolerances
    conv = converged(b["rb"], tol32) & act & ~nonfinite
    want_flag = np.where(conv, F32(0), np.where(nonfinite, F32(3), a["flag"]))
    assert np.array_equal(b["flag"], want_flag), ("flag", b["flag"], want_flag)
    assert (new["S"][conv] == 0).all() and (new["S"][nonfinite] == 3).all()
    assert same_bits(new["Z"], b["zb"]) and same_bits(new["R"], b["rb"]), "Z, R are the stored best"
    return dict(accept=int(acc.sum()), reject=int(rej.sum()), freeze=int(conv.sum()), frozen=int(idle.sum()),
                undecided=int((act & ~clear).sum()))


def check_last_status(snap, lo, hi, tol):
    """the status of every still-active instance is `final_status` of the stored state -> (status 1, status 2, decisiveness)"""
    s = unpack(snap["st"])
    act = s["flag"] == ACTIVE
    fs, dec = final_status(*(s[k][..., act].astype(np.float64) for k in ("zb", "rb", "Jb")), lo, hi, tol)
    assert np.array_equal(snap["S"][act], fs), ("status", snap["S"][act], fs)
    assert np.array_equal(snap["S"][~act], s["flag"][~act].astype(np.int32))
    return int((fs == 1).sum()), int((fs == 2).sum()), float(dec.min(initial=np.inf))
