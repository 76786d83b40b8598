"""Float64 restatement of the loop closed through the estimator (aircraft_amd/csrc/ac_lqg.hpp; include/aircraft_hip.h,
ac_sense_f32 .. ac_lqg_rollout_f32) for the tests: the noise definition, the sensor schedule and dropout, the
simulated sensors, the process noise, the control law (in float64, and as the float32 fmaf chain the header writes out), the
score of an estimate against the truth, the closed loop itself, the host build's entry points and the recorded worst float32
errors of the score.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests import ekf_ref as E
from tests.mppi_ref import box_muller, philox4x32_10

GROUPS = 5
MEAS, DROP_A, DROP_B, PROC = 0, 4, 5, 6  # purposes (counter word 3)

# e32 of the score: the host build (g++, -ffp-contract=off) against score() on identical float32-rounded inputs, worst instance
# over ekf_ref.inputs of every model (the truth against the estimate under P0), measured value plus 10 %.
# tests/test_host_lqg.py measures them and fails if they are exceeded; the GPU tests hold the device to 8 x these.
# "e": max |de| / sqrt(P_ii) over the 12 coordinates; "nees": |dnees| / (1 + nees).
E32_WORST = {"e": 1.35e-6, "nees": 3.74e-7}  # measured 1.22e-6 (poly), 3.39e-7 (linear)


@dataclass
class Sensors:
    """ac_sense_opts"""
    seed: int = 0
    instance_offset: int = 0
    period: tuple = (1, 1, 1, 1, 1)
    phase: tuple = (0, 0, 0, 0, 0)
    dropout: tuple = (0.0, 0.0, 0.0, 0.0, 0.0)
    mag: tuple = tuple(E.MAG)


def words(s, n, step, purpose):
    """the four uint32 words of (global instance, step, purpose) for instances 0 .. n-1"""
    g = np.arange(n, dtype=np.uint64) + np.uint64(s.instance_offset)
    return philox4x32_10(g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), int(step) & 0xFFFFFFFF, purpose, int(s.seed) & 0xFFFFFFFF,
                         (int(s.seed) >> 32) & 0xFFFFFFFF)


def normals(s, n, step, first, calls):
    """(normals (4 calls, n), Box-Muller radii (4 calls, n)) of the purposes first .. first + calls - 1"""
    nrm, rad = np.empty((4 * calls, n)), np.empty((4 * calls, n))
    for p in range(calls):
        x = words(s, n, step, first + p)
        for h in (0, 1):
            na, nb, r = box_muller(x[2 * h], x[2 * h + 1])
            nrm[4 * p + 2 * h], nrm[4 * p + 2 * h + 1] = na, nb
            rad[4 * p + 2 * h] = rad[4 * p + 2 * h + 1] = r
    return nrm, rad


def uniforms(s, n, step):
    """(5, n): the dropout uniforms of the five groups, multiples of 2^-24 (exact in float32 and float64)"""
    a, b = words(s, n, step, DROP_A), words(s, n, step, DROP_B)
    w = np.stack([a[0], a[1], a[2], a[3], b[0]]).astype(np.uint64)
    return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def report_mask(s, n, step):
    """(n,) int32: bits of the rows that report at `step`"""
    u = uniforms(s, n, step)
    mask = np.zeros(n, np.int32)
    for j in range(GROUPS):
        due = (int(step) - s.phase[j]) % s.period[j] == 0
        # (the comparison is the device's: its float32 dropout against an exact multiple of 2^-24)
        rep = due & ~(u[j] < np.float64(np.float32(s.dropout[j])))
        mask |= np.where(rep, 7 << (3 * j), 0).astype(np.int32)
    return mask


def sense(x, sigma_r, s, step, eps=0.0):
    """-> Z (15, n) (NaN where a row does not report), mask (n,), the noise-free h (15, n), the Box-Muller radius of every row"""
    n = x.shape[1]
    mask = report_mask(s, n, step)
    nrm, rad = normals(s, n, step, MEAS, 4)
    with np.errstate(all="ignore"):
        hx = E.h(x, np.asarray(s.mag, dtype=np.float64), eps)
    rep = ((mask[None, :] >> np.arange(15)[:, None]) & 1) == 1
    sg = np.broadcast_to(np.asarray(sigma_r, dtype=np.float64).reshape(15, -1), (15, n))
    return np.where(rep, hx + sg * nrm[:15], np.nan), mask, hx, rad[:15]


def disturb(x, sigma_q, s, step):
    """-> x [+] (sigma_q . normals) (13, n), d (12, n), the radii (12, n)"""
    n = x.shape[1]
    nrm, rad = normals(s, n, step, PROC, 3)
    d = np.broadcast_to(np.asarray(sigma_q, dtype=np.float64).reshape(12, -1), (12, n)) * nrm
    return E.boxplus(x, d), d, rad


def policy(fb, xnom, unom, Kx, lo, hi):
    """u (7, n) = clip(unom + Kx (fb - xnom)) in float64"""
    u = unom + np.einsum("rcn,cn->rn", Kx, fb - xnom)
    return np.minimum(np.maximum(u, np.asarray(lo)[:, None]), np.asarray(hi)[:, None])


def fmaf(a, b, c):
    """the correctly rounded float32 a * b + c of float32 arrays: the product is exact in float64; the sum is rounded to odd (its
    error from a two-sum), so the second rounding to float32 cannot double-round"""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    # towards err: one ulp up in magnitude when err has the sign of s, else the odd neighbour below
    up = (err > 0) == (s > 0)
    bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def policy32(fb, xnom, unom, Kx, lo, hi):
    """the float32 chain the header writes out: acc = Unom_r; acc = fmaf(Kx[r][c], fb_c - Xnom_c, acc) for c = 0 .. 12; clip"""
    f = lambda v: np.asarray(v, dtype=np.float32)  # noqa: E731
    fb, xnom, unom, Kx = f(fb), f(xnom), f(unom), f(Kx)
    dx = fb - xnom
    u = np.empty_like(unom)
    for r in range(7):
        acc = unom[r].copy()
        for c in range(13):
            acc = fmaf(Kx[r, c], dx[c], acc)
        u[r] = np.minimum(np.maximum(acc, np.float32(lo[r])), np.float32(hi[r]))
    return u


def score(x, xh, P):
    """-> e (12, n) = x [-] x^, nees (n,) = e' P^-1 e (NaN without a Cholesky factor), status (n,)"""
    n = x.shape[1]
    e = E.boxminus(x, xh)
    nees, status = np.full(n, np.nan), np.zeros(n, np.int32)
    for k in range(n):
        try:
            if not np.isfinite(P[:, :, k]).all():
                raise np.linalg.LinAlgError
            Lc = np.linalg.cholesky(P[:, :, k])
            y = np.linalg.solve(Lc, e[:, k])
            nees[k] = y @ y
        except np.linalg.LinAlgError:
            status[k] = 1
    return e, nees, status


def err_e(a, ref, P):
    """max_i |de_i| / sqrt(P_ii) per instance"""
    return (np.abs(a - ref) / np.sqrt(P[np.arange(12), np.arange(12)])).max(axis=0)


def rollout(orc, x0, xh0, P0, Xnom, Unom, Kx, Qd, Rd, sigma_q, sigma_r, s, dt, lo, hi, eps=0.0, feedback="estimate", step0=0):
    """The closed loop of ac_lqg_rollout_f32 with the EKF, in float64 -> dict of X, Xhat (T+1, 13, n), U, Z, mask, nis, nees, err,
    used, status per step"""
    T = Unom.shape[0]
    x, xh, P = np.array(x0, dtype=np.float64), np.array(xh0, dtype=np.float64), np.array(P0, dtype=np.float64)
    out = {k: [] for k in ("X", "Xhat", "U", "Z", "mask", "nis", "nees", "err", "used", "status")}
    out["X"].append(x)
    out["Xhat"].append(xh)
    for k in range(T):
        u = policy(xh if feedback == "estimate" else x, Xnom[k], Unom[k], Kx[k], lo, hi)
        x = orc.state_update(x, u, dt)
        if sigma_q is not None:
            x = disturb(x, sigma_q, s, step0 + k)[0]
        z, mask, _, _ = sense(x, sigma_r, s, step0 + k + 1, eps)
        xp, A = orc.step_sens(xh, u, dt)[:2]
        o = E.step(xh, P, xp, A, z, mask, Qd, Rd, np.asarray(s.mag, dtype=np.float64), eps)
        xh, P = o["X"], o["P"]
        e, nees, _ = score(x, xh, P)
        for key, v in (("X", x), ("Xhat", xh), ("U", u), ("Z", z), ("mask", mask), ("nis", o["nis"]), ("nees", nees), ("err", e),
                       ("used", o["used"]), ("status", o["status"])):
            out[key].append(v)
    return {k: np.stack(v) for k, v in out.items()}


# ---- the host build's entry points (tests/host_lqg/lqg_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) -------------------------
_fp, _ip, c32 = E._fp, E._ip, E.c32


def sense_opts(s):
    from aircraft_amd import _lib

    o = _lib.SenseOpts()
    o.mag_ned[:] = [float(v) for v in s.mag]
    o.seed_lo, o.seed_hi = int(s.seed) & 0xFFFFFFFF, int(s.seed) >> 32
    o.instance_offset = int(s.instance_offset)
    o.period[:], o.phase[:], o.dropout[:] = s.period, s.phase, s.dropout
    return o


def _lib_host(header):
    from tests.test_host_lqg import lib_host

    return lib_host(header)


def rows32(a, rows, n):
    return c32(np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(rows, -1), (rows, n)))


def host_schedule(s, step, T, n, header=None):
    out = np.zeros((T, n), np.int32)
    o = sense_opts(s)
    assert _lib_host(header).host_lqg_schedule(C.byref(o), int(step), T, n, _ip(out)) == 0
    return out


def host_sense(x, sigma_r, s, step, eps=0.0, header=None):
    n = x.shape[1]
    xs, sg = c32(x), rows32(sigma_r, 15, n)
    Z, mask = np.zeros((15, n), np.float32), np.zeros(n, np.int32)
    o = sense_opts(s)
    assert _lib_host(header).host_lqg_sense(C.byref(o), C.c_float(eps), int(step), _fp(xs), _fp(sg), n, _fp(Z), _ip(mask)) == 0
    return Z, mask


def host_disturb(x, sigma_q, s, step, header=None):
    n = x.shape[1]
    xs, sg = c32(x), rows32(sigma_q, 12, n)
    Xo = np.zeros((13, n), np.float32)
    o = sense_opts(s)
    assert _lib_host(header).host_lqg_disturb(C.byref(o), int(step), _fp(xs), _fp(sg), n, _fp(Xo)) == 0
    return Xo


def host_policy(fb, xnom, unom, Kx, lo, hi, header=None):
    n = fb.shape[1]
    a = [c32(np.asarray(lo, dtype=np.float64)), c32(np.asarray(hi, dtype=np.float64)), c32(fb), c32(xnom), c32(unom), c32(np.reshape(Kx, (91, n)))]
    U = np.zeros((7, n), np.float32)
    assert _lib_host(header).host_lqg_policy(*[_fp(v) for v in a], n, _fp(U)) == 0
    return U


def host_score(x, xh, P, header=None):
    n = x.shape[1]
    a = [c32(x), c32(xh), c32(np.reshape(P, (144, n)))]
    e, nees, st = np.zeros((12, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    assert _lib_host(header).host_lqg_score(*[_fp(v) for v in a], n, _fp(e), _fp(nees), _ip(st)) == 0
    return e, nees, st
