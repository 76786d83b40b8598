"""Float64 restatement of the flight-mode analysis (aircraft_amd/csrc/ac_eig.hpp; include/aircraft_hip.h, ac_eig_f32 and
ac_modes_f32) for the tests: the structural zeros, the selection of chart coordinates, the closed loop, the
eigenvalues and s = log(lambda) / dt; the matching distance between two eigenvalue sets; the canonical order; the host
build's entry points; the recorded worst e32 and the case sets C1-C5.  TEST INFRASTRUCTURE, NOT PRODUCT."""
import ctypes as C

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import lqr_ref as L

FLIGHT = (3, 4, 5, 6, 7, 9, 10, 11)
PATH = tuple(i for i in range(12) if L.Q11[i] != 0)
ALL = tuple(range(12))
COORDS = {"8": FLIGHT, "11": PATH, "12": ALL}
DT = L.DT
MAX_ITERS = 30

# e32: the float32 outputs of the host build (g++, -ffp-contract=off; float64 arithmetic inside) against float64 eigvals of THE SAME float32 matrix, worst instance per case
# set, as the matching distance err_eig below (tests/test_host_modes.py measures them and fails when an instance exceeds
# 2 x; DESIGN.md §4.16 quotes them).  "s" is err_s on C1 (s dt of the flight blocks).  The GPU tests assert the host/float64
# pair within 2 x these first, then the device within 8 x the batch's worst host e32.
E32_WORST = {"C1": 5.9e-8, "C2": 3.0e-8, "C3": 5.9e-8, "C5": 5.9e-8, "s": 3.6e-7, "chain": 1.8e-5, "chain_s": 1.8e-5}


def f32x(a):
    return L.f32x(a)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------
def structural(A):
    """a copy of A_xi (12, 12, n) with the entries [flight rows][columns 0, 1, 2, 8] exactly 0"""
    A = np.array(A, dtype=np.float64)
    for r in FLIGHT:
        A[r, list(L.IGNORABLE)] = 0.0
    return A


def matrix(A, B=None, K=None, coords=FLIGHT):
    """the matrix whose eigenvalues ac_modes_f32 returns, in float64: structural zeros, minus B K, rows and columns of coords"""
    M = structural(A)
    if K is not None:
        M = M - L.mm(np.asarray(B, dtype=np.float64), np.asarray(K, dtype=np.float64))
    c = list(coords)
    return M[np.ix_(c, c)]


def eigvals(M):
    """float64 eigenvalues of every instance of M (m, m, n) -> (m, n) complex (LAPACK's order: compare by matching only)"""
    M = np.asarray(M, dtype=np.float64)
    return np.stack([np.linalg.eigvals(M[:, :, i]) for i in range(M.shape[2])], axis=-1)


def s_of(lam, dt):
    """s = log(lambda) / dt"""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(lam, dtype=np.complex128)) / dt


def reference(A, B=None, K=None, coords=FLIGHT, dt=DT):
    lam = eigvals(matrix(A, B, K, coords))
    return lam, s_of(lam, dt)


# ---- measures ----------------------------------------------------------------------------------------------------------------
def match_dist(a, b):
    """largest distance in the assignment of the set a to the set b that minimises the summed distance"""
    D = np.abs(np.asarray(a)[:, None] - np.asarray(b)[None, :])
    r, c = linear_sum_assignment(D)
    return float(D[r, c].max())


def err_eig(a, b):
    """per instance: match_dist / max(1, max |b|) for a, b (m, n); inf where a is not finite"""
    out = np.full(a.shape[1], np.inf)
    for i in range(a.shape[1]):
        if np.isfinite(a[:, i]).all():
            out[i] = match_dist(a[:, i], b[:, i]) / max(1.0, float(np.abs(b[:, i]).max()))
    return out


def err_s(sa, sb, dt):
    """err_eig on s dt"""
    return err_eig(np.asarray(sa) * dt, np.asarray(sb) * dt)


def check_order(wr, wi):
    """the canonical order and the conjugate pairs of float32 outputs wr, wi (m, n), bitwise"""
    wr, wi = np.asarray(wr, dtype=np.float32), np.asarray(wi, dtype=np.float32)
    for i in range(wr.shape[1]):
        r, im = wr[:, i], wi[:, i]
        if not np.isfinite(r).all():
            continue
        mag = r * r + im * im  # float32 products and sum, as the routine forms them
        key = [(-float(mag[k]), -float(im[k]), -float(r[k])) for k in range(len(r))]
        assert key == sorted(key), ("order", i, r, im)
        # every + member has its - member: the same real part bit for bit, the imaginary part negated (reals of the same
        # float32 modulus may stand between the two)
        free = [k for k in range(len(r)) if im[k] < 0]
        for k in range(len(r)):
            if im[k] > 0:
                mate = [j for j in free if im[j] == -im[k] and r[j] == r[k]]
                assert mate, ("pair", i, r, im)
                free.remove(mate[0])
        assert not free, ("pair", i, r, im)


U32 = 2.0 ** -24  # float32 unit roundoff


def sigma_form_err(raw, m, dt):
    """How well sigma and omega [raw rows 2, 3] agree with the logarithm of the routine's OWN float32 eigenvalues [rows 0, 1],
    per instance, as a fraction of what the log1p form may lose.  With t = |wr^2 - 1| + wi^2 and u = 2^-24:
    d = fma(wr - 1, fl(wr + 1), fl(wi^2)) carries at most 3 u t (the difference is exact for 1/2 <= wr <= 2, else one more
    rounding, counted), which log1p divides by 1 + d = |lambda|^2; log1pf itself is good to 2 ulp = 4 u |log1p d|, and the
    division by dt rounds once more.  For sigma dt = log1p(d) / 2 that is 1.5 u t / |lambda|^2 + 2.5 u |log1p d|.  omega dt: atan2f to
    2 ulp and one division, 5 u |omega dt|.  log(hypot(wr, wi)) instead loses u |lambda| in sigma dt: thousands of times the bound
    where |lambda| - 1 is 1e-4.  The step is the float32 dt the kernel divides by.  -> (sigma error / bound, omega error / bound)"""
    wr, wi, sg, om = (np.asarray(raw[k][:m], dtype=np.float64) for k in range(4))
    dt32 = float(np.float32(dt))
    t, mag2 = np.abs(wr * wr - 1.0) + wi * wi, wr * wr + wi * wi
    l1p = np.log1p((wr - 1.0) * (wr + 1.0) + wi * wi)
    es = np.abs(sg * dt32 - 0.5 * l1p) / (U32 * (1.5 * t / mag2 + 2.5 * np.abs(l1p)) + 1e-300)
    eo = np.abs(om * dt32 - np.arctan2(wi, wr)) / (5 * U32 * np.abs(np.arctan2(wi, wr)) + 1e-300)
    return es.max(axis=0), eo.max(axis=0)


# ---- the host build's entry points (tests/host_modes/modes_host.cpp: g++, -DAC_HOST_CHECK -ffp-contract=off) -------------------
_FP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int)


def _host(header=None):
    from tests.test_host_modes import lib_host

    return lib_host(header)


def _fp(a):
    return a.ctypes.data_as(_FP)


def host_eig(M, max_iters=MAX_ITERS, header=None):
    """-> lam (m, n) complex128, status, iters, and the float32 (wr, wi) of the host build on float32-rounded M (m, m, n)"""
    m, n = M.shape[0], M.shape[2]
    a = L.c32(np.reshape(M, (m * m, n)))
    wr, wi = np.zeros((m, n), np.float32), np.zeros((m, n), np.float32)
    st, it = np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert _host(header).host_eig(_fp(a), m, int(max_iters), n, _fp(wr), _fp(wi), st.ctypes.data_as(_IP), it.ctypes.data_as(_IP)) == 0
    return wr.astype(np.float64) + 1j * wi, st, it, (wr, wi)


def coords_mask(coords):
    return sum(1 << int(c) for c in coords)


def host_modes(A, B=None, K=None, coords=FLIGHT, dt=DT, max_iters=MAX_ITERS, header=None):
    """k_modes_eig's unit on float32-rounded A_xi (12, 12, n), B_xi, K -> lam, s (m, n) complex128, status, iters, raw [4][12][n]"""
    n, m = A.shape[2], len(coords)
    a = L.c32(np.reshape(A, (144, n)))
    b = L.c32(np.reshape(B, (84, n))) if K is not None else None
    k = L.c32(np.reshape(K, (84, n))) if K is not None else None
    out = np.zeros((4, 12, n), np.float32)
    st, it = np.zeros(n, np.int32), np.zeros(n, np.int32)
    rc = _host(header).host_modes_eig(_fp(a), _fp(b) if b is not None else None, _fp(k) if k is not None else None,
                                      coords_mask(coords), m, int(max_iters), C.c_float(dt), n, _fp(out[0]), _fp(out[1]),
                                      _fp(out[2]), _fp(out[3]), st.ctypes.data_as(_IP), it.ctypes.data_as(_IP))
    assert rc == 0
    o = out.astype(np.float64)
    return o[0, :m] + 1j * o[1, :m], o[2, :m] + 1j * o[3, :m], st, it, out


def embed_flight(M):
    """an 8 x 8 flight block (8, 8, n) as the A_xi (12, 12, n) whose flight block it is (zero elsewhere)"""
    A = np.zeros((12, 12, M.shape[2]))
    A[np.ix_(FLIGHT, FLIGHT)] = M
    return A


# ---- the case sets -----------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def projection(name, dt=DT):
    """float64 oracle projection (A_xi, B_xi) on lqr_ref.grid(name)"""
    def make():
        ac, orc, x, u = L.grid(name)
        return L.oracle_projection(orc, x, u, dt)

    return _cached(("proj", name, dt), make)


C1_KEYS = (("poly", 0.01), ("default", 0.01), ("linear", 0.01), ("real_net", 0.01), ("poly", 0.05))


def c1():
    """flight: {label: (M (8, 8, n) float32-exact, dt)}"""
    return _cached("c1", lambda: {f"{name}@{dt}": (f32x(matrix(projection(name, dt)[0])), dt) for name, dt in C1_KEYS})


def closed_gains(name, sel):
    """lqr_ref.solve's float64 K on the float32-rounded oracle projection, and the instances that converged"""
    def make():
        A, B = (f32x(a) for a in projection(name))
        _, K, _, st, _ = L.solve(A, B, L.SELECTIONS[sel])
        return K, st == 0

    return _cached(("K", name, sel), make)


def c2():
    """closed: A_xi - B_xi K for the selections 8, 11, 12 on poly and default, converged instances only"""
    def make():
        out = {}
        for name in ("poly", "default"):
            A, B = (f32x(a) for a in projection(name))
            for sel in ("8", "11", "12"):
                K, ok = closed_gains(name, sel)
                out[f"{name}:{sel}"] = (f32x(matrix(A[..., ok], B[..., ok], K[..., ok], COORDS[sel])), DT)
        return out

    return _cached("c2", make)


def raw_jacobian(name, dt=DT):
    def make():
        ac, orc, x, u = L.grid(name)
        return orc.step_sens(x, u, dt)[1]

    return _cached(("raw", name, dt), make)


def c3():
    """full: the 12 x 12 A_xi (structural zeros, all coordinates) and the raw 13 x 13 A on poly and default"""
    def make():
        out = {}
        for name in ("poly", "default"):
            out[f"{name}:all"] = (f32x(matrix(projection(name)[0], coords=ALL)), DT)
            out[f"{name}:raw13"] = (f32x(raw_jacobian(name)), DT)
        return out

    return _cached("c3", make)


def cyclic(m):
    P = np.zeros((m, m))
    for i in range(m):
        P[(i + 1) % m, i] = 1.0
    return P


def companion():
    """companion matrix of (l - 0.5)(l^2 - 1.8 l + 0.85)(l + 2): roots 0.5, 0.9 +- 0.2i, -2"""
    p = np.polymul(np.polymul([1, -0.5], [1, -1.8, 0.85]), [1, 2.0])
    Cm = np.zeros((4, 4))
    Cm[0] = -p[1:]
    Cm[1:, :3] = np.eye(3)
    return Cm, np.array([0.5, 0.9 + 0.2j, 0.9 - 0.2j, -2.0])


def upper13():
    rng = np.random.default_rng(13)
    return f32x(np.triu(rng.standard_normal((13, 13))))


def badly_scaled():
    """D S D^-1 of a C1 block, D = diag(2^+-12): (M (8, 8, n), the block S itself)"""
    S = c1()["poly@0.01"][0]
    d = 2.0 ** (12 * np.array([1, -1, 1, -1, -1, 1, -1, 1]))
    return f32x(S * d[:, None, None] / d[None, :, None]), S


def c5(m, n, seed=0):
    """shapes: seeded Gaussian matrices (m, m, n)"""
    return f32x(np.random.default_rng(1000 * seed + 17 * m + n).standard_normal((m, m, n)))


# ---- the chain from (x, u) -----------------------------------------------------------------------------------------------------
CHAIN_MODELS = ("poly", "default", "real_net")
CHAIN_LOOPS = (("open", "8"), ("open", "12"), ("closed", "8"), ("closed", "12"))


def chain64(orc, x, u, K=None, coords=FLIGHT, dt=DT):
    """all float64: the oracle's step sensitivities, the projection, the structural zeros, A - B K, the selection, eigvals, s"""
    xp, A, B, _ = orc.step_sens(x, u, dt)
    Ax, Bx = L.project(x, xp, A, B)
    return reference(Ax, Bx, K, coords, dt)


def chain32(orc, x, u, K=None, coords=FLIGHT, dt=DT):
    """the float32 chain: the host build's projection of the oracle's float32-rounded (x+, A, B), then the host build's
    eigenvalues -> lam, s, status"""
    xp, A, B, _ = (f32x(a) for a in orc.step_sens(x, u, dt))
    Ax, Bx = L.host_project(x, xp, A, B)
    lam, s, st, _, _ = host_modes(Ax, Bx, K, coords, dt)
    return lam, s, st


def chain_e32(orc, x, u, K=None, coords=FLIGHT, dt=DT):
    """per instance: err_eig and err_s of the float32 chain against the float64 chain, and the float64 chain itself"""
    lam64, s64 = chain64(orc, x, u, K, coords, dt)
    lam32, s32, st = chain32(orc, x, u, K, coords, dt)
    return err_eig(lam32, lam64), err_s(s32, s64, dt), lam64, s64


def check_textbook(solve):
    """C4 with exact answers; solve(M (m, m, n), max_iters) -> lam, status, iters, (wr, wi) is the host build or the device"""
    def one(Mx, max_iters=MAX_ITERS):
        lam, st, it, (wr, wi) = solve(np.asarray(Mx, dtype=np.float64)[:, :, None], max_iters)
        return lam[:, 0], int(st[0]), int(it[0]), wr[:, 0], wi[:, 0]

    lam, st, it, wr, wi = one([[2.5]])
    assert st == 0 and it == 0 and wr[0] == np.float32(2.5) and wi[0] == 0
    lam, st, it, wr, wi = one([[0, 1], [-1, 0]])
    assert st == 0 and list(wr) == [0, 0] and list(wi) == [1, -1]
    for m in (3, 4):  # the trailing 2 x 2 gives zero shifts: no progress without the exceptional shifts
        lam, st, it, wr, wi = one(cyclic(m))
        assert st == 0 and it > 10, (m, st, it)
        assert match_dist(lam, np.exp(2j * np.pi * np.arange(m) / m)) <= 4e-7, (m, lam)
        check_order(wr[:, None], wi[:, None])
    U = upper13()
    lam, st, it, wr, wi = one(U)
    assert st == 0 and it == 0 and (wi == 0).all()
    assert sorted(wr.tolist()) == sorted(np.diag(U).astype(np.float32).tolist())  # bit for bit
    check_order(wr[:, None], wi[:, None])
    # the same matrix with rows and columns shuffled: the permutation search alone still isolates every eigenvalue
    perm = np.random.default_rng(5).permutation(13)
    lam, st, it, wr2, wi2 = one(U[np.ix_(perm, perm)])
    assert st == 0 and it == 0 and np.array_equal(wr2, wr) and (wi2 == 0).all(), (it, wr2 - wr)
    for Z, v in ((np.zeros((7, 7)), 0.0), (np.eye(6), 1.0)):
        lam, st, it, wr, wi = one(Z)
        assert st == 0 and it == 0 and (wr == v).all() and (wi == 0).all()
    Cm, roots = companion()
    lam, st, it, wr, wi = one(Cm)
    assert st == 0 and match_dist(lam, roots) <= 2e-6, lam
    check_order(wr[:, None], wi[:, None])
    # status 3: one NaN, one Inf; status 1: one iteration per eigenvalue is not enough for a flight block
    S = c1()["poly@0.01"][0][:, :, 0]
    for v in (np.nan, np.inf):
        bad = S.copy()
        bad[2, 5] = v
        lam, st, it, wr, wi = one(bad)
        assert st == 3 and it == 0 and np.isnan(wr).all() and np.isnan(wi).all()
    lam, st, it, wr, wi = one(S, max_iters=1)
    assert st == 1 and np.isnan(wr).all() and np.isnan(wi).all()


def check_balancing(solve):
    """D S D^-1 with D = diag(2^+-12) of a C1 block: C1's error level against the eigenvalues of S"""
    Mx, S = badly_scaled()
    lam, st, it, _ = solve(Mx, MAX_ITERS)
    e = err_eig(lam, eigvals(S))
    assert (st == 0).all() and (e <= 2 * E32_WORST["C1"]).all(), float(e.max())
