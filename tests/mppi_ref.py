"""NumPy restatement of the MPPI noise, sampler and update (aircraft_amd/csrc/ac_mppi.hpp).
Philox4x32-10 in exact uint32 / uint64 arithmetic; normals, sample and update in float64."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
N_MAX = np.sqrt(48 * np.log(2.0))  # r at u1 = 2^-24


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counters and keys: broadcastable integer arrays.  Returns four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniforms(xa, xb):
    u1 = ((np.asarray(xa, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (np.asarray(xb, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def box_muller(xa, xb):
    """(na, nb, r) in float64 from one word pair."""
    u1, u2 = uniforms(xa, xb)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2), r


def normals(seed, it, K, B, H, instance_offset=0, want_radius=False):
    """n [H][7][K][B] (float64): the draw of (seed, it, k, g = instance_offset + b, t, row)."""
    k = np.arange(K, dtype=np.uint64)[None, :, None]
    g = (np.arange(B, dtype=np.uint64) + np.uint64(instance_offset))[None, None, :]
    t = np.arange(H, dtype=np.uint64)[:, None, None]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    n = np.empty((H, 8, K, B))
    rad = np.empty((H, 8, K, B))
    for j in (0, 1):
        x = philox4x32_10(k, g, t, (2 * int(it) + j) & 0xFFFFFFFF, k0, k1)
        for p in (0, 1):
            na, nb, r = box_muller(x[2 * p], x[2 * p + 1])
            n[:, 4 * j + 2 * p], n[:, 4 * j + 2 * p + 1] = na, nb
            rad[:, 4 * j + 2 * p] = rad[:, 4 * j + 2 * p + 1] = r
    return (n[:, :7], rad[:, :7]) if want_radius else n[:, :7]


def sample(Unom, sigma, u_min, u_max, seed, it, K, instance_offset=0, keep_nominal=True, want_radius=False):
    """Unom [H][7][B] -> Uc [H][7][K*B] (column k*B + b), float64."""
    Unom = np.asarray(Unom, dtype=np.float64)
    H, _, B = Unom.shape
    sg, lo, hi = (np.asarray(v, dtype=np.float64)[None, :, None, None] for v in (sigma, u_min, u_max))
    n, rad = normals(seed, it, K, B, H, instance_offset, want_radius=True)
    n = np.where(sg == 0, 0.0, n)
    if keep_nominal:
        n[:, :, 0, :] = 0.0
    Uc = np.minimum(np.maximum(Unom[:, :, None, :] + sg * n, lo), hi).reshape(H, 7, K * B)
    return (Uc, rad.reshape(H, 7, K * B)) if want_radius else Uc


def weights(J, K, lam):
    """J [K*B] -> (w normalised [K][B], stats [4][B]) in float64."""
    J = np.asarray(J, dtype=np.float64).reshape(K, -1)
    B = J.shape[1]
    fin = np.isfinite(J)
    Jm = np.where(fin, J, np.inf)
    jmin = Jm.min(axis=0)
    any_ = fin.any(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(fin, np.exp(-(Jm - np.where(any_, jmin, 0.0)) / lam), 0.0)
    eta = w.sum(axis=0)
    stats = np.zeros((4, B))
    stats[0] = jmin
    stats[1] = np.where(any_, eta ** 2 / np.maximum((w ** 2).sum(axis=0), 1e-300), 0.0)
    stats[2] = fin.sum(axis=0)
    stats[3] = np.where(any_, Jm.argmin(axis=0), -1)
    return np.where(any_, w / np.where(any_, eta, 1.0), 0.0), stats


def update(J, Uc, Unom, K, lam, u_min, u_max):
    """(Unew [H][7][B], stats [4][B]) in float64 from the given J [K*B], Uc [H][7][K*B], Unom [H][7][B]."""
    Unom = np.asarray(Unom, dtype=np.float64)
    H, _, B = Unom.shape
    w, stats = weights(J, K, lam)
    lo, hi = (np.asarray(v, dtype=np.float64)[None, :, None] for v in (u_min, u_max))
    blend = (np.asarray(Uc, dtype=np.float64).reshape(H, 7, K, B) * w[None, None]).sum(axis=2)
    Unew = np.where(stats[2][None, None, :] > 0, np.minimum(np.maximum(blend, lo), hi), Unom)
    return Unew, stats
