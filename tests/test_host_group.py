"""The column of the group Cholesky (aircraft_amd/csrc/ac_group.hpp: grp_chol_column) compiled for the
host with g++ (tests/host_group/group_host.cpp, -DAC_HOST_CHECK -ffp-contract=off) and driven through GroupHost: e32, the
float32 build against float64 (tests/group_ref.py) on identical float32-rounded matrices at the conditioning of the smoother's
grids; a failed pivot planted at column 0, 5 and 11; a NaN entry; mutated copies of the header that these checks must catch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import group_ref as G

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_group")
CSRC = os.path.abspath(os.path.join(os.path.dirname(HERE), "..", "aircraft_amd", "csrc"))
HEADER = os.path.join(CSRC, "ac_group.hpp")
FP = C.POINTER(C.c_float)
IP = C.POINTER(C.c_int)
_LIBS = {}


def lib_host(header=None):
    """the host build of ac_group.hpp, or of the copy `header` (built next to that copy)"""
    key = header or HEADER
    if key in _LIBS:
        return _LIBS[key]
    src = os.path.join(HERE, "group_host.cpp")
    so = os.path.join(HERE, "libgroup_host.so") if header is None else os.path.splitext(header)[0] + ".so"
    deps = [src, key, os.path.join(CSRC, "ac_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        cmd = ["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC]
        if header is not None:
            cmd.append(f'-DAC_GROUP_HEADER="{header}"')
        subprocess.run(cmd + ["-o", so, src], check=True)
    lib = C.CDLL(so)
    lib.host_group_chol.argtypes = [FP, FP, FP, IP]
    lib.host_group_chol.restype = C.c_int
    _LIBS[key] = lib
    return lib


def host_chol(M, header=None):
    """the float32 host build -> L (12, 12) float32, inv (12,) float32, ok (12,) bool"""
    m = np.ascontiguousarray(M, np.float32)
    L, inv, ok = np.zeros((12, 12), np.float32), np.zeros(12, np.float32), np.zeros(12, np.int32)
    p = lambda a: a.ctypes.data_as(FP)  # noqa: E731
    rc = lib_host(header).host_group_chol(p(m), p(L), p(inv), ok.ctypes.data_as(IP))
    assert rc == 0, "the lanes of the group disagree on a pivot"
    return L, inv, ok.astype(bool)


# ---- the e32 measurement -------------------------------------------------------------------------------------------------------
def measure(header=None):
    """e32 of every measure over group_ref.cases(): {measure: worst}"""
    worst = dict.fromkeys(G.E32_WORST, 0.0)
    for M in G.cases():
        L32, w32, ok = host_chol(M, header)
        assert ok.all(), "a pivot of a positive definite matrix failed"
        for k, v in G.errors(M, L32.astype(np.float64), w32.astype(np.float64)).items():
            worst[k] = max(worst[k], v)
    return worst


_MEASURED = []


def measured():
    if not _MEASURED:
        _MEASURED.append(measure())
    return _MEASURED[0]


def check(m):
    """the assertions a measurement has to meet (the mutated header must fail at least one)"""
    for key, bar in G.E32_WORST.items():
        assert m[key] <= bar, (key, m[key], bar)


def test_e32_within_recorded_worst():
    m = measured()
    print("[group e32] " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
    check(m)


def test_recorded_worst_is_not_slack():
    """E32_WORST is the measured worst, not a loose bound: each entry is within 3 x of what is measured."""
    for key, bar in G.E32_WORST.items():
        assert bar <= 3 * measured()[key], (key, measured()[key], bar)


# ---- failed pivots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("col", [0, 5, 11])
def test_planted_pivot_failure(col):
    """M_cc = 0 makes the pivot of column c fail (0 minus a sum of squares) and is read by no earlier column: the function
    reports it there, the earlier columns keep their bits, and column c is formed with pivot 1: inv_c = 1 and L_rc is the
    fmaf chain t itself, whose entry r = c is the failed pivot.  t is compared with the same sum in float64 over the host's
    own earlier columns: its c fused steps each round once, by at most 2^-24 of a partial sum that |M_rc| + sum |L_rk L_ck|
    bounds."""
    M = G.cases()[3]
    clean = host_chol(M)
    Mp = M.copy()
    Mp[col, col] = 0.0
    L32, inv, ok = host_chol(Mp)
    assert ok[:col].all() and not ok[col] and inv[col] == 1.0
    assert np.array_equal(L32[:, :col].view(np.uint32), clean[0][:, :col].view(np.uint32))
    assert np.array_equal(inv[:col].view(np.uint32), clean[1][:col].view(np.uint32))
    Lp = L32[:, :col].astype(np.float64)
    t = Mp[:, col] - Lp @ Lp[col]
    bound = col * 2.0 ** -24 * (np.abs(Mp[:, col]) + np.abs(Lp) @ np.abs(Lp[col])) * (1 + 2.0 ** -20)
    assert (np.abs(L32[col:, col] - t[col:]) <= bound[col:]).all(), (L32[col:, col], t[col:], bound[col:])
    assert L32[col, col] <= 0.0
    if col == 0:
        assert np.array_equal(L32[:, 0], Mp[:, 0].astype(np.float32))


def test_nan_entry():
    """a NaN in M_73 (and M_37): columns 0-2 keep their bits, L_73 is NaN, the pivot of column 7 is not finite and is reported;
    every pivot that fails is replaced by 1, so 1 / L_jj stays finite whatever the matrix holds"""
    M = G.cases()[3]
    clean = host_chol(M)
    Mn = M.copy()
    Mn[7, 3] = Mn[3, 7] = np.nan
    L32, inv, ok = host_chol(Mn)
    assert ok[:7].all() and not ok[7] and inv[7] == 1.0 and np.isnan(L32[7, 3])
    assert np.array_equal(L32[:, :3].view(np.uint32), clean[0][:, :3].view(np.uint32))
    assert np.isfinite(inv).all() and (inv > 0).all()


# ---- a mutated header must fail ----------------------------------------------------------------------------------------------------
MUTATIONS = {
    "pivot_sum_dropped": ("d = fmaf(-lj, lj, d);", ""),
    "row_sum_against_the_wrong_row": ("const float lj = m[j][c];", "const float lj = m[r][c];"),
}


@pytest.mark.parametrize("which", sorted(MUTATIONS))
def test_mutated_header_fails(which, tmp_path):
    old, new = MUTATIONS[which]
    text = open(HEADER).read()
    assert text.count(old) == 1, which
    path = str(tmp_path / f"ac_group_{which}.hpp")
    with open(path, "w") as f:
        f.write(text.replace(old, new).replace('#include "ac_math.hpp"', f'#include "{CSRC}/ac_math.hpp"'))
    with pytest.raises(AssertionError):
        check(measure(path))
