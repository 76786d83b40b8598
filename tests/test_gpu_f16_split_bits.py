"""The fused form of the f16 activation split (v_fma_mixlo_f16 / v_fma_mixhi_f16 of the residual times S = 2^11) gives the bits
of the form it replaced (two v_mul_f32 by S and a v_cvt_pk_f16_f32): csrc/f16_split_check.hip runs both on the device over every
finite fp32 pattern with |x| < 2^15 — the range the f16 gate admits — subnormals and both zeros included, in the low and in the
high half of a pair, and counts the patterns whose residual plane differs.  None may."""
import ctypes as C

import pytest

from aircraft_amd import _lib

pytestmark = pytest.mark.gpu

PATTERNS = 2 * 0x47000000  # magnitudes below the bits of 2^15, both signs


def test_fused_split_is_bit_identical_over_the_whole_range(gpu):
    out = (C.c_ulonglong * 4)()
    _lib.check(_lib.load().ac_f16_split_check(out), "ac_f16_split_check")
    low, high, seen, first = (int(v) for v in out)
    print(f"patterns {seen}; residual planes that differ: low half {low}, high half {high}"
          + (f"; e.g. fp32 bits {first - 1:#010x}" if first else ""))
    assert seen == PATTERNS
    assert low == 0 and high == 0
