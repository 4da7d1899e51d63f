"""GPU: the device side of hipstr_amd/csrc/float_lse.h — the code every kernel inlines — against the oracle's restatement, bit for bit,
over every float argument the functions can receive (float_lse_cases.py; test_float_lse.py pins the oracle to the compiled reference and
the header's host side to the oracle over the same ranges).  hipstr_debug_float_fn makes the arguments on the device and returns result
bits only; a band is at most 2^26 arguments.  On a mismatch the first few (argument bits, got, want) are reported.

The device has its own conversions, its own reciprocal and a hand-made division (v_rcp_f32, a Newton step, a residual correction)
where the host divides: the division is swept over every float denominator of both of its ranges against the host's IEEE quotient,
and the control — the bare n * rcp(d) — must fail somewhere in each, which shows that the sweep reaches denominators a shorter
sequence gets wrong.

NaN and infinities are left out: the reference's behaviour there is not relied on anywhere (float_lse_cases.py)."""
import numpy as np
import pytest

from hipstr_amd import capi
import float_lse_cases as fc
from test_float_lse import check_lse2, check_lse_vec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fn,band,lo,count", fc.SWEEPS, ids=fc.SWEEP_IDS)
def test_device_equals_oracle(hmm, oracle, fn, band, lo, count):
    got = capi.float_fn(hmm, "hipstr_debug_float_fn", fn, lo, count)
    want = capi.float_fn(oracle, "oracle_float_fn", fn, lo, count)
    bad, n = fc.first_bad(lo, got, want)
    assert n == 0, "%s: %d of %d results differ, first %s" % (fn, n, count, " ".join(bad))
    if band == "const":     # |p| <= 2^-27: one value for all of them (fastexp: bits 0x3f800080)
        assert np.all(got == got[0]) and (fn != "fastexp" or got[0] == fc.FASTEXP_CONST), (fn, hex(got[0]), np.unique(got)[:4])
    if fn == "fastexp" and band == "-0.0":
        assert got[0] == 0x3F800000


@pytest.mark.parametrize("fn,ctl", [("div_pow2", "rcp_pow2"), ("div_log", "rcp_log")])
def test_division_control_fails(hmm, oracle, fn, ctl):
    """n * rcp(d), without the Newton step and the correction, is NOT the IEEE quotient somewhere among the swept denominators."""
    lo, hi = fc.DIV_BANDS[fn]; count = hi - lo + 1
    d = (np.uint32(lo) + np.arange(count, dtype=np.uint32)).view(np.float32)
    want = (fc.DIV_NUM[fn] / d).view(np.uint32)                      # numpy's float32 quotient: the host's IEEE division
    assert np.array_equal(want, capi.float_fn(oracle, "oracle_float_fn", fn, lo, count))
    got = capi.float_fn(hmm, "hipstr_debug_float_fn", ctl, lo, count)
    n = int(np.count_nonzero(got != want))
    print("%s: n * rcp(d) differs from the quotient at %d of %d denominators" % (fn, n, count))
    assert n > 0


@pytest.fixture(scope="module")
def pairs():
    return fc.lse2_pairs()


@pytest.fixture(scope="module")
def rows():
    return fc.lse_rows()


def test_lse2_device_equals_oracle(hmm, oracle, pairs):
    """The double wrapper on the device: strict threshold test (the threshold itself and one double ulp either side), ordering ((a, b)
    and (b, a) give the same bits, a == b, +-0.0), the double-to-float cast at and around the midpoints between adjacent floats,
    |hi| from 10^-3 to 10^5 and the library's "impossible" magnitude, the final double addition."""
    check_lse2(pairs, lambda a, b: capi.fast_lse2(hmm, "hipstr_debug_fast_lse2", a, b), lambda a, b: capi.fast_lse2(oracle, "oracle_fast_lse2_batch", a, b))


def test_lse_vec_device_equals_oracle(hmm, oracle, rows):
    """The streaming Lse on the device over rows of 1, 2, 63, 64, 65, 300 and 4096 values that straddle the threshold, all-equal rows, and
    every row reversed and shuffled: float terms summed in double are exact in any order, so the bits must not move."""
    check_lse_vec(rows, lambda r: capi.fast_lse_vec(hmm, "hipstr_debug_fast_lse_vec", r), lambda r: capi.fast_lse_vec(oracle, "oracle_fast_lse_vec_batch", r))
