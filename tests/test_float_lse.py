"""CPU: the float log-sum-exp primitives, exhaustively.  Every number the library produces passes through the reference's bit-trick
fasterexp / fasterlog (vector log-sum-exp) and fastexp / fastlog (pair log-sum-exp); their arguments are floats, so the ranges they
can receive are enumerated in full (float_lse_cases.py) and every comparison is bit equality:

  * the oracle's restatement (oracle/hipstr_oracle.c) against the compiled reference's own functions — skipped where the compiled
    reference is not built, as in test_oracle_vs_ref.py;
  * the host side of hipstr_amd/csrc/float_lse.h — what em.hip's host path and prep.cpp run — against the oracle;
  * a numpy float32 restatement against the oracle on one band of 2^23 arguments per function: a witness that no C compiler's
    contraction or excess-precision choice can touch.

NaN and infinities are left out: the reference's behaviour there is not relied on anywhere (float_lse_cases.py).
test_float_lse_gpu.py compares the header's device side with the same oracle over the same ranges."""
import numpy as np
import pytest

from hipstr_amd import capi
import float_lse_cases as fc

needs_ref = pytest.mark.skipif(not capi.have_ref(), reason="compiled reference not available")


@pytest.fixture(scope="module")
def ref():
    return capi.load_ref()


def _check(fn, lo, count, got, want):
    bad, n = fc.first_bad(lo, got, want)
    assert n == 0, "%s: %d of %d results differ, first %s" % (fn, n, count, " ".join(bad))


@needs_ref
@pytest.mark.parametrize("fn,band,lo,count", fc.SWEEPS, ids=fc.SWEEP_IDS)
def test_oracle_equals_reference(oracle, ref, fn, band, lo, count):
    _check(fn, lo, count, capi.float_fn(oracle, "oracle_float_fn", fn, lo, count), capi.float_fn(ref, "ref_float_fn", fn, lo, count))


@pytest.mark.parametrize("fn,band,lo,count", fc.SWEEPS, ids=fc.SWEEP_IDS)
def test_header_host_equals_oracle(oracle, hmm_host, fn, band, lo, count):
    got = capi.float_fn(hmm_host, "hipstr_debug_float_fn_host", fn, lo, count)
    _check(fn, lo, count, got, capi.float_fn(oracle, "oracle_float_fn", fn, lo, count))
    if band == "const":     # |p| <= 2^-27: one value for all of them (fastexp: bits 0x3f800080)
        assert np.all(got == got[0]) and (fn != "fastexp" or got[0] == fc.FASTEXP_CONST), (fn, hex(got[0]), np.unique(got)[:4])
    if fn == "fastexp" and band == "-0.0":
        assert got[0] == 0x3F800000


def test_pair_term_stays_inside_the_fastlog_sweep(oracle):
    """1 + fastexp(p) over the whole sweep of p lies in [1, 0x1.001p+1], the range fastlog is swept over (its maximum is 0x1.0000cp+1)."""
    top = 0
    for _, lo, count in fc.EXP_BANDS:
        e = capi.float_fn(oracle, "oracle_float_fn", "fastexp", lo, count).view(np.float32)
        x = (np.float32(1) + e).view(np.uint32)
        assert x.min() >= 0x3F800000
        top = max(top, int(x.max()))
    assert top == 0x40000060 and top <= 0x40000800, hex(top)


# ---------------------------------------------------------------------------------------------- numpy float32 witness
_f = np.float32


def _np_fasterexp(p):
    y = _f(1.442695040) * p
    c = np.where(y < _f(-126), _f(-126), y)
    return (_f(8388608) * (c + _f(126.94269504))).astype(np.uint32)


def _np_fasterlog(x):
    y = x.view(np.uint32).astype(np.float32) * _f(8.2629582881927490e-8)
    return (y - _f(87.989971088)).view(np.uint32)


def _np_fastexp(p):
    q = _f(1.442695040) * p
    offset = np.where(q < 0, _f(1), _f(0))
    c = np.where(q < _f(-126), _f(-126), q)
    w = np.trunc(c).astype(np.int32)
    z = c - w.astype(np.float32) + offset
    t = c + _f(121.2740575) + _f(27.7280233) / (_f(4.84252568) - z) - _f(1.49012907) * z
    return (_f(8388608) * t).astype(np.uint32)


def _np_fastlog(x):
    vi = x.view(np.uint32)
    mx = ((vi & np.uint32(0x007FFFFF)) | np.uint32(0x3F000000)).view(np.float32)
    y = vi.astype(np.float32) * _f(1.1920928955078125e-7)
    l2 = y - _f(124.22551499) - _f(1.498030302) * mx - _f(1.72587999) / (_f(0.3520887068) + mx)
    return (_f(0.69314718) * l2).view(np.uint32)


def _np_lse2_term(p):
    return _np_fastlog(_f(1) + _np_fastexp(p).view(np.float32))


_NP = {"fasterexp": (_np_fasterexp, 0xC0000000), "fastexp": (_np_fastexp, 0xC0000000), "lse2_term": (_np_lse2_term, 0xC0000000),   # [-4, -2)
       "fastlog": (_np_fastlog, 0x3F800000), "fasterlog": (_np_fasterlog, 0x40800000)}                                             # [1, 2), [4, 8)


@pytest.mark.parametrize("fn", sorted(_NP))
def test_numpy_restatement_equals_oracle(oracle, fn):
    f, lo = _NP[fn]; count = 1 << 23
    x = (np.uint32(lo) + np.arange(count, dtype=np.uint32)).view(np.float32)
    assert all(type(v) is np.float32 for v in (_f(1) * x[0], x[0] - _f(1)))      # the arithmetic stays in float32
    _check(fn, lo, count, f(x), capi.float_fn(oracle, "oracle_float_fn", fn, lo, count))


@pytest.mark.parametrize("fn", sorted(fc.DIV_BANDS))
def test_numpy_quotient_equals_oracle(oracle, fn):
    lo, hi = fc.DIV_BANDS[fn]; count = hi - lo + 1
    d = (np.uint32(lo) + np.arange(count, dtype=np.uint32)).view(np.float32)
    _check(fn, lo, count, (fc.DIV_NUM[fn] / d).view(np.uint32), capi.float_fn(oracle, "oracle_float_fn", fn, lo, count))


# ---------------------------------------------------------------------------------------------- the double wrappers
@pytest.fixture(scope="module")
def pairs():
    return fc.lse2_pairs()


@pytest.fixture(scope="module")
def rows():
    return fc.lse_rows()


def _same_bits(got, want, what, args):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, "%s: %d differ, first %s" % (what, bad.size, [(args(i), got[i].hex(), want[i].hex()) for i in bad[:6]])


def check_lse2(pairs, run, want_run):
    """fast_log_sum_exp(a, b) from `run` against `want_run` on every pair both ways round; the two orders give the same bits."""
    a, b = pairs
    ab, ba = run(a, b), run(b, a)
    _same_bits(ab, want_run(a, b), "lse2(a, b)", lambda i: (a[i].hex(), b[i].hex()))
    _same_bits(ba, ab, "lse2(b, a) against lse2(a, b)", lambda i: (a[i].hex(), b[i].hex()))
    # what the cases are there for: both sides of the strict threshold are taken, and the threshold itself takes the float path
    d = np.where(a > b, b - a, a - b); hi = np.maximum(a, b)
    below = d < fc.LOG_THRESH
    assert below.any() and (~below).any() and (d == fc.LOG_THRESH).any()
    assert np.array_equal(ab[below], hi[below]) and np.all(ab[~below] > hi[~below])


def check_lse_vec(rows, run, want_run):
    """fast_log_sum_exp(vector) from `run` against `want_run`; a row reversed or shuffled gives the same bits."""
    rr, groups = rows
    got = run(rr)
    _same_bits(got, want_run(rr), "lse_vec", lambda i: (len(rr[i]), rr[i][:4].tolist()))
    for g in groups:
        assert len(set(got[g].view(np.uint64).tolist())) == 1, (len(rr[g[0]]), [x.hex() for x in got[g]])


@needs_ref
def test_lse2_oracle_equals_reference(oracle, ref, pairs):
    check_lse2(pairs, lambda a, b: capi.fast_lse2(oracle, "oracle_fast_lse2_batch", a, b), lambda a, b: capi.fast_lse2(ref, "ref_fast_lse2_batch", a, b))


def test_lse2_header_host_equals_oracle(oracle, hmm_host, pairs):
    check_lse2(pairs, lambda a, b: capi.fast_lse2(hmm_host, "hipstr_debug_fast_lse2_host", a, b), lambda a, b: capi.fast_lse2(oracle, "oracle_fast_lse2_batch", a, b))


@needs_ref
def test_lse_vec_oracle_equals_reference(oracle, ref, rows):
    check_lse_vec(rows, lambda r: capi.fast_lse_vec(oracle, "oracle_fast_lse_vec_batch", r), lambda r: capi.fast_lse_vec(ref, "ref_fast_lse_vec_batch", r))


def test_lse_vec_header_host_equals_oracle(oracle, hmm_host, rows):
    check_lse_vec(rows, lambda r: capi.fast_lse_vec(hmm_host, "hipstr_debug_fast_lse_vec_host", r), lambda r: capi.fast_lse_vec(oracle, "oracle_fast_lse_vec_batch", r))


def test_thresholds_agree(oracle, hmm_host):
    """The library's LOG_THRESH is the double the cases are built around."""
    t = fc.LOG_THRESH
    a = np.array([t, np.nextafter(t, -np.inf)]); b = np.zeros(2)
    got = capi.fast_lse2(hmm_host, "hipstr_debug_fast_lse2_host", a, b)
    assert got[0] > 0.0 and got[1] == 0.0
