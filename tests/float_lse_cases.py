"""The argument ranges and cases of the float log-sum-exp sweeps, shared by test_float_lse.py (CPU: oracle against the compiled reference,
float_lse.h's host side against the oracle) and test_float_lse_gpu.py (float_lse.h's device side against the oracle).

A float function's domain can be enumerated: a sweep is a range of consecutive float BIT PATTERNS [lo, lo + count), cut into bands of
at most 2^26 arguments (256 MB of result bits, about a second of oracle time each).  For negative floats ascending bit patterns are
descending values.

NaN and the infinities are left out everywhere: the reference's behaviour there (casts of out-of-range floats to integers) is not
relied on anywhere in the library — a log-likelihood that is not finite never reaches these functions."""
import struct

import numpy as np

BAND = 1 << 26


def f2b(x):
    """bit pattern of the float nearest to x"""
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bands(lo, hi_incl, name):
    """[lo, hi_incl] (bit patterns) in bands of at most 2^26: (id, first pattern, count)"""
    out = []; n = hi_incl - lo + 1
    for k, off in enumerate(range(0, n, BAND)):
        out.append(("%s[%d]" % (name, k), lo + off, min(BAND, n - off)))
    return out


# fastexp, fasterexp and the pair term fastlog(1 + fastexp(p)): every float from -2^-27 to -8.0 — all of [LOG_THRESH = ln 0.001 = -6.9, 0)
# with margin for the double-to-float cast —, the floats of smaller magnitude down to -2^-28, where the result is one constant
# (fastexp: 0x3f800080), and the two zeros.
EXP_LO, EXP_HI = 0xB2000000, 0xC1000000            # -2^-27, -8.0
CONST_LO, CONST_HI = 0xB1800000, 0xB2000000        # -2^-28 .. -2^-27, both ends included (2^23 + 1 patterns)
EXP_BANDS = bands(EXP_LO, EXP_HI, "sweep") + [("const", CONST_LO, CONST_HI - CONST_LO + 1), ("-0.0", 0x80000000, 1), ("+0.0", 0, 1)]
assert sum(c for _, _, c in EXP_BANDS[:4]) == 251658241 and len(EXP_BANDS) == 7
# fastlog: every float of [1, 0x1.001p+1] — every mantissa, hence every denominator of its division, and the values above 2 that
# 1 + fastexp(p) reaches (the largest is 0x1.0000cp+1).
LOG_BANDS = bands(0x3F800000, 0x40000800, "sweep")
# fasterlog: every float of [2^-10, 2^16): a sum of float terms that each passed the threshold (2^-10 < term <= 1) lies there.
FASTERLOG_BANDS = bands(0x3A800000, 0x47800000 - 1, "sweep")
# the two divisions: every float denominator of [3.80, 4.90] (4.84252568f - z, z in [0, 1]) and of [0.84, 1.36] (0.3520887068f + mx, mx
# in [0.5, 1)), one float beyond the decimal ends
DIV_BANDS = {"div_pow2": (f2b(3.80) - 1, f2b(4.90) + 1), "div_log": (f2b(0.84) - 1, f2b(1.36) + 1)}
DIV_NUM = {"div_pow2": np.float32(27.7280233), "div_log": np.float32(1.72587999)}

SWEEPS = ([("fastexp",) + b for b in EXP_BANDS] + [("fasterexp",) + b for b in EXP_BANDS] + [("lse2_term",) + b for b in EXP_BANDS]
          + [("fastlog",) + b for b in LOG_BANDS] + [("fasterlog",) + b for b in FASTERLOG_BANDS]
          + [(k, "all", lo, hi - lo + 1) for k, (lo, hi) in DIV_BANDS.items()])
SWEEP_IDS = ["%s-%s" % (s[0], s[1]) for s in SWEEPS]
FASTEXP_CONST = 0x3F800080


def first_bad(lo, got, want):
    """the first few (argument bits, got, want) of a mismatch, in hex"""
    bad = np.flatnonzero(got != want)
    return ["(%#010x: got %#010x, want %#010x)" % (lo + i, got[i], want[i]) for i in bad[:8]], bad.size


# ------------------------------------------------------------------------------ the double wrapper fast_log_sum_exp(a, b)
LOG_THRESH = float(np.log(0.001))
IMPOSSIBLE = -1000000000.0             # HS_IMPOSSIBLE (hipstr_amd/csrc/layout.h)


def _around(x):
    """x and one double ulp either side"""
    x = np.asarray(x, np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def lse2_pairs():
    """About 10^6 (a, b) pairs; every one is also used swapped.  With hi = 0 the difference lo - hi is lo itself, exactly: that is how
    a chosen double `diff` reaches the threshold test (strict: diff == LOG_THRESH takes the float path) and the double-to-float cast."""
    rng = np.random.default_rng(20261019)
    lo = [_around([LOG_THRESH])]                                                            # the threshold and one double ulp either side
    f = -rng.uniform(2.0 ** -27, 8.0, 100_000).astype(np.float32)
    f = np.concatenate([f, np.float32([LOG_THRESH]), np.nextafter(np.float32(LOG_THRESH), np.float32([-10, 0]))])
    mid = 0.5 * (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64))    # exact: between adjacent floats
    lo.append(_around(mid))                                                                 # ties-to-even in the cast, and either side
    lo.append(np.array([0.0, -0.0]))
    lo = np.concatenate(lo); hi = np.zeros_like(lo)
    a = [lo, lo, lo]; b = [hi, -hi, hi]                                                       # hi = +0.0 and -0.0
    a[2] = np.where(lo == 0, -lo, lo)                                                        # (+0, -0) against (-0, +0) ...
    # |hi| from 10^-3 to 10^5, both signs, the difference on either side of the threshold
    h = np.exp(rng.uniform(np.log(1e-3), np.log(1e5), 200_000)) * rng.choice([-1.0, 1.0], 200_000)
    a.append(h + rng.uniform(-7.5, 0.0, h.size)); b.append(h)
    # the threshold approached at magnitude: lo = fl(hi + LOG_THRESH) lands within an ulp of hi of it, on either side
    h2 = np.exp(rng.uniform(np.log(1e-3), np.log(1e5), 50_000)) * rng.choice([-1.0, 1.0], 50_000)
    a.append(h2 + LOG_THRESH); b.append(h2)
    # a == b over the same magnitudes, and the library's "impossible" value with both arguments equal
    e = np.concatenate([h[:50_000], [IMPOSSIBLE, 2 * IMPOSSIBLE, 0.0, -0.0, 1e-3, -1e5]])
    a.append(e); b.append(e.copy())
    return np.concatenate(a), np.concatenate(b)


# ------------------------------------------------------------------------------ fast_log_sum_exp(vector)
ROW_SIZES = (1, 2, 63, 64, 65, 300, 4096)


def lse_rows():
    """(rows, groups): rows of 1, 2, 63, 64, 65, 300 and 4096 values that straddle the threshold (max - 9 .. max, LOG_THRESH = -6.9) at
    several magnitudes, all-equal rows, rows with a value exactly LOG_THRESH below the maximum (strict test: dropped) and one double
    ulp either side; every row also reversed and shuffled.  groups[g] = indices of rows that hold the same values in another order."""
    rng = np.random.default_rng(20261020)
    base = []
    for n in ROW_SIZES:
        for mag in (0.0, -3.25, -731.5, 1e5, IMPOSSIBLE):
            v = mag - rng.uniform(0.0, 9.0, n); v[rng.integers(n)] = mag
            base.append(v)
            base.append(np.full(n, mag - rng.uniform(0, 50)))                      # all equal
        base.append(np.concatenate([[0.0], _around([LOG_THRESH]), -rng.uniform(0.0, 9.0, n)]))
    rows, groups = [], []
    for v in base:
        g = [len(rows)]; rows.append(v)
        if len(v) > 1:
            g += [len(rows), len(rows) + 1]; rows += [v[::-1].copy(), rng.permutation(v)]
        groups.append(g)
    return rows, groups
