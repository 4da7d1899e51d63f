"""GPU: the flank sweeps' fused column pass (band_sweep_coop: column 0 initialised, one top-down pass per column, the last pass without
its rows) at the smallest shapes its pass structure can go wrong at, bit for bit against the oracle — one-shot and two resident passes
on one upload, as tests/test_routes_gpu.py compares; the route of every batch asserted from the launch plan.

Per batch, loci whose reads carry caller-given seeds (hipstr_hmm_process_reads_seeded / hipstr_hmm_upload_seeded):
  * read sides of 1, 2 and 3 columns on either side (seeds 1, 2, 3 and len-4, len-3, len-2) next to a seed in the read's middle: the
    reads of a locus side share a wavefront (trailing flank: 64 / npad reads per wavefront for groups of <= 32 alleles; leading flank:
    reads are the lanes), so lanes run past their own read end, and a side of one column stores right after the initialisation.
    A side of 0 columns does not exist: a seed must leave a base on either side (prep refuses 0 and len-1, HapAligner.cpp:316);
  * flank rowsets of 1, 2, 16, 17, 60 and 61 rows after the block's first row (the right flank, one base longer: trailing flank of the
    left side, leading flank of the right side; 61 rows are two rounds of bands, the boundary between them handed over through memory)
    — the short shape takes rowsets up to its limit only;
  * allele groups of 1, 3, 8, 9 and 33 members: the select path, the 8-lane emission table with rows s and s + 8, the full table, a
    wavefront per read;
through trail_default + lead_default, trail_short, and trail_latency + lead_latency."""
import numpy as np
import pytest

from hipstr_amd import capi
import route_cases as rc
import util

pytestmark = pytest.mark.gpu
FILL = -3.25
AUTO = -2                      # HIPSTR_SEED_AUTO: the library computes the seed
DEPTHS = (1, 2, 16, 17, 60, 61)
GROUPS = (1, 3, 8, 9, 33)


def _locus(b, rng, seeds, rf, n_alleles):
    """One locus: 16-base left flank, `n_alleles` STR alleles, right flank of rf + 1 bases (a rowset of rf rows after its first), seven
    whole-haplotype reads with seeds 1, 2, 3, the middle, len-4, len-3, len-2."""
    L, R = rc._seq(rng, 16), rc._seq(rng, rf + 1)
    strs = ["CAG" * k for k in range(5, 5 + n_alleles)]
    ref = L + strs[0] + R
    n = len(ref)
    reads = [(ref, "".join(chr(ord("5") + (7 * j + 3 * i) % 40) for j in range(n)), 0, True) for i in range(7)]
    util.simple_locus(L, strs, R, 3, reads, batch=b)
    seeds += [1, 2, 3, n // 2, n - 4, n - 3, n - 2]


def _batch(tag, depths, group_depth, pad):
    rng, b, seeds = rc._rng(tag), capi.Batch(), []
    for d in depths:
        _locus(b, rng, seeds, d, 3)
    for g in GROUPS:
        _locus(b, rng, seeds, group_depth, g)
    for _ in range(pad):                     # single-read loci (two leading and two trailing items each) push the item counts past a limit
        rc.add_locus(b, rng, strs=("CAG" * 6,))
        seeds.append(AUTO)
    return b.finalize(), np.array(seeds, np.int32)


def _check(hmm, oracle, b, seed_in, what):
    want, ws = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL, seed_in=seed_in)
    got, gs = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL, seed_in=seed_in)
    given = seed_in != AUTO
    assert np.array_equal(ws[given], seed_in[given]), what + ": the oracle did not take the given seeds"
    assert np.array_equal(gs, ws), what + ": seeds differ"
    assert np.array_equal(got == FILL, want == FILL), what + ": untouched entries differ"
    assert np.array_equal(got, want), "%s: max|diff| %g" % (what, np.nanmax(np.abs(got - want)))
    dev = hmm.hipstr_hmm_upload_seeded(b.ptr, capi._ptr(seed_in, capi._i32p))
    assert dev, hmm.hipstr_last_error()
    try:
        n_reads, n_out, _ = capi.batch_dims(b.ptr)
        for rep in range(2):
            assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error()
            p = np.full(max(n_out, 1), FILL); s = np.full(max(n_reads, 1), -7, np.int32)
            assert hmm.hipstr_hmm_fetch(dev, p.ctypes.data_as(capi._f64p), s.ctypes.data_as(capi._i32p)) == 0
            assert np.array_equal(s[:n_reads], ws), "%s resident pass %d: seeds differ" % (what, rep)
            assert np.array_equal(p[:n_out], want), "%s resident pass %d differs" % (what, rep)
    finally:
        hmm.hipstr_hmm_free(dev)


@pytest.fixture(scope="module")
def lim(hmm):
    return rc.lim_of(hmm)


# name -> (depths, depth of the group loci, padding loci, environment, expected lead route, expected trail route)
def _shapes(lim):
    short = tuple(d for d in DEPTHS if d <= lim["HS_SHORT_TRAIL_ROWS"])
    pad = lim["HS_LAT_ITEMS"] // 2 + 1
    return {
        "default": (DEPTHS, 61, pad, {}, "lead_default", "trail_default"),
        "short": (short, 17, pad, {}, "lead_default", "trail_short"),
        "latency": (DEPTHS, 61, 0, {"HIPSTR_FLANK_SYSTOLIC": "0"}, "lead_latency", "trail_latency"),
    }


@pytest.mark.parametrize("shape", ["default", "short", "latency"])
def test_fused_sweep_against_the_oracle(hmm, oracle, lim, shape):
    depths, gdepth, pad, env, lead, trail = _shapes(lim)[shape]
    assert shape != "short" or set(depths) == {1, 2, 16, 17}
    b, seed_in = _batch("fused_" + shape, depths, gdepth, pad)
    with rc.environ(env):
        plan = capi.launch_plan(hmm, b.ptr)
        assert [c["lead"]["route"] for c in plan["chunks"]] == [lead] and [c["trail"]["route"] for c in plan["chunks"]] == [trail], plan["chunks"]
        assert plan["max_rows"] - 1 == max(max(depths), gdepth, 15)
        _check(hmm, oracle, b, seed_in, shape)
