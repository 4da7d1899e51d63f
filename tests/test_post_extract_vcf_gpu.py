"""GPU: hipstr_post_extract_vcf — hipstr_post_extract's outputs in the record's allele order — against hipstr_post_extract's own output
gathered through the numpy restatement of write_vcf_record's index rules (tests/post_extract_vcf_cases.py).  Every value is a copy, so
doubles are compared as bit patterns.  Diploid and haploid loci of V = 1, 2, 5 and a V = 33 locus (more entries than a workgroup has
threads), every combination of the three calc_* flags, an identity order (hipstr_post_extract's bytes), BPDIFFS / AC, the refusals, and
poisoned cache blocks."""
import itertools

import numpy as np
import pytest

from hipstr_amd import capi
import post_extract_vcf_cases as pc
from test_poison_gpu import poisoned, same_bits

pytestmark = pytest.mark.gpu

#        A   V  S  haploid
LOCI = [(1, 1, 3, False), (2, 2, 4, False), (10, 5, 6, False), (1, 1, 2, True), (4, 2, 3, True), (5, 5, 5, True), (66, 33, 2, False), (6, 5, 0, False)]
KEYS = ("best_hap", "best_gt", "log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff", "gls", "pls", "phased_gls")


@pytest.fixture(scope="module")
def case(hmm):
    pb, nv, h2a = pc.post_batch(capi, 5, LOCI)
    n2o, o2n = pc.orders(3, nv)
    assert not np.array_equal(n2o, pc.orders(0, nv, identity=True)[0])
    at = np.concatenate([[0], np.cumsum(nv)])
    assert all(not np.array_equal(n2o[at[l]:at[l + 1]], np.arange(nv[l])) for l in (2, 5, 6)), "a locus of five variants keeps its order"
    return pb, nv, h2a, n2o, o2n


def strip(d):
    return {k: d[k] for k in KEYS}


@pytest.mark.parametrize("flags", list(itertools.product((True, False), repeat=3)))
def test_every_layout_equals_the_restated_gather(hmm, case, flags):
    pb, nv, h2a, n2o, o2n = case
    kw = dict(calc_gls=flags[0], calc_pls=flags[1], calc_phased_gls=flags[2])
    plain = capi.run_post_extract_flat(hmm, pb, nv, h2a, **kw)
    got = capi.run_post_extract_flat(hmm, pb, nv, h2a, order=(n2o, o2n), **kw)
    want = pc.permute_gt_outputs(plain, pb, nv, n2o, o2n)
    same_bits(strip(got), strip(want), "hipstr_post_extract_vcf %s" % (flags,))
    if all(flags):
        assert not np.array_equal(got["gls"], plain["gls"]) and not np.array_equal(got["best_gt"], plain["best_gt"])
        assert np.array_equal(np.sort(got["gls"]), np.sort(plain["gls"])) and np.all(got["best_gt"] >= 0)
    # what was not asked for is not written
    for k, f in zip(("gls", "pls", "phased_gls"), flags):
        if not f:
            assert np.all(np.isnan(got[k])) if got[k].dtype == np.float64 else np.all(got[k] == capi.UNTOUCHED), k


def test_identity_order_gives_post_extracts_bytes(hmm, case):
    pb, nv, h2a, _, _ = case
    ident = pc.orders(0, nv, identity=True)
    plain = capi.run_post_extract_flat(hmm, pb, nv, h2a)
    same_bits(strip(capi.run_post_extract_flat(hmm, pb, nv, h2a, order=ident)), strip(plain), "identity order")
    # and hipstr_post_extract itself is what it was: the wrapper of the suite's other tests gives the same arrays
    listed = capi.run_gt_extract(hmm, "hipstr_", pb, nv, h2a)
    for k in ("gls", "pls", "phased_gls"):
        same_bits(np.concatenate(listed[k]), plain[k], k)
    same_bits({k: listed[k] for k in KEYS[:7]}, {k: plain[k] for k in KEYS[:7]}, "per sample")


def test_bp_diffs_and_allele_counts_in_the_new_order(hmm, case):
    pb, nv, h2a, n2o, o2n = case
    tot = int(nv.sum())
    at = np.repeat(np.concatenate([[0], np.cumsum(nv)])[:-1], nv)
    bp = (np.arange(tot) * 3 - 7).astype(np.int32); ac = (np.arange(tot) % 11).astype(np.int32)
    got = capi.run_post_extract_flat(hmm, pb, nv, h2a, order=(n2o, o2n), allele_bp_diff=bp, allele_count=ac)
    assert np.array_equal(got["bp_diffs"], bp[at + n2o]) and np.array_equal(got["ac"], ac[at + n2o])
    first = np.concatenate([[0], np.cumsum(nv)])[:-1]
    assert np.array_equal(got["ac"][first], ac[first])                                  # REFAC stays allele_count[0]
    only = capi.run_post_extract_flat(hmm, pb, nv, h2a, order=(n2o, o2n), allele_count=ac, calc_gls=False, calc_pls=False, calc_phased_gls=False)
    assert np.array_equal(only["ac"], ac[at + n2o]) and np.all(only["bp_diffs"] == capi.UNTOUCHED)
    # a batch without samples still gathers them
    pb0, nv0, h2a0 = pc.post_batch(capi, 1, [(4, 3, 0, False)])
    got0 = capi.run_post_extract_flat(hmm, pb0, nv0, h2a0, order=([0, 2, 1], [0, 2, 1]), allele_bp_diff=[0, 4, -2], allele_count=[5, 6, 7])
    assert list(got0["bp_diffs"]) == [0, -2, 4] and list(got0["ac"]) == [5, 7, 6]


def test_refusals_write_nothing(hmm, case):
    pb, nv, h2a, n2o, o2n = case
    def refused(msg, order, **kw):
        with pytest.raises(RuntimeError, match=msg) as e:
            capi.run_post_extract_flat(hmm, pb, nv, h2a, order=order, **kw)
        for k, v in e.value.raw.items():
            assert np.all(np.isnan(v)) if v.dtype == np.float64 else np.all(v == capi.UNTOUCHED), k
    five = int(np.cumsum(nv)[1])                                   # where the V = 5 locus begins
    bad = n2o.copy(); bad[five], bad[five + 1] = bad[five + 1], bad[five]
    inv = o2n.copy(); inv[five], inv[five + 1] = inv[five + 1], inv[five]
    refused("new_to_old\\[0\\] must be 0", (bad, inv))
    bad = n2o.copy(); bad[five + 2] = bad[five + 3]
    refused("not a permutation", (bad, o2n))
    bad = n2o.copy(); bad[five + 2] = 5
    refused("not a permutation", (bad, o2n))
    bad = n2o.copy(); bad[five + 2] = -1
    refused("not a permutation", (bad, o2n))
    inv = o2n.copy(); inv[five + 1], inv[five + 2] = inv[five + 2], inv[five + 1]
    refused("its inverse", (n2o, inv))
    refused("null argument", (n2o, o2n), null=("new_to_old",))
    refused("null argument", (n2o, o2n), null=("old_to_new",))
    refused("requested output array missing", (n2o, o2n), allele_count=np.zeros(int(nv.sum()), np.int32), null=("ac",))
    refused("requested output array missing", (n2o, o2n), allele_bp_diff=np.zeros(int(nv.sum()), np.int32), null=("bp_diffs",))


def test_on_poisoned_cache_blocks(hmm, case):
    pb, nv, h2a, n2o, o2n = case
    plain = capi.run_post_extract_flat(hmm, pb, nv, h2a)
    want = strip(pc.permute_gt_outputs(plain, pb, nv, n2o, o2n))
    out = poisoned(hmm, lambda: strip(capi.run_post_extract_flat(hmm, pb, nv, h2a, order=(n2o, o2n))), "post_extract_vcf")
    same_bits(out[0], want, "poisoned against the gather")
