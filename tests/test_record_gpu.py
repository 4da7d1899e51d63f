"""GPU: hipstr_bias_pvalues and hipstr_record_fields (include/hipstr_hmm.h; hipstr_amd/csrc/record.hip) against their host forms and against
the compiled reference routines (tests/golden/record_pvalues.npz).

The bound: integers identical; doubles exact where the reference's value is exact (1, 0.0, 1.01) or infinite (a p-value that underflowed
to 0: log10 gives -inf on both sides), otherwise within 1e-9 absolute — the project's bound for values that pass through the host's libm
(tests/test_genotype_flow.py).  The device uses correctly rounded exp / log / log10 (cr_math.h) where the host form uses
glibc's; the number of values that are not bit-identical and their largest distance in ulps are printed as a record, not asserted
(tools/record_fields_timing.py writes them to profiles/record_fields_parity.txt): glibc's log10 is not correctly rounded for about one
argument in seven."""
import numpy as np
import pytest

from hipstr_amd import capi
import record_cases as rc
from test_record_host import assert_fields, common_refusals, counts_of

pytestmark = pytest.mark.gpu
BOUND = 1e-9


@pytest.fixture(scope="module")
def quadruples(hmm):
    """The whole golden once on the device and once through the host form."""
    u1, u2, r1, r2, ab, fs = rc.all_quadruples()
    dev = capi.bias_pvalues(hmm, u1, u2, r1, r2)
    last = capi.record_last(hmm)
    host = capi.bias_pvalues(hmm, u1, u2, r1, r2, host=True)
    return dict(q=(u1, u2, r1, r2), gold=(ab, fs), dev=dev, host=host, last=last)


def close(dev, want, what):
    """The bound of this module; returns (values not bit-identical, largest distance in ulps)."""
    assert not np.any(np.isnan(dev)), what
    # (1 only comes from an empty total, 1.01 from "not applicable"; a 0.0 that comes out of the clamp min(1.0, p) is a computed value)
    exact = np.isinf(want) | (want == 1.0) | (want == rc.NOT_APPLICABLE)
    assert np.array_equal(dev[exact].view(np.uint64), want[exact].view(np.uint64)), what
    assert np.all(np.isfinite(dev[~exact])), what
    assert np.all(np.abs(dev[~exact] - want[~exact]) <= BOUND), (what, float(np.max(np.abs(dev[~exact] - want[~exact]))))
    differ = dev.view(np.uint64) != want.view(np.uint64)
    return int(differ.sum()), int(rc.ulps(dev[differ], want[differ]).max()) if differ.any() else 0


def test_pvalues_against_the_host_form_and_the_golden(quadruples):
    (ab_d, fs_d), (ab_h, fs_h), (ab_g, fs_g) = quadruples["dev"], quadruples["host"], quadruples["gold"]
    u1, u2, r1, r2 = quadruples["q"]
    n_ab, ulp_ab = close(ab_d, ab_h, "ab against the host form")
    n_fs, ulp_fs = close(fs_d, fs_h, "fs against the host form")
    print("record parity: ab %d of %d not bit-identical (largest %d ulp), fs %d of %d (largest %d ulp)" % (n_ab, len(ab_d), ulp_ab, n_fs, len(fs_d), ulp_fs))
    has_ab, has_fs = ~np.isnan(ab_g), ~np.isnan(fs_g)
    close(ab_d[has_ab], ab_g[has_ab], "ab against the golden")
    close(fs_d[has_fs], fs_g[has_fs], "fs against the golden")
    # the exact cases of compute_allele_bias, and the clamp at n = 2k + 1
    tot = u1.astype(np.int64) + u2
    equal = (u1 == u2) & (tot > 0)
    assert np.all(ab_d[tot == 0] == 1.0) and np.all(ab_d[equal] == 0.0) and not np.any(np.signbit(ab_d[equal])) and equal.sum() > 20
    assert ab_d[(u1 == 4) & (u2 == 5)][0] == 0.0          # bdtr(4, 9, .5) = 0x1.0000000000001p-1: only the clamp gives log10(1)
    # a p-value that underflows is -inf on both sides, nothing else is infinite
    assert np.array_equal(np.isinf(ab_d), np.isinf(ab_h)) and np.array_equal(np.isinf(fs_d), np.isinf(fs_h)) and np.isinf(ab_h).sum() > 0
    # beyond the table the host twin computed the pair inside the call: the host form's bits
    beyond = tot > rc.TABLE_READS
    assert quadruples["last"]["lanes"] == len(u1) and quadruples["last"]["host_lanes"] == int(beyond.sum()) > 0
    assert np.array_equal(ab_d[beyond].view(np.uint64), ab_h[beyond].view(np.uint64)) and np.array_equal(fs_d[beyond].view(np.uint64), fs_h[beyond].view(np.uint64))
    assert quadruples["last"]["bytes_up"] >= 16 * len(u1) and quadruples["last"]["bytes_down"] >= 16 * len(u1)


def test_pvalues_refusals_and_empty(hmm):
    for kw, word in ((dict(uniq_one=[-1]), "negative"), (dict(rv_uniq_one=[4]), "rv_uniq exceeds uniq"), (dict(uniq_two=None), "null argument"),
                     (dict(n=-1), "must not be negative")):
        a = dict(uniq_one=[3], uniq_two=[3], rv_uniq_one=[1], rv_uniq_two=[1]); a.update(kw)
        with pytest.raises(RuntimeError, match=word):
            capi.bias_pvalues(hmm, **a)
    ab, fs = capi.bias_pvalues(hmm, [], [], [], [])
    assert len(ab) == 0 and len(fs) == 0
    # an odd size, more than one workgroup, the last one partly empty
    u1 = np.arange(131, dtype=np.int32) % 40; u2 = (np.arange(131, dtype=np.int32) * 7) % 33
    dev = capi.bias_pvalues(hmm, u1, u2, u1 // 2, u2 // 3); host = capi.bias_pvalues(hmm, u1, u2, u1 // 2, u2 // 3, host=True)
    close(dev[0], host[0], "ab"); close(dev[1], host[1], "fs")


def forced_post_batch(b):
    """A posterior batch whose likelihoods force the MAP pairs of a fields batch: two reads per sample with reads, the first phased to
    strand one and 50 log units in favour of hap_a, the second phased to strand two and in favour of hap_b; a sample without reads has
    no read at all (its MAP pair is the run's own choice)."""
    read_off, label, p1, p2, ll = [0], [], [], [], []
    i = 0
    for l in range(b.n_loci):
        A = int(b.n_alleles[l])
        for s in range(int(b.n_samples[l])):
            if b.n_aligned[i] > 0:
                for which, h in enumerate(b.map_gt[i]):
                    row = np.full(A, -50.0); row[int(h)] = 0.0
                    ll.append(row); label.append(s)
                    p1.append(0.0 if which == 0 else -1000.0); p2.append(-1000.0 if which == 0 else 0.0)
            i += 1
        read_off.append(len(label))
    return capi.PostBatch(b.n_alleles, b.n_samples, read_off, label, p1, p2, np.ones(len(label), np.int32), np.concatenate(ll) if ll else np.zeros(0),
                          haploid=b.haploid)


class Run(object):
    """hipstr_post_upload + hipstr_post_launch of a fields batch, its MAP pairs fetched."""

    def __init__(self, hmm, b):
        self.hmm, self.b = hmm, b
        self.pb = forced_post_batch(b)
        self.pd = hmm.hipstr_post_upload(self.pb.ptr, None)
        assert self.pd, hmm.hipstr_last_error().decode()
        assert hmm.hipstr_post_launch(self.pd, None) == 0, hmm.hipstr_last_error().decode()
        S = b.n_samp
        post = np.zeros(max(int(self.pb.post_off[-1]), 1)); tot = np.zeros(S); gt = np.zeros(2 * S, np.int32); lt = np.zeros(b.n_loci)
        assert hmm.hipstr_post_fetch(self.pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p),
                                     lt.ctypes.data_as(capi._f64p)) == 0, hmm.hipstr_last_error().decode()
        self.map_gt = gt.reshape(-1, 2)

    def fields(self, host=False, **kw):
        b = self.b
        a = dict(n_variants=b.n_variants, hap_to_allele=b.hap_to_allele, counts=counts_of(b), sample_reported=b.reported, sample_masked=b.masked,
                 max_flank_indel_frac=b.frac)
        a.update(kw)
        if host:
            a.setdefault("map_gt", self.map_gt)
            return capi.run_record_fields(self.hmm, self.pb, **a)
        return capi.run_record_fields(self.hmm, self.pb, pd=self.pd, **a)

    def close(self):
        self.hmm.hipstr_post_free(self.pd)


@pytest.mark.parametrize("seed", rc.FIELD_SEEDS)
def test_fields_on_resident_posteriors(hmm, seed):
    b = rc.fields_batch(seed)
    r = Run(hmm, b)
    try:
        with_reads = b.n_aligned > 0
        assert np.array_equal(r.map_gt[with_reads], b.map_gt[with_reads])      # the likelihoods forced the pairs (a sample without reads gets the run's own)
        got = r.fields(); want = r.fields(host=True)
        assert_fields(got, want, exact_doubles=False, what=seed)
        computed = got["ab"] != rc.NOT_APPLICABLE
        assert computed.sum() >= 1 and capi.record_last(hmm)["lanes"] == b.n_samp
        assert np.all(got["ab"][computed & (b.uniq_one == b.uniq_two) & (b.uniq_one > 0)] == 0.0)
        # the restated loops on the same pairs
        b.map_gt = r.map_gt
        pv = lambda *q: tuple(x[0] for x in capi.bias_pvalues(hmm, *[[v] for v in q], host=True))
        assert_fields(got, rc.expect_fields(b, pv), exact_doubles=False, what=seed)
        # without the optional arrays
        got = r.fields(sample_reported=None, sample_masked=None); want = r.fields(host=True, sample_reported=None, sample_masked=None)
        assert_fields(got, want, exact_doubles=False, what=seed)
    finally:
        r.close()


def test_a_sample_beyond_the_table_takes_the_host_twin(hmm):
    b = rc.fields_batch(2)
    b.reported[:] = 1; b.masked[:] = 0; b.n_flank_indel[:] = 0
    r = Run(hmm, b)
    try:
        first = r.fields()
        computed = np.flatnonzero(first["ab"] != rc.NOT_APPLICABLE)
        assert len(computed) >= 3
        s = int(computed[1])
        b.uniq_one[s], b.uniq_two[s], b.rv_uniq_one[s], b.rv_uniq_two[s] = 2600, 2500, 1200, 1300          # 5100 reads: beyond the table
        got = r.fields(); want = r.fields(host=True)
        last = capi.record_last(hmm)
        assert last["lanes"] == b.n_samp and last["host_lanes"] == 1
        assert_fields(got, want, exact_doubles=False)
        assert got["ab"][s] == want["ab"][s] and got["fs"][s] == want["fs"][s] and got["dab"][s] == 5100 and np.isfinite(got["fs"][s]) and got["fs"][s] < 0
        others = np.setdiff1d(computed, [s])
        assert np.array_equal(got["ab"][others].view(np.uint64), first["ab"][others].view(np.uint64))        # the rest stayed on the device
    finally:
        r.close()


def test_more_than_one_wavefront_per_locus(hmm):
    """130 samples in one locus (three wavefronts, the last with two lanes) beside a locus of one sample: the per-locus sums cross
    workgroups."""
    rng = np.random.RandomState(7)
    b = rc.Batch()
    b.n_loci = 2; b.n_samples = np.array([130, 1], np.int32); b.n_alleles = np.array([4, 2], np.int32); b.haploid = np.zeros(2, np.uint8)
    b.n_variants = np.array([3, 2], np.int32); b.hap_to_allele = np.array([0, 1, 2, 1, 0, 1], np.int32)
    n = b.n_samp = 131
    b.map_gt = np.stack([rng.randint(0, 4, n), rng.randint(0, 4, n)], 1).astype(np.int32); b.map_gt[130] = (1, 0)
    b.reported = (rng.rand(n) < 0.9).astype(np.uint8); b.masked = (rng.rand(n) < 0.1).astype(np.uint8)
    b.n_aligned = (20 * rng.randint(1, 30, n)).astype(np.int32); b.n_aligned[::17] = 0
    b.n_flank_indel = (3 * b.n_aligned // 20 + rng.randint(-1, 2, n)).clip(0).astype(np.int32)
    b.n_snp = rng.randint(0, 20, n).astype(np.int32); b.n_stutter = rng.randint(0, 20, n).astype(np.int32)
    b.uniq_one = rng.randint(0, 300, n).astype(np.int32); b.uniq_two = rng.randint(0, 300, n).astype(np.int32)
    b.rv_uniq_one = (b.uniq_one * rng.rand(n)).astype(np.int32); b.rv_uniq_two = (b.uniq_two * rng.rand(n)).astype(np.int32)
    b.frac = 0.0
    r = Run(hmm, b)
    try:
        got = r.fields(); want = r.fields(host=True)
        assert_fields(got, want, exact_doubles=False)
        # every one of the three wavefronts adds to the locus' sums
        assert all(np.any(want["status"][a:b] == rc.PASS) for a, b in ((0, 64), (64, 128), (128, 130))) and want["n_filt"][0] > 0 and want["n_skip"][0] > 0
    finally:
        r.close()


def test_refusals(hmm):
    def run(b, **kw):
        r = Run(hmm, b)
        try:
            return r.fields(**kw)
        finally:
            r.close()
    common_refusals(run)
    # (a haploid run's MAP pairs are homozygous — its heterozygous prior is -DBL_MAX/2 — so the device never meets the reference's assertion
    # on pairs of its own; the host form, which takes any pairs, is refused in tests/test_record_host.py.  The same holds for the kernel's
    # other two refusals, a pair outside [-1, A) and a sample with reads and without a pair: NO GPU test reaches the kernel's three error
    # branches or its "nothing written" rule after them; they restate hipstr_record::fields, whose refusals the host tests cover.)
    b = rc.fields_batch(1)
    r = Run(hmm, b)
    try:
        pd = hmm.hipstr_post_upload(r.pb.ptr, None)          # not launched
        assert pd
        try:
            with pytest.raises(RuntimeError, match="call hipstr_post_launch first"):
                capi.run_record_fields(hmm, r.pb, b.n_variants, b.hap_to_allele, counts_of(b), pd=pd)
        finally:
            hmm.hipstr_post_free(pd)
    finally:
        r.close()
    # (nor a sample without a MAP pair: a run gives every sample one, the first diplotype where it has no reads)


def test_empty_batch(hmm):
    pb = capi.PostBatch([], [], [0], [], [], [], [], [])
    got = capi.run_record_fields(hmm, pb, [], [], {nm: [] for nm in capi.RECORD_COUNTS})
    assert all(len(v) == 0 for v in got.values())
    pb = capi.PostBatch([2, 3], [0, 0], [0, 0, 0], [], [], [], [], np.zeros(0))
    got = capi.run_record_fields(hmm, pb, [2, 1], [0, 1, 0, 0, 0], {nm: [] for nm in capi.RECORD_COUNTS})
    assert list(got["allele_count"]) == [0, 0, 0] and list(got["an"]) == [0, 0] and list(got["dp"]) == [0, 0]
    assert capi.record_last(hmm)["lanes"] == 0
