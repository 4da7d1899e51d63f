"""GPU: hipstr_cigar_bp_diffs and hipstr_sample_histograms (hipstr_amd/csrc/record_reads.hip) against their host forms, which
tests/test_record_reads_host.py holds to the compiled reference: every output byte equal, on every case of tests/record_reads_cases.py —
the goldens' cases in one batch (reads and samples below and above the device's caps together, so the host twin works inside the call), the
named loci one at a time, batches whose samples cross the chunks of the offsets' scan, another skip value, and all of it again on
poisoned cache blocks.  Last, the two calls in a row as a record uses them (ALLREADS) and as learn_stutter_model does."""
import numpy as np
import pytest

from hipstr_amd import capi
import record_reads_cases as rc
from test_poison_gpu import poisoned, same_bits

pytestmark = pytest.mark.gpu


def both_cigars(hmm, loci):
    rq = capi.cigar_request(loci)
    dev = capi.run_cigar_bp_diffs(hmm, rq)
    last = capi.record_reads_last(hmm)
    host = capi.run_cigar_bp_diffs(hmm, rq, host=True)
    same_bits(dev, host, "hipstr_cigar_bp_diffs against its host form")
    return dev, last


def both_histograms(hmm, loci, skip=rc.SKIP):
    a = rc.histogram_arrays(loci)
    pb = rc.post_batch(capi, a)
    dev = capi.run_sample_histograms(hmm, pb, a["value"], skip)
    last = capi.record_reads_last(hmm)
    host = capi.run_sample_histograms(hmm, pb, a["value"], skip, host=True)
    same_bits(dev, host, "hipstr_sample_histograms against its host form")
    return dev, last


def test_cigars_of_the_goldens_in_one_batch(hmm):
    loci = rc.cigar_loci()
    (got, bp), last = both_cigars(hmm, loci)
    want_got, want_bp = rc.cigar_golden()
    assert np.array_equal(got, want_got) and np.array_equal(bp, want_bp)
    beyond = sum(1 for l in loci for r in l[3] if len(r[1]) > rc.CIGAR_DEVICE_RUNS)
    assert beyond == 2 and last["items"] == len(got) and last["host_items"] == beyond and last["bytes_up"] > 0 and last["bytes_down"] > 0


def test_cigars_one_locus_at_a_time_and_without_reads(hmm):
    for l in rc.cigar_unit_loci():
        both_cigars(hmm, [l])
    (got, _), last = both_cigars(hmm, [(5, 6, 0, []), (7, 8, 1, [])])
    assert len(got) == 0 and last["items"] == 0
    (got, _), last = both_cigars(hmm, [])
    assert len(got) == 0
    # more reads than one workgroup takes, none beyond the cap
    (got, _), last = both_cigars(hmm, rc.cigar_fuzz_loci(77, n_loci=60, max_reads=40))
    assert len(got) > 3 * 256 and last["host_items"] == 0 and 0 < got.sum() < len(got)


def test_cigar_refusals_launch_nothing(hmm):
    rq = capi.cigar_request([(102, 147, 2, [(100, [("M", 50)])])])
    rq["cigar_len"][0] = 0
    with pytest.raises(RuntimeError, match="non-positive length") as e:
        capi.run_cigar_bp_diffs(hmm, rq)
    assert np.all(e.value.raw[0] == 0xEE) and np.all(e.value.raw[1] == capi.UNTOUCHED)


def test_histograms_of_the_goldens_in_one_batch(hmm):
    loci = rc.histogram_loci()
    (po, hv, hc), last = both_histograms(hmm, loci)
    samples = [s for l in loci for s in l]
    beyond = sum(1 for s in samples if len(s) > rc.HISTOGRAM_DEVICE_READS)
    assert beyond == 3 and last["items"] == len(samples) and last["host_items"] == beyond
    assert sum(1 for s in samples if len(s) == rc.HISTOGRAM_DEVICE_READS) >= 1            # the largest sample the wavefront takes
    for s, (text, v) in enumerate(zip(rc.histogram_golden(), samples)):
        assert list(zip(hv[po[s]:po[s + 1]].tolist(), hc[po[s]:po[s + 1]].tolist())) == rc.pairs_of_string(text), s
    both_histograms(hmm, loci, skip=2)


def test_histograms_across_the_scans_chunks_and_alone(hmm):
    loci = rc.histogram_fuzz_loci(31, n_loci=130)
    (po, _, _), last = both_histograms(hmm, loci)
    assert len(po) - 1 > 3 * 256 and last["host_items"] == 0 and po[-1] > 0
    # exactly one chunk, one more, one less
    for n in (255, 256, 257, 512):
        both_histograms(hmm, [[[i % 5, rc.SKIP, -i] for i in range(n)]])
    for l in rc.histogram_unit_loci():
        both_histograms(hmm, [l])
    (po, hv, _), _ = both_histograms(hmm, [])
    assert list(po) == [0] and len(hv) == 0
    (po, hv, _), _ = both_histograms(hmm, [[[], []], []])
    assert list(po) == [0, 0, 0] and len(hv) == 0
    (po, hv, _), _ = both_histograms(hmm, [[[rc.SKIP], [rc.SKIP] * 70]])
    assert list(po) == [0, 0, 0]


def test_on_poisoned_cache_blocks(hmm):
    cig = capi.cigar_request(rc.cigar_loci())
    a = rc.histogram_arrays(rc.histogram_loci())
    pb = rc.post_batch(capi, a)
    def run():
        return capi.run_cigar_bp_diffs(hmm, cig), capi.run_sample_histograms(hmm, pb, a["value"], rc.SKIP)
    out = poisoned(hmm, run, "record reads")
    same_bits(out[0], (capi.run_cigar_bp_diffs(hmm, cig, host=True), capi.run_sample_histograms(hmm, pb, a["value"], rc.SKIP, host=True)), "poisoned against the host forms")


def test_allreads_and_the_ems_reads_in_a_row(hmm):
    """Twelve loci x 3 samples x 8 reads: the CIGARs' sizes, the reads without a size or a seed marked, the histograms — on the device and
    through the host forms — and learn_stutter_model's batch from the same sizes, trained."""
    rng = np.random.default_rng(12)
    loci = []
    for l in rc.cigar_fuzz_loci(12, n_loci=12, max_reads=0):
        rs, re_, pad, _ = l
        reads = []
        for _ in range(24):
            d = int(rng.integers(-2, 3)) * 2
            mid = [("I", d)] if d > 0 else [("D", -d)] if d < 0 else []
            reads.append((rs - pad - int(rng.integers(5, 30)), [("M", 40)] + mid + [("M", 120)]) if rng.random() < 0.9 else (rs + 3, [("M", 100)]))
        loci.append((rs, re_, pad, reads))
    rq = capi.cigar_request(loci)
    seed = np.where(rng.random(12 * 24) < 0.9, 5, -1)
    samples = rc.histogram_arrays([[[0] * 8] * 3] * 12)
    pb = rc.post_batch(capi, samples)
    out = []
    for host in (False, True):
        got, bp = capi.run_cigar_bp_diffs(hmm, rq, host=host)
        value = np.where((got == 1) & (seed >= 0), bp, rc.SKIP).astype(np.int32)
        out.append((got, bp, capi.run_sample_histograms(hmm, pb, value, rc.SKIP, host=host)))
    same_bits(out[0], out[1], "the chain on the device against the host forms")
    got, bp, (po, hv, hc) = out[0]
    assert 0 < hc.sum() == int(((got == 1) & (seed >= 0)).sum()) < len(got) and set(hv.tolist()) <= {-4, -2, 0, 2, 4} and len(set(hv.tolist())) == 5
    em = capi.em_batch_from_bp_diffs(hmm, pb, got, bp, rq["region_start"], rq["region_stop"], 10)
    same = rc.em_batch_restated(samples, got, bp, rq["region_start"], rq["region_stop"], 10)
    same_bits({k: em[k] for k in same}, same, "hipstr_em_batch_from_bp_diffs")
    assert not em["too_few"].any()
    trained, stutter, n_iter, ll = capi.run_em(hmm, "hipstr_", period=np.full(12, 2, np.int32), n_samples=samples["n_samples"], read_off=em["read_off"],
                                               sample_label=em["sample_label"], num_bps=em["num_bps"], log_p1=em["log_p1"], log_p2=em["log_p2"])[:4]
    assert len(trained) == 12 and np.all(np.isfinite(ll[np.asarray(trained) == 1]))
