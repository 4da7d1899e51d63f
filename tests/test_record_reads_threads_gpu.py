"""GPU: hipstr_record_alleles, hipstr_cigar_bp_diffs, hipstr_sample_histograms and hipstr_post_extract_vcf from eight host threads at once,
against the same calls made one after another.

tests/test_threads_gpu.py's protocol and mechanics (tests/thread_jobs.py): every job runs once on the main thread before a worker starts,
that result is checked against the call's host form (hipstr_post_extract_vcf: against hipstr_post_extract gathered in numpy), and every
threaded result must equal it bit for bit; two rounds, the jobs dealt to the workers and then in reverse order, the caches' free blocks poisoned before each; afterwards every block is back and a serial pass
takes nothing from the driver.  The jobs differ in size — the goldens' batches with their reads and samples beyond the device's caps,
single loci, batches of several hundred samples — so the threads hold blocks of different sizes from the shared caches at any moment."""
import pytest

from hipstr_amd import capi
import post_extract_vcf_cases as pc
import record_alleles_cases as ac
import record_reads_cases as rc
import thread_jobs as tj
from test_poison_gpu import same_bits
from test_threads_gpu import two_rounds

pytestmark = pytest.mark.gpu
W = tj.W


@pytest.fixture(autouse=True)
def not_stuck():
    assert not tj.STUCK, "an earlier test of this module left a job stuck: %s" % tj.STUCK


@pytest.fixture(scope="module")
def workers(hmm):
    hmm.hipstr_hmm_trim()
    w = tj.Workers(W)
    yield w
    w.close()


def cigar_job(hmm, loci, name):
    rq = capi.cigar_request(loci)
    run = lambda: capi.run_cigar_bp_diffs(hmm, rq)
    check = lambda got: same_bits(got, capi.run_cigar_bp_diffs(hmm, rq, host=True), name + " against the host form")
    return tj.Job(name, run, check)


def histogram_job(hmm, loci, name, skip=rc.SKIP):
    a = rc.histogram_arrays(loci)
    pb = rc.post_batch(capi, a)
    run = lambda: capi.run_sample_histograms(hmm, pb, a["value"], skip)
    check = lambda got: same_bits(got, capi.run_sample_histograms(hmm, pb, a["value"], skip, host=True), name + " against the host form")
    return tj.Job(name, run, check)


def alleles_job(hmm, cases, name):
    loci = [ac.locus_of(c) for c in cases]
    run = lambda: capi.run_record_alleles(hmm, loci)
    check = lambda got: same_bits(got, capi.run_record_alleles(hmm, loci, host=True), name + " against the host form")
    return tj.Job(name, run, check)


def vcf_job(hmm, seed, loci, name):
    keys = ("best_hap", "best_gt", "log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff", "gls", "pls", "phased_gls")
    pb, nv, h2a = pc.post_batch(capi, seed, loci)
    order = pc.orders(seed + 1, nv)
    run = lambda: {k: v for k, v in capi.run_post_extract_flat(hmm, pb, nv, h2a, order=order).items() if k in keys}
    def check(got):
        want = pc.permute_gt_outputs(capi.run_post_extract_flat(hmm, pb, nv, h2a), pb, nv, *order)
        same_bits(got, {k: want[k] for k in keys}, name + " against the gathered hipstr_post_extract")
    return tj.Job(name, run, check)


def test_record_reads_calls_from_eight_threads(hmm, workers):
    capi._record_reads_sigs(hmm); capi._record_alleles_sigs(hmm)   # bound before a worker starts
    jobs = [cigar_job(hmm, rc.cigar_loci(), "cigars/golden"), histogram_job(hmm, rc.histogram_loci(), "histograms/golden"),
            histogram_job(hmm, rc.histogram_loci(), "histograms/golden, skip 2", skip=2)]
    for t in range(W):
        jobs.append(cigar_job(hmm, rc.cigar_fuzz_loci(100 + t, n_loci=10 + 7 * t, max_reads=30), "cigars/%d" % t))
        jobs.append(histogram_job(hmm, rc.histogram_fuzz_loci(200 + t, n_loci=5 + 12 * t), "histograms/%d" % t))
        jobs.append(vcf_job(hmm, 300 + t, [(2 + t, 2, 3, False), (5 + 3 * t, 5, 4 + t, t % 2 == 1), (14, 6 + t, 2, False)], "post_extract_vcf/%d" % t))
        jobs.append(alleles_job(hmm, ac.random_cases(400 + t, 4 + 5 * t) + ([ac.beyond_cap_case()] if t % 3 == 0 else []), "record_alleles/%d" % t))
    jobs.append(alleles_job(hmm, ac.unit_cases(), "record_alleles/unit"))
    for i, l in enumerate(rc.histogram_unit_loci()):
        jobs.append(histogram_job(hmm, [l], "histograms/unit %d" % i))
    two_rounds(hmm, workers, jobs, "record reads")
