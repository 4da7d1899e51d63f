"""GPU: hipstr_record_fields at the end of the resident genotype() chain.  tests/flow_chain.py's driver takes the twelve loci of its cases
through genotype() as one batch on the device backend and leaves the final posteriors launched; then the record's calls of INTEGRATION.md
§2a follow — hipstr_post_assign(HIPSTR_ASSIGN_VCF), hipstr_hmm_trace_resident, hipstr_assign_trace_stats_dev, hipstr_record_fields — and the
result is held against hipstr_record_fields_host on the same counts and the fetched MAP pairs: integers identical, doubles within the bound
of tests/test_record_gpu.py."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
import record_cases as rc
from test_record_host import assert_fields

pytestmark = pytest.mark.gpu


def test_record_fields_after_the_chain(hmm, oracle):
    names = list(fc.CASES)
    states = [fc.State(fc.Inputs(n), oracle) for n in names]
    be = fc.DeviceBackend(hmm)
    td = None
    try:
        k, pooled, seeds = fc.genotype_pass(states, be, oracle, None)          # genotype(): the final posteriors are launched on be.pd
        n_samp = int(k.samp_off[-1])
        asg = capi.run_assign(hmm, be.pd, seeds, pool_index=k.pool_index, pool_off=k.pool_off, rule=capi.ASSIGN_VCF, n_reads=k.n, n_samp=n_samp)
        assert asg["rc"] == 0
        h2r = capi.hap_aln_info(hmm, "hipstr_", pooled.ptr)
        td = capi.run_trace_resident(hmm, pooled.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, flags=0)
        # the STR block's option of every haplotype, the variants' length differences, the regions
        h2a = np.concatenate([s.options()[:, 1] for s in states]).astype(np.int32)
        n_variants = np.array([len(s.blocks[1][2]) for s in states], np.int32)
        bp = np.concatenate([[len(o) - len(s.blocks[1][2][0]) for o in s.blocks[1][2]] for s in states]).astype(np.int32)
        start = np.array([s.blocks[1][0] for s in states], np.int32); stop = np.array([s.blocks[1][1] for s in states], np.int32)
        n_stutter, n_flank_indel, _ = capi.assign_trace_stats_dev(hmm, be.pb, asg["read_req"], td, asg["best_hap"], h2a, bp, n_variants, start, stop)
        counts = dict(n_aligned=asg["n_aligned"], n_snp=asg["n_snp"], n_stutter=n_stutter, n_flank_indel=n_flank_indel, uniq_one=asg["uniq_one"],
                      uniq_two=asg["uniq_two"], rv_uniq_one=asg["rv_uniq_one"], rv_uniq_two=asg["rv_uniq_two"])
        got = capi.run_record_fields(hmm, be.pb, n_variants, h2a, counts, pd=be.pd)
        assert capi.record_last(hmm)["lanes"] == n_samp
        # the MAP pairs, fetched, for the host form
        A = np.array([s.A for s in states], np.int64)
        post = np.zeros(max(int((k.n_samples.astype(np.int64) * A * A).sum()), 1)); tot = np.zeros(n_samp); gt = np.zeros(2 * n_samp, np.int32); lt = np.zeros(len(states))
        assert hmm.hipstr_post_fetch(be.pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p),
                                     lt.ctypes.data_as(capi._f64p)) == 0, hmm.hipstr_last_error().decode()
        want = capi.run_record_fields(hmm, be.pb, n_variants, h2a, counts, map_gt=gt)
        assert_fields(got, want, exact_doubles=False)
        # the chain's samples have reads and heterozygous calls: the stage did something
        assert np.sum(got["status"] == rc.PASS) > n_samp // 2 and np.sum(got["ab"] != rc.NOT_APPLICABLE) >= 10 and got["dp"].sum() == asg["n_aligned"][got["status"] == rc.PASS].sum()
        assert np.array_equal(got["an"], [2 * int(np.sum(got["status"][k.samp_off[l]:k.samp_off[l + 1]] == rc.PASS)) for l in range(len(states))])
    finally:
        if td is not None:
            td.close()
        be.close()
