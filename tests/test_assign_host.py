"""CPU: hipstr_assign_trace_stats (host only: the read counts of a VCF record that need the tracebacks, seq_stutter_genotyper.cpp:1124-1127
and :1150-1154) on hand-made trace outputs, hipstr_post_assign's refusal of NULL arguments without a device, and the launch decisions
of the assignment stage (post_layout.h) on either side of their thresholds."""
import ctypes as C

import numpy as np
import pytest

from hipstr_amd import capi

NO_STR = -100000            # HIPSTR_NO_STR_DATA
NO_ML = capi.NO_ML_BP


def _pb(n_alleles, n_samples, read_off, sample_label):
    n = len(sample_label)
    return capi.PostBatch(n_alleles, n_samples, read_off, sample_label, np.zeros(n), np.zeros(n), np.ones(n, np.int32), None)


def _trace(stutter, ins, dele, start, stop):
    return dict(stutter_size=stutter, flank_ins=ins, flank_del=dele, aln_start=start, aln_stop=stop)


def test_stutter_and_flank_indel_counts(hmm_host):
    # one locus, 2 samples, 8 reads; requests: 0 no STR data, 1 stutter 0, 2 stutter -4, 3 stutter +2, 4 ins only, 5 del only, 6 both
    tr = _trace([NO_STR, 0, -4, 2, 0, 0, 0], [0, 0, 0, 0, 3, 0, 1], [0, 0, 0, 0, 0, 2, 1], [100] * 7, [200] * 7)
    pb = _pb([3], [2], [0, 9], [0, 0, 0, 0, 0, 1, 1, 1, 1])
    read_req = [0, 1, 2, 3, -1, 4, 5, 6, 2]          # read 4 skipped; reads 2 and 8 share request 2 across the samples
    ns, nf, ml = capi.run_assign_trace_stats(hmm_host, pb, read_req, tr, [0, 1, 2, 0, -1, 1, 1, 2, 2], [0, 1, 1], [0, -8], [2], [150], [160])
    assert list(ns) == [2, 1] and list(nf) == [0, 3]
    # all span [146, 164]: the bp difference of the haplotype's variant plus the stutter; no STR data counts as 0
    assert list(ml) == [0, -8, -8 - 4, 0 + 2, NO_ML, -8, -8, -8, -8 - 4]


@pytest.mark.parametrize("region_start,bound", [(0, 0), (3, 0), (4, 0), (5, 1), (150, 146)])
def test_span_rule(hmm_host, region_start, bound):
    """ml_bp only when aln_start < (region_start > 4 ? region_start - 4 : 0) and aln_stop > region_stop + 4 (:1152-1154)."""
    region_stop = region_start + 20
    starts = [bound - 1, bound, bound + 1, bound - 1, bound - 1, bound - 1]
    stops = [region_stop + 5, region_stop + 5, region_stop + 5, region_stop + 4, region_stop + 3, region_stop + 6]
    tr = _trace([1] * 6, [0] * 6, [0] * 6, starts, stops)
    pb = _pb([1], [1], [0, 6], [0] * 6)
    ns, nf, ml = capi.run_assign_trace_stats(hmm_host, pb, list(range(6)), tr, [0] * 6, [0], [7], [1], [region_start], [region_stop])
    assert list(ml) == [8, NO_ML, NO_ML, NO_ML, NO_ML, 8]        # (with a bound of 0 no start but -1 lies below it)
    assert list(ns) == [6] and list(nf) == [0]


def test_two_loci_offsets(hmm_host):
    """hap_to_allele is indexed by locus (sum A_l), allele_bp_diff by variant (sum V_l), the samples run on across the loci."""
    pb = _pb([2, 3], [1, 2], [0, 2, 5], [0, 0, 0, 1, 1])
    tr = _trace([0, 3, NO_STR], [0, 1, 0], [0, 0, 0], [10, 10, 10], [500, 500, 500])
    ns, nf, ml = capi.run_assign_trace_stats(hmm_host, pb, [0, 1, 2, 1, -1], tr, [1, 0, 2, 1, -1], [0, 1, 0, 1, 2], [0, 4, 0, -4, 12],
                                             [2, 3], [100, 100], [200, 200])
    assert list(ns) == [1, 0, 1] and list(nf) == [1, 0, 1]
    assert list(ml) == [4, 0 + 3, 12, -4 + 3, NO_ML]


def test_bad_arguments_refused(hmm_host):
    pb = _pb([2], [1], [0, 2], [0, 0])
    tr = _trace([0, 0], [0, 0], [0, 0], [1, 1], [9, 9])
    good = dict(read_req=[0, 1], best_hap=[0, 1], hap_to_allele=[0, 1], allele_bp_diff=[0, 4], n_variants=[2], region_start=[3], region_stop=[5])
    def run(pb=pb, tr=tr, **kw):
        a = dict(good); a.update(kw)
        return capi.run_assign_trace_stats(hmm_host, pb, a["read_req"], tr, a["best_hap"], a["hap_to_allele"], a["allele_bp_diff"], a["n_variants"],
                                           a["region_start"], a["region_stop"])
    run()
    for kw, word in ((dict(best_hap=[0, 2]), "best_hap"), (dict(best_hap=[-1, 0]), "best_hap"), (dict(hap_to_allele=[0, 2]), "hap_to_allele"),
                     (dict(n_variants=[0]), "inconsistent"), (dict(pb=_pb([2], [1], [0, 2], [0, 1])), "sample_label"),
                     (dict(tr=dict(tr, aln_stop=None)), "aln_stop")):
        with pytest.raises(RuntimeError, match=word):
            run(**kw)
    run(read_req=[-1, 0], best_hap=[-1, 1])          # a skipped read's best_hap is not looked at
    # NULL pointers
    fn = hmm_host.hipstr_assign_trace_stats
    z = np.zeros(4, np.int32); p = z.ctypes.data_as(capi._i32p)
    t = capi.HipstrTraceOut()
    for nm in ("stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop"):
        setattr(t, nm, p)
    args = [pb.ptr, p, C.byref(t)] + [p] * 9
    for i in range(len(args)):
        bad = list(args); bad[i] = None
        assert fn(*bad) != 0 and b"null" in hmm_host.hipstr_last_error()


def test_post_assign_null_arguments_fail_without_a_device(hmm_host):
    capi._sig(hmm_host.hipstr_post_assign, C.c_int, [C.c_void_p, C.POINTER(capi.HipstrAssignRequest), C.POINTER(capi.HipstrAssignOut)])
    rq = capi.HipstrAssignRequest(); o = capi.HipstrAssignOut()
    for a in ((None, None, None), (None, C.byref(rq), C.byref(o))):
        assert hmm_host.hipstr_post_assign(*a) != 0
        assert b"null" in hmm_host.hipstr_last_error()


def test_launch_decisions(hmm_host):
    """hs_assign_waves_per_unit / hs_assign_workgroups / hs_assign_table_slots (post_layout.h) on either side of HS_ASSIGN_WAVE_READS = 256 and
    HS_ASSIGN_DIRECT_MAX = 4096."""
    capi._sig(hmm_host.hipstr_debug_assign_plan, C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)])
    def plan(*a):
        out = (C.c_int64 * 4)()
        assert hmm_host.hipstr_debug_assign_plan(*a, out) == 0
        return list(out)
    assert plan(256, 9, 4096, 500) == [1, 3, 4096, 0]            # one wavefront per unit, four units per workgroup; a direct table
    assert plan(257, 9, 4097, 500) == [4, 9, 1024, 1]            # a workgroup per unit; hashed: the power of two from twice the reads
    assert plan(0, 0, 0, 0)[:2] == [1, 0]
    assert plan(5000, 1, 10 ** 6, 512)[2:] == [1024, 1] and plan(5000, 1, 10 ** 6, 513)[2:] == [2048, 1] and plan(1, 1, 10 ** 6, 1)[2:] == [64, 1]
