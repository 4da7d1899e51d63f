"""CPU: what the trace cache (hipstr_trace_cache_*, include/hipstr_hmm.h) decides without a device — the refusals of its creation, the
re-keying and the listing of an empty cache — and the decisions of hipstr_amd/csrc/trace_cache_layout.h through
hipstr_debug_trace_cache_plan: the compaction rule on both sides of each threshold, the launch arithmetic of the gather at the sizes where
the scan's carry crosses a wavefront."""
import ctypes as C

import numpy as np
import pytest

from hipstr_amd import capi


def why(lib):
    return lib.hipstr_last_error().decode()


@pytest.mark.parametrize("pool_off, n_alleles, n_loci, message", [
    ([1, 3], [2], None, "pool_off must start at 0"),
    ([0, 5, 3], [2, 2], None, "pool_off must be ascending"),
    ([0, 5], [0], None, "allele count out of range"),
    ([0, 5], [9999], None, "allele count out of range"),
    ([0, 5], [2], -1, "negative locus count"),
    (None, [2], None, "null argument"),
    ([0, 5], None, 1, "null argument"),
])
def test_creation_refuses(hmm_host, pool_off, n_alleles, n_loci, message):
    with pytest.raises(RuntimeError) as e:
        capi.TraceCache(hmm_host, pool_off, n_alleles, n_loci=n_loci)
    assert message in str(e.value)


def test_an_empty_cache_lists_nothing_and_remaps(hmm_host):
    tc = capi.TraceCache(hmm_host, [0, 4, 9], [3, 2])
    er, ea = tc.entries()
    assert len(er) == 0 and len(ea) == 0
    st = tc.stats()
    assert st == dict(n_hits=0, n_misses=0, n_inserted=0, n_segments=0, n_live=0, n_dead=0)
    tc.remap([4, 1], [0, 2, -1, 0, -1])                # a permutation with a hole, a dropped haplotype: nothing to re-key
    tc.remap([2, 2], [1, 0, -1, -1, 0])                # (the old counts are now 4 and 1: five entries)
    tc.clear(); tc.clear([1, 0]); tc.compact()
    assert tc.stats()["n_segments"] == 0
    tc.close()


@pytest.mark.parametrize("new_n, mapping, message", [
    ([0, 2], [0, 1, 2, 0, 1], "allele count out of range"),
    ([3, 2], [0, 1, 3, 0, 1], "allele_mapping entry out of range at locus 0"),
    ([3, 2], [0, 1, -2, 0, 1], "allele_mapping entry out of range at locus 0"),
    ([3, 2], [0, 1, 2, 1, 1], "two old columns mapped to one new column at locus 1"),
])
def test_remap_refuses_what_hipstr_rm_remap_refuses(hmm_host, new_n, mapping, message):
    tc = capi.TraceCache(hmm_host, [0, 4, 9], [3, 2])
    with pytest.raises(RuntimeError) as e:
        tc.remap(new_n, mapping)
    assert message in str(e.value)
    tc.remap([3, 2], [2, 1, 0, 1, 0])                  # the counts are unchanged by a refusal: five entries still fit
    with pytest.raises(RuntimeError):
        tc.remap([3, 2], None)
    tc.close()


def test_entries_with_a_small_cap_returns_3(hmm_host):
    """An empty cache needs no room; a negative cap is too small for it too.  (A filled cache: tests/test_trace_cache_gpu.py.)"""
    tc = capi.TraceCache(hmm_host, [0, 4], [3])
    n = np.full(1, -5, np.int32)
    assert hmm_host.hipstr_trace_cache_entries(tc.h, 0, n.ctypes.data_as(capi._i32p), None, None) == 0 and n[0] == 0
    assert hmm_host.hipstr_trace_cache_entries(tc.h, -1, n.ctypes.data_as(capi._i32p), None, None) == 3 and n[0] == 0
    assert "cap is too small" in why(hmm_host)
    assert hmm_host.hipstr_trace_cache_entries(tc.h, 4, None, None, None) == 1 and "null argument" in why(hmm_host)
    assert hmm_host.hipstr_trace_cache_entries(None, 4, n.ctypes.data_as(capi._i32p), None, None) == 1
    tc.close()


def test_null_handles_are_refused(hmm_host):
    capi._trace_cache_sigs(hmm_host)
    st = capi.HipstrTraceCacheStats()
    assert hmm_host.hipstr_trace_cache_remap(None, None, None) == 1 and "null argument" in why(hmm_host)
    assert hmm_host.hipstr_trace_cache_clear(None, None) == 1
    assert hmm_host.hipstr_trace_cache_compact(None) == 1
    assert hmm_host.hipstr_trace_cache_stats(None, C.byref(st)) == 1
    h = C.c_void_p(0xdead)
    assert hmm_host.hipstr_trace_cache_view(None, C.byref(h)) == 1 and not h.value
    h = C.c_void_p(0xdead)
    assert hmm_host.hipstr_trace_cache_round(None, None, 0, None, None, None, None, None, C.byref(h), None) == 1 and not h.value
    hmm_host.hipstr_trace_cache_free(None)


def test_gather_refusals_that_need_no_device(hmm_host):
    capi._trace_cache_sigs(hmm_host)
    for kw, message in ((dict(n_src=-1), "negative count"), (dict(n_out=-1), "negative count")):
        with pytest.raises(RuntimeError) as e:
            capi.trace_dev_gather(hmm_host, [], [], [], **kw)
        assert message in str(e.value)
    with pytest.raises(RuntimeError) as e:
        capi.trace_dev_gather(hmm_host, [None], [0], [0])
    assert "null source 0" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        capi.trace_dev_gather(hmm_host, [], [0], [0])
    assert "out_src out of range at record 0" in str(e.value)
    assert hmm_host.hipstr_trace_dev_gather(0, None, 0, None, None, None) == 1 and "null argument" in why(hmm_host)


# ------------------------------------------------------------------ trace_cache_layout.h
def test_compaction_rule_on_both_sides_of_each_threshold(hmm_host):
    """hs_tc_should_compact: more than HS_TC_MAX_SEGMENTS segments, or at least HS_TC_COMPACT_MIN_DEAD dead records that outnumber the live."""
    p = capi.trace_cache_plan(hmm_host)
    D, S = p["min_dead"], p["max_segments"]
    assert (D, S) == (4096, 16)
    rule = lambda live, dead, segs: capi.trace_cache_plan(hmm_host, n_live=live, n_dead=dead, n_segments=segs)["compact"]
    # the segment count alone
    assert rule(1000, 0, S) == 0 and rule(1000, 0, S + 1) == 1
    assert rule(0, 0, 0) == 0 and rule(0, 0, 1) == 0
    # the dead share: strictly more dead than live ...
    assert rule(D, D, 1) == 0 and rule(D - 1, D, 1) == 1 and rule(D + 1, D, 1) == 0
    assert rule(10 * D, 10 * D + 1, 2) == 1 and rule(10 * D, 10 * D, 2) == 0
    # ... and at least D of them (a small cache is never compacted for its share)
    assert rule(0, D - 1, 1) == 0 and rule(0, D, 1) == 1
    assert rule(5, D - 1, S) == 0 and rule(5, D - 1, S + 1) == 1


@pytest.mark.parametrize("n", [0, 1, 32, 33, 63, 64, 65, 130, 256, 257])
def test_gather_launch_arithmetic(hmm_host, n):
    p = capi.trace_cache_plan(hmm_host, n_out=n)
    assert (p["len_threads"], p["wave"], p["totals_bytes"]) == (256, 64, 64)
    assert p["len_workgroups"] == -(-n // 256)
    assert p["scan_steps"] == -(-n // 64) and p["scan_steps_flank"] == -(-2 * n // 64)      # the flank pool's carry crosses at half the records
    assert p["copy_workgroups"] == max(n, 1)           # the empty gather still writes the seven leading zeros
    assert p["pieces"] == 8 * n and p["pool_fits"] == 1


def test_pool_limit_is_int32_max(hmm_host):
    assert capi.trace_cache_plan(hmm_host, n_out=2 ** 31 - 1)["pool_fits"] == 1
    assert capi.trace_cache_plan(hmm_host, n_out=2 ** 31)["pool_fits"] == 0
    with pytest.raises(RuntimeError):
        capi.trace_cache_plan(hmm_host, n_out=-1)


# ------------------------------------------------------------------ the reference's cache on the flow fixtures, restated
def test_restated_misses_of_the_flow_batch(hmm_host, oracle):
    """tests/flow_chain.py's twelve loci as one batch on the host backend, the reference's trace_cache_ restated as the driver's dictionary
    (tests/flow_chain_cache.py).  The first pass makes four trace calls of 1826 requests.  A cache that takes every record misses
    1826 / 32 / 0 / 0 of them: 1858 tracebacks where the uncached chain computes 7304.  With locus_takes as the chain sets it — a locus that
    is DONE takes nothing — the handful of keys a DONE locus misses is missed again in every later call; still far below half.
    tests/test_flow_chain_cache_gpu.py holds hipstr_trace_cache_round to the second column, call by call."""
    import flow_chain as fc
    import flow_chain_cache as fcc
    be = fcc.CountingHostBackend(hmm_host, oracle)
    fc.run(list(fc.CASES), be, oracle, None)
    first = be.calls[:4]
    assert [n for n, _, _ in first] == [1826] * 4
    assert [e for _, _, e in first] == [1826, 32, 0, 0]
    assert all(m >= e for _, m, e in be.calls) and [m for _, m, _ in first][:2] == [1826, 32]
    assert 2 * sum(m for _, m, _ in first) < 7304
    assert 2 * sum(m for _, m, _ in be.calls) < sum(n for n, _, _ in be.calls)
