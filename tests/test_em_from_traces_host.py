"""CPU: hipstr_em_batch_from_traces (host only; include/hipstr_hmm.h) — the batch SeqStutterGenotyper::recompute_stutter_models hands to
EMStutterGenotyper::train (seq_stutter_genotyper.cpp:1555-1566) — against a numpy restatement of those lines (tests/em_trace_cases.py),
every refusal with the outputs untouched, and the declarations and exports of the new entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from hipstr_amd import capi
import em_trace_cases as etc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mixed_case():
    return etc.build([
        # strict spanning on both sides, seed < 0, no request, an empty sample in the middle, two reads on one request
        dict(period=2, runs=[[("in", 12), ("start", 14), ("stop", 16), ("in", 10)], [], [("seed", 12), ("noreq",), ("in", 14), ("share", 14)]]),
        dict(period=3, runs=[[], []]),                                              # an empty locus (its samples stay)
        dict(period=6, haploid=True, runs=[[("noreq",), ("seed", 3)], [("in", -4), ("in", 0), ("in", 18)]]),
        dict(period=1, runs=[[("start", 5), ("stop", 5)]]),                         # reads, but none enters
    ], seed=5)


def test_equals_the_numpy_restatement(hmm_host):
    c = _mixed_case()
    got = etc.host_batch(hmm_host, c)
    want = etc.restate(c)
    assert etc.same_batch(got, want), (got, want)
    assert list(got["read_off"]) == [0, 4, 4, 7, 7]
    assert list(got["num_bps"]) == [12, 10, 14, 14, -4, 0, 18] and list(got["sample_label"]) == [0, 0, 2, 2, 1, 1, 1]


def test_strict_spanning_and_missing_traces_one_by_one(hmm_host):
    for kind, enters in (("in", True), ("start", False), ("stop", False), ("seed", False)):
        c = etc.build([dict(period=2, runs=[[(kind, 9)]])])
        got = etc.host_batch(hmm_host, c)
        assert int(got["read_off"][1]) == (1 if enters else 0), kind
        assert etc.same_batch(got, etc.restate(c))
    c = etc.build([dict(period=2, runs=[[("noreq",)]])])
    assert int(etc.host_batch(hmm_host, c)["read_off"][1]) == 0
    # one past either bound spans
    c = etc.build([dict(period=2, runs=[[("in", 9)]])])
    t = dict(c.trace); t["aln_start"] = np.array([etc.BLK_START - 1], np.int32); t["aln_stop"] = np.array([etc.BLK_END + 1], np.int32)
    assert int(etc.host_batch(hmm_host, c, trace=t)["read_off"][1]) == 1


def test_empty_batch(hmm_host):
    c = etc.build([])
    got = etc.host_batch(hmm_host, c)
    assert list(got["read_off"]) == [0] and len(got["num_bps"]) == 0


def _untouched(e):
    o = e.value.outputs
    return (np.all(o["read_off"] == capi.UNTOUCHED) and np.all(o["sample_label"] == capi.UNTOUCHED) and np.all(o["num_bps"] == capi.UNTOUCHED)
            and np.all(np.isnan(o["log_p1"])) and np.all(np.isnan(o["log_p2"])))


def test_refusals_leave_the_outputs_untouched(hmm_host):
    base = [dict(period=2, runs=[[("in", 12), ("in", 10)], [("in", 14)]]), dict(period=2, runs=[[("in", 8)]])]
    c = etc.build(base)
    # read_req outside [-1, n_req)
    for bad in (c.n_req, -2):
        rr = c.read_req.copy(); rr[1] = bad
        with pytest.raises(RuntimeError, match=r"read_req outside \[-1, n_req\)") as e:
            capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), c.seed, rr, c.req_read, c.trace)
        assert _untouched(e)
    # a read whose request belongs to another locus
    rr = c.read_req.copy(); rr[0] = c.n_req - 1
    with pytest.raises(RuntimeError, match="request belongs to another locus") as e:
        capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), c.seed, rr, c.req_read, c.trace)
    assert _untouched(e)
    # pooled->n_loci differs
    p1 = etc.pooled(1, [etc.BLK_START], [etc.BLK_END], [2], [0, c.n_req])
    with pytest.raises(RuntimeError, match="pooled->n_loci differs") as e:
        capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(p1), c.seed, c.read_req, c.req_read, c.trace)
    assert _untouched(e)
    # requests that are not grouped by locus / outside the pooled reads
    q = c.req_read.copy(); q[0], q[-1] = q[-1], q[0]
    with pytest.raises(RuntimeError, match="grouped by locus") as e:
        capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), c.seed, c.read_req, q, c.trace)
    assert _untouched(e)
    q = c.req_read.copy(); q[-1] = c.n_req
    with pytest.raises(RuntimeError, match="outside the pooled reads") as e:
        capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), c.seed, c.read_req, q, c.trace)
    assert _untouched(e)
    # a trace without one of the four arrays
    for nm in ("aln_start", "aln_stop", "stutter_size", "str_seq_off"):
        t = dict(c.trace); t[nm] = None
        with pytest.raises(RuntimeError, match="trace output without") as e:
            capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), c.seed, c.read_req, c.req_read, t)
        assert _untouched(e)
    # null arguments
    for kw in (dict(seed=None), dict(read_req=None), dict(req_read=None), dict(bptr=None), dict(trace=None)):
        a = dict(bptr=C.pointer(c.pooled), seed=c.seed, read_req=c.read_req, req_read=c.req_read, trace=c.trace); a.update(kw)
        if kw.get("req_read", 0) is None:
            # (without req_read the wrapper passes n_req = 0: every read_req >= 0 is then out of range)
            with pytest.raises(RuntimeError, match="read_req outside") as e:
                capi.em_batch_from_traces(hmm_host, c.pb, **a)
        else:
            with pytest.raises(RuntimeError, match="null argument") as e:
                capi.em_batch_from_traces(hmm_host, c.pb, **a)
        assert _untouched(e)
    fn = hmm_host.hipstr_em_batch_from_traces
    assert fn(None, None, None, None, None, None, None, None) != 0 and b"null argument" in hmm_host.hipstr_last_error()


def test_read_without_str_data_is_refused_and_named(hmm_host):
    # reads 2 and 4 enter without STR data: the lowest is named; a NO_STR_DATA request nobody enters with is no error
    c = etc.build([dict(period=2, runs=[[("in", 12), ("in", 10)], [("nostr",), ("in", 14), ("nostr",)]])])
    with pytest.raises(RuntimeError, match=r"read 2 enters the EM but its request has no STR data") as e:
        etc.host_batch(hmm_host, c)
    assert _untouched(e)
    seed = c.seed.copy(); seed[[2, 4]] = -1
    got = capi.em_batch_from_traces(hmm_host, c.pb, C.pointer(c.pooled), seed, c.read_req, c.req_read, c.trace)
    assert list(got["num_bps"]) == [12, 10, 14]
    t = dict(c.trace); t["aln_stop"] = c.trace["aln_stop"].copy(); t["aln_stop"][[2, 4]] = etc.BLK_END       # they no longer span
    assert list(etc.host_batch(hmm_host, c, trace=t)["num_bps"]) == [12, 10, 14]


def test_declared_and_exported(hmm_host):
    pub = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read()
    dbg = open(os.path.join(ROOT, "include", "hipstr_hmm_debug.h")).read()
    for nm in ("hipstr_em_batch_from_traces", "hipstr_em_train_dev"):
        assert hasattr(hmm_host, nm) and ("int %s(" % nm) in pub and ("int %s(" % nm) not in dbg
    for nm in ("hipstr_debug_em_input_plan", "hipstr_debug_em_input_fetch"):
        assert hasattr(hmm_host, nm) and ("int %s(" % nm) in dbg and ("int %s(" % nm) not in pub
    # the resident entry point refuses null arguments without a device
    assert hmm_host.hipstr_em_train_dev(None, None, None, None) != 0 and b"null argument" in hmm_host.hipstr_last_error()
