"""GPU: every exit of a stage call gives every block back.  The stage calls take their device and pinned blocks from the context's caches
(hipstr_amd/csrc/api_internal.h: ResultBlocks, ChunkBlocks, ScratchBufs, HostArena); other host threads draw from the same caches, so a
block must be back, behind the stream, whichever way the call leaves.  hipstr_debug_cache_stats counts the blocks that are out: out[2] for
the device cache, out[6] for the pinned one.  With the input handles alive both numbers are read, the call is made, and they are read
again: (a) after a normal return, (b) after the return-3 path — a capacity one too small, found after the results were fetched — and (c)
after a refusal found only after blocks were taken and work was queued (the check kernel's verdict on a decreasing str_seq_off; a read
that enters the EM without STR data).  The cases are the smallest ones of the stages' own test modules; what the calls compute is held to
its yardsticks there."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from hipstr_amd import capi
import em_trace_cases as etc
import flank_cases as fc
import hapgen_cases as hc
import pool_cases as pc
import test_assign_gpu as ta
import test_census_gpu as tc
import test_trace_assemble_gpu as tta
from em_cases import em_case
from nw_cases import nw_pairs

pytestmark = pytest.mark.gpu


def in_use(hmm):
    o = (C.c_int64 * 12)()
    assert hmm.hipstr_debug_cache_stats(o) == 0
    return int(o[2]), int(o[6])


@contextmanager
def balanced(hmm, what):
    """The blocks out of the device and the pinned cache are the same after the body as before it, however the body ends."""
    before = in_use(hmm)
    try:
        yield
    finally:
        after = in_use(hmm)
        assert after == before, "%s: blocks in use (device, pinned) %r before, %r after" % (what, before, after)


@contextmanager
def launched(hmm, pb, launch=True):
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd, hmm.hipstr_last_error().decode()
    try:
        if launch:
            assert hmm.hipstr_post_launch(pd, None) == 0
        yield pd
    finally:
        hmm.hipstr_post_free(pd)


@contextmanager
def handle(td):
    try:
        yield td
    finally:
        td.close()


def test_post_assign(hmm):
    """Two loci, three samples, eleven reads in six pools: the request list has three entries."""
    row = lambda A, h: [(-1.0 if k == h else -30.0) - 0.01 * k for k in range(A)]
    pb, _ = ta.make_pb([(3, [[(-0.5, -0.5, row(3, 0))] * 3, [(-0.2, -0.9, row(3, 2))] * 2]), (2, [[(-0.5, -0.5, row(2, 1))] * 6])])
    n = int(pb.a["read_off"][-1]); ns = int(pb.samp_off[-1])
    seed = np.full(n, 3, np.int32); seed[1] = -1
    pool = np.array([0, 1, 0, 1, 2] + [0, 1, 2, 0, 1, 2], np.int32); pool_off = np.array([0, 3, 6], np.int32)
    with launched(hmm, pb) as pd:
        kw = dict(pool_index=pool, pool_off=pool_off, rule=capi.ASSIGN_RETRACE, n_reads=n, n_samp=ns)
        with balanced(hmm, "hipstr_post_assign"):
            full = capi.run_assign(hmm, pd, seed, **kw)
        assert full["rc"] == 0 and full["n_req"] >= 2
        with balanced(hmm, "hipstr_post_assign without a request list"):
            assert capi.run_assign(hmm, pd, seed, n_reads=n, n_samp=ns)["rc"] == 0
        with balanced(hmm, "hipstr_post_assign, cap_req one too small"):
            small = capi.run_assign(hmm, pd, seed, cap_req=full["n_req"] - 1, **kw)
        assert small["rc"] == 3 and small["n_req"] == full["n_req"]


def test_post_census_and_post_census_dev(hmm):
    c = tc.content_case()                       # three loci, six requests, two candidates of eight characters each
    n_samp = int(c.pb.samp_off[-1])
    with launched(hmm, c.pb) as pd:
        host = lambda **kw: capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=n_samp, **kw)
        with balanced(hmm, "hipstr_post_census"):
            want = host()
        need = int(want["cand_off"][-1]); chars = sum(len(s) for x in want["cand"] for s in x)
        assert want["rc"] == 0 and need == 2 and chars == 16
        with balanced(hmm, "hipstr_post_census, cap_cand one too small"):
            assert host(cap_cand=need - 1)["rc"] == 3
        with balanced(hmm, "hipstr_post_census, cap_chars one too small"):
            assert host(cap_cand=need, cap_chars=chars - 1)["rc"] == 3
        with handle(capi.trace_dev_from_host(hmm, c.trace, len(c.req_read))) as td:
            dev = lambda td=td, **kw: capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, None, hap_to_allele=c.h2a, n_samp=n_samp, td=td, **kw)
            with balanced(hmm, "hipstr_post_census_dev"):
                got = dev()
            assert got["rc"] == 0 and got["cand"] == want["cand"]
            with balanced(hmm, "hipstr_post_census_dev, cap_cand one too small"):
                assert dev(cap_cand=need - 1)["rc"] == 3
            with balanced(hmm, "hipstr_post_census_dev, cap_chars one too small"):
                assert dev(cap_cand=need, cap_chars=chars - 1)["rc"] == 3
        # the check kernel's verdict: blocks were taken, the arena was sent and a kernel has run when the call refuses
        t = dict(c.trace); t["str_seq_off"] = c.trace["str_seq_off"].copy(); t["str_seq_off"][2] = 3
        with handle(capi.trace_dev_from_host(hmm, t, len(c.req_read))) as td:
            with balanced(hmm, "hipstr_post_census_dev on a decreasing str_seq_off"):
                with pytest.raises(RuntimeError, match="str_seq_off must not decrease"):
                    dev(td=td)
        # ... and the one found in the results: a spanning request without STR data
        t = dict(c.trace); t["stutter_size"] = [-4, tc.NO_STR, -4, 4, -4, 4]
        with handle(capi.trace_dev_from_host(hmm, t, len(c.req_read))) as td:
            with balanced(hmm, "hipstr_post_census_dev on a spanning request without STR data"):
                with pytest.raises(RuntimeError, match="a spanning request without STR data"):
                    dev(td=td)


def test_assign_trace_stats_dev(hmm):
    """Two loci, three samples, seven reads on five requests."""
    pb = capi.PostBatch([2, 3], [2, 1], [0, 4, 7], [0, 0, 1, 1, 0, 0, 0], np.zeros(7), np.zeros(7), np.ones(7, np.int32), None)
    nq = 5
    tr = dict(ll=np.zeros(nq), max_index=np.zeros(nq, np.int32), stutter_size=[-4, 0, tc.NO_STR, 2, 0], flank_ins=[0, 1, 0, 0, 0], flank_del=[0, 0, 2, 0, 0],
              aln_start=[-1, 0, 2, 0, 1], aln_stop=[40, 24, 40, 30, 25])
    read_req = [0, 1, -1, 2, 3, 4, 3]; best = [0, 1, -1, 0, 2, 0, 1]
    with handle(capi.trace_dev_from_host(hmm, tr, nq)) as td:
        with balanced(hmm, "hipstr_assign_trace_stats_dev"):
            st = capi.assign_trace_stats_dev(hmm, pb, read_req, td, best, [0, 1, 0, 1, 2], [-2, 0, 0, 3, 6], [2, 3], [4, 5], [24, 25])
        assert st[0].sum() > 0 and st[1].sum() > 0


def test_flank_assemble_dev(hmm):
    c = fc.build(fc.unit_loci()[:3])            # five samples: no reads, short strings, a SNP kept and a SNP pruned
    with launched(hmm, c.pb, launch=False) as pd, handle(capi.trace_dev_from_host(hmm, c.trace, c.n_req)) as td:
        run = lambda **kw: capi.run_flank(hmm, td=td, pd=pd, **fc.args(c, **kw))
        full = run()
        assert full["rc"] == 0
        caps = dict(full["need"])
        with balanced(hmm, "hipstr_flank_assemble_dev"):
            assert run(caps=caps)["rc"] == 0
        with balanced(hmm, "hipstr_flank_assemble_dev, cap_opts one too small"):
            assert run(caps=dict(caps, opts=caps["opts"] - 1))["rc"] == 3


def test_em_train_dev(hmm):
    c = etc.build([dict(period=2, runs=[[("in", 12), ("in", 10)], [("in", 14)]]), dict(period=2, runs=[[("in", 8), ("noreq",)]])])
    wide = etc.build([dict(period=6, runs=[[("in", s) for s in (0, 10000, 0, 0, 6)], [("in", 0), ("in", 6)]])], seed=4)       # em_prepare on the fetched arrays
    nostr = etc.build([dict(period=2, runs=[[("in", 12), ("nostr",)], [("in", 14)]])])
    for case, what, ok in ((c, "", True), (wide, " through the host's preparation", True), (nostr, " on a read without STR data", False)):
        with launched(hmm, case.pb, launch=False) as pd, handle(capi.trace_dev_from_host(hmm, case.trace, case.n_req)) as td:
            train = lambda: capi.em_train_dev(hmm, pd, case.n_loci, C.pointer(case.pooled), case.seed, case.read_req, case.req_read, td)
            with balanced(hmm, "hipstr_em_train_dev" + what):
                if ok:
                    assert len(train()[0]) == case.n_loci
                else:
                    # the select kernel's verdict: five kernels have run and the counts are home when the call refuses
                    with pytest.raises(RuntimeError, match="enters the EM but its request has no STR data"):
                        train()


def test_pool_reads(hmm):
    rng = np.random.default_rng(3)
    b = pc.batch_of(pc.count_loci(rng))         # loci of 0, 1, 50 identical and 50 distinct reads
    with balanced(hmm, "hipstr_pool_reads"):
        got = capi.run_pool(hmm, b.ptr)
    assert capi.pool_last(hmm)["device_loci"] == 6 and int(got["n_pools"][:6].sum()) == 52


def test_hapgen(hmm):
    loci = hc.unit_status()                     # eight loci of two reads
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    with balanced(hmm, "hipstr_hapgen"):
        capi.run_hapgen(hmm, b.ptr, rq)
    assert capi.hapgen_last(hmm)["device_loci"] == len(loci)


def test_trace_seeded(hmm, oracle):
    sb, rr, aa, h2r = tta._small(oracle, seed=12, reads=12, alleles=4)
    _, seeds = capi.run_align(oracle, "oracle_", sb.ptr)
    with balanced(hmm, "hipstr_hmm_trace_seeded"):
        got = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, req_seed=[int(seeds[r]) for r in rr])
    assert len(got) == len(rr) > 0
    with balanced(hmm, "hipstr_hmm_trace_ex, records assembled on the device"):
        capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=capi.TRACE_ASSEMBLE_DEVICE)


def test_nw_align(hmm):
    pairs = nw_pairs(5, n=6)
    with balanced(hmm, "hipstr_nw_align"):
        assert len(capi.run_nw(hmm, "hipstr_", pairs)) == len(pairs)


def test_em_train(hmm):
    kw = em_case(7, n_loci=2, samples=(3, 4), reads_per_sample=(2, 3))
    with balanced(hmm, "hipstr_em_train"):
        assert len(capi.run_em(hmm, "hipstr_", **kw)[0]) == 2
