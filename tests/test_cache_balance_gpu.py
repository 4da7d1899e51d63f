"""GPU: every exit of a stage call gives every block back.  The stage calls take their device and pinned blocks from the context's caches
(hipstr_amd/csrc/api_internal.h: ResultBlocks, ChunkBlocks, ScratchBufs, HostArena); other host threads draw from the same caches, so a
block must be back, behind the stream, whichever way the call leaves.  hipstr_debug_cache_stats counts the blocks that are out: out[2] for
the device cache, out[6] for the pinned one.  With the input handles alive both numbers are read, the call is made, and they are read
again: (a) after a normal return, (b) after the return-3 path — a capacity one too small, found after the results were fetched — and (c)
after a refusal found only after blocks were taken and work was queued (the check kernel's verdict on a decreasing str_seq_off; a read
that enters the EM without STR data).  The cases are the smallest ones of the stages' own test modules; what the calls compute is held to
its yardsticks there.

The handles themselves are balanced around their whole life, freed early (before a launch, an align, a scatter) included: the posterior
run in both of its forms (hipstr_post_upload / launch / fetch / free, hipstr_post_run, hipstr_post_extract), the read matrix
(hipstr_rm_create / scatter / remap / fetch / free, a refused remap) and the forward handle (hipstr_hmm_upload / align / fetch / free,
hipstr_hmm_process_reads); so are the four debug entry points of the float and cr_math primitives."""
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
import test_readmat_gpu as trm
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


def small_pb():
    """Two loci, three samples, eleven reads."""
    row = lambda A, h: [(-1.0 if k == h else -30.0) - 0.01 * k for k in range(A)]
    return ta.make_pb([(3, [[(-0.5, -0.5, row(3, 0))] * 3, [(-0.2, -0.9, row(3, 2))] * 2]), (2, [[(-0.5, -0.5, row(2, 1))] * 6])])[0]


def large_pb():
    """One locus of 64 haplotypes and 128 samples, one read per sample: the results alone are 128 x 64 x 64 x 8 B = 4 MiB, so the run takes
    the form with a block per array."""
    rng = np.random.default_rng(11)
    return capi.PostBatch([64], [128], [0, 128], np.arange(128), -rng.random(128), -rng.random(128), np.ones(128, np.int32), -50 * rng.random(128 * 64))


def post_results(pb):
    S = int(pb.samp_off[-1])
    k = [np.zeros(int(pb.post_off[-1])), np.zeros(S), np.zeros(2 * S, np.int32), np.zeros(pb.struct.n_loci)]
    return k, [a.ctypes.data_as(t) for a, t in zip(k, (capi._f64p, capi._f64p, capi._i32p, capi._f64p))]


@pytest.mark.parametrize("make", [small_pb, large_pb], ids=["small", "large"])
def test_posterior_run(hmm, make):
    """Upload, launch, fetch, free; upload then free; hipstr_post_run — the three ways give the same results."""
    pb = make()
    assert (int(pb.post_off[-1]) * 8 >= 4 << 20) == (make is large_pb)
    with balanced(hmm, "hipstr_post_upload, launch, fetch, free"):
        with launched(hmm, pb) as pd:
            got, ptrs = post_results(pb)
            assert hmm.hipstr_post_fetch(pd, *ptrs) == 0, hmm.hipstr_last_error().decode()
    with balanced(hmm, "hipstr_post_upload, free"):
        with launched(hmm, pb, launch=False):
            pass
    with balanced(hmm, "hipstr_post_run"):
        one, ptrs = post_results(pb)
        assert hmm.hipstr_post_run(pb.ptr, None, *ptrs) == 0, hmm.hipstr_last_error().decode()
    for a, b in zip(got, one):
        assert np.array_equal(a, b)
    assert np.all(got[2] >= 0) and np.all(np.isfinite(got[0])) and np.all(got[1] < 0)


def test_post_extract(hmm):
    """The small run, two variants on three and on two haplotypes: every optional output, then none."""
    pb = small_pb()
    kw = dict(n_variants=[2, 2], hap_to_allele=[0, 1, 1, 0, 1])
    with balanced(hmm, "hipstr_post_extract, gls + pls + phased_gls"):
        full = capi.run_gt_extract(hmm, "hipstr_", pb, **kw)
    with balanced(hmm, "hipstr_post_extract, no optional output"):
        bare = capi.run_gt_extract(hmm, "hipstr_", pb, calc_gls=False, calc_pls=False, calc_phased_gls=False, **kw)
    for k in ("best_hap", "best_gt", "log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post"):
        assert np.array_equal(full[k], bare[k]), k
    assert np.all(full["best_gt"] >= 0) and np.all(full["best_gt"] < 2) and full["best_hap"].tolist() == [[0, 0], [2, 2], [1, 1]] and full["best_gt"].tolist() == [[0, 0], [1, 1], [1, 1]]
    assert all(len(g) == 3 and np.isfinite(g).all() for g in full["gls"]) and all(min(p) == 0 for p in full["pls"])


def test_read_matrix(hmm):
    """Two loci of 3 and 4 haplotypes, seven and two reads, three mate pairs: created without initial values, filled from an aligned batch,
    a remap that raises the first locus' haplotype count (more flags than the staging blocks hold: they are replaced), one that lowers it."""
    small = trm.pooled_batch(trm.SHAPES1[1:3], [5, 2], [None, None])
    A = [3, 4]; ro = [0, 7, 9]; pool = [0, 1, 2, 3, 4, 4, 0, 0, 1]; mates = [0, 1, 0, 0, 0, 1, 0, 0, 1]
    dev = trm.upload_and_align(hmm, small)
    try:
        with balanced(hmm, "hipstr_rm_create, scatter, remap, remap, fetch, free"):
            with handle(capi.ReadMatrix(hmm, A, ro, pool, mates)) as rm:
                rm.scatter(dev)
                before, seeds = rm.fetch()
                rm.remap([5, 4], [4, 0, 2] + [0, 1, 2, 3])
                rm.remap([2, 4], [0, -1, -1, -1, 1] + [0, 1, 2, 3])
                after, seeds2 = rm.fetch()
            rows = before[:21].reshape(7, 3)
            assert np.array_equal(after[:14].reshape(7, 2), rows[:, [1, 0]]) and np.array_equal(after[14:], before[21:]) and np.array_equal(seeds, seeds2)
            assert np.all(before != trm.UNALIGNED) and np.all(seeds >= 0)
        with balanced(hmm, "hipstr_rm_create, free"):
            capi.ReadMatrix(hmm, A, ro, pool, mates).close()
        with balanced(hmm, "hipstr_rm_remap refused, free"):
            with handle(capi.ReadMatrix(hmm, A, ro, pool, mates)) as rm:
                with pytest.raises(RuntimeError, match="two old columns mapped to one new column"):
                    rm.remap([3, 4], [0, 1, 1] + [0, 1, 2, 3])
    finally:
        hmm.hipstr_hmm_free(dev)


def test_forward_handle(hmm):
    """One locus: upload, align, fetch, free; upload, free; hipstr_hmm_process_reads."""
    sb = capi.SynthBatch(n_loci=1, reads_per_locus=20, n_str_alleles=4, seed=2)
    n_reads, n_out, _ = capi.batch_dims(sb.ptr)
    probs = np.full(n_out, np.nan); seeds = np.full(n_reads, -7, np.int32)
    with balanced(hmm, "hipstr_hmm_upload, align, fetch, free"):
        dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev, hmm.hipstr_last_error().decode()
        try:
            assert hmm.hipstr_hmm_align(dev, None) == 0
            assert hmm.hipstr_hmm_fetch(dev, probs.ctypes.data_as(capi._f64p), seeds.ctypes.data_as(capi._i32p)) == 0, hmm.hipstr_last_error().decode()
        finally:
            hmm.hipstr_hmm_free(dev)
    with balanced(hmm, "hipstr_hmm_upload, free"):
        dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev, hmm.hipstr_last_error().decode()
        hmm.hipstr_hmm_free(dev)
    with balanced(hmm, "hipstr_hmm_process_reads"):
        one, s1 = capi.run_align(hmm, "hipstr_hmm_", sb.ptr)
    assert np.array_equal(one, probs, equal_nan=True) and np.array_equal(s1, seeds) and (seeds >= 0).sum() > 10


def test_debug_primitives(hmm):
    """Three arguments each."""
    x = np.array([-1.5, 0.25, 3.0]); y = np.zeros(3)
    with balanced(hmm, "hipstr_debug_cr_math"):
        assert hmm.hipstr_debug_cr_math(0, x.ctypes.data_as(capi._f64p), y.ctypes.data_as(capi._f64p), 3) == 0, hmm.hipstr_last_error().decode()
    assert np.allclose(y, np.exp(x), rtol=1e-12, atol=0)
    with balanced(hmm, "hipstr_debug_float_fn"):
        got = capi.float_fn(hmm, "hipstr_debug_float_fn", "fastexp", 0x3f800000, 3)
    assert np.array_equal(got, capi.float_fn(hmm, "hipstr_debug_float_fn_host", "fastexp", 0x3f800000, 3))
    a = np.array([-1.0, -20.0, -3.0]); b = np.array([-2.0, -1.0, -3.0])
    with balanced(hmm, "hipstr_debug_fast_lse2"):
        got = capi.fast_lse2(hmm, "hipstr_debug_fast_lse2", a, b)
    assert np.array_equal(got, capi.fast_lse2(hmm, "hipstr_debug_fast_lse2_host", a, b))
    rows = [np.array([-1.0]), np.array([-2.0, -1.0, -30.0]), np.array([-3.0, -3.0])]
    with balanced(hmm, "hipstr_debug_fast_lse_vec"):
        got = capi.fast_lse_vec(hmm, "hipstr_debug_fast_lse_vec", rows)
    assert np.array_equal(got, capi.fast_lse_vec(hmm, "hipstr_debug_fast_lse_vec_host", rows))


def test_post_assign(hmm):
    """Two loci, three samples, eleven reads in six pools: the request list has three entries."""
    pb = small_pb()
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


def test_em_train_other_exits(hmm, monkeypatch):
    """The same two loci through the round-4 host loop, and with max_iter = 0 (no locus trains: the call takes its blocks, its side stream and
    its events, and gives them back); a repeated call finds every block in the caches, eight in a row as well."""
    kw = em_case(7, n_loci=2, samples=(3, 4), reads_per_sample=(2, 3))
    monkeypatch.setenv("HIPSTR_EM_HOST_LOOP", "1")
    with balanced(hmm, "hipstr_em_train, HIPSTR_EM_HOST_LOOP=1"):
        host = capi.run_em(hmm, "hipstr_", **kw)
    monkeypatch.delenv("HIPSTR_EM_HOST_LOOP")
    with balanced(hmm, "hipstr_em_train, max_iter = 0"):
        none = capi.run_em(hmm, "hipstr_", **dict(kw, max_iter=0))
    assert not none[0].any() and not none[2].any()
    first = capi.run_em(hmm, "hipstr_", **kw)
    allocs = hmm.hipstr_debug_driver_allocs()
    with balanced(hmm, "hipstr_em_train, eight calls in a row"):
        for _ in range(8):
            again = capi.run_em(hmm, "hipstr_", **kw)
            assert all(np.array_equal(a, b) for a, b in zip(again, first))
    assert hmm.hipstr_debug_driver_allocs() == allocs
    assert np.array_equal(host[0], first[0]) and np.array_equal(host[2], first[2])
