"""GPU: every resident stage call from many host threads at once, against the same calls made one after another.

The deployment shape of INTEGRATION.md is one host thread per locus: N threads of one process run the whole genotype() chain, each on its
own pair of streams (thread_stream / thread_aux_stream, api.hip); the context, the event pool and the two block caches are shared.  What
keeps that safe is one rule (api_internal.h, the destructors of HostArena, ScratchBufs, ResultBlocks and ChunkBlocks): a block goes back to
its cache only after the stream that may still be working on it has been waited for, whichever way the call leaves.  A call that breaks it
is invisible from one thread — the next taker queues behind the unfinished work on the same stream — and overwrites a block under a
running kernel from two.  The per-thread records (t_last of pool.hip, hapgen.hip and alleles.hip, g_last* of flank.hip, hipstr_last_error)
and the global map of read matrices are the other state only a second thread can get wrong.

The yardstick is the serial result, which the rest of the suite pins to the reference: every job (tests/thread_jobs.py) runs once on the
main thread before a worker starts, that result is checked by the stage's own helper against the oracle, the golden records or the
restatement, and every threaded result must equal it bit for bit.  No tolerance anywhere.

Mechanics: one pool of 8 daemon threads for the whole module (a thread's streams live until the process ends); everything in this
process; between rounds, with every worker idle, hipstr_debug_cache_poison with 0xFF, 0x7F, 0x80 in turn, so that a block read before it
is written holds something other than the last round's correct answer; no process-global switch changes while workers run.  The main
thread waits for a round at most max(60 s, 20 x the serial wall time of that round's jobs, measured in the same test); when the limit is
reached the test fails with the jobs still running and every later test of the module fails at once, without a library call."""
import math
import threading
import time

import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
import flow_chain_flanks as ff
import flow_chain_hapgen as fh
import flow_chain_step as fs
import thread_jobs as tj
from test_flow_chain_gpu import ROUND_KEYS, same_rounds
from test_flow_chain_step import same_flank_rounds
from test_poison_gpu import same_bits

pytestmark = pytest.mark.gpu
W = tj.W


@pytest.fixture(autouse=True)
def not_stuck():
    assert not tj.STUCK, "an earlier test of this module left a chain stuck: %s" % tj.STUCK


@pytest.fixture(scope="module")
def workers(hmm):
    assert not tj.STUCK
    capi._alleles_sigs(hmm)
    hmm.hipstr_hmm_trim()                       # what the tests before left in the caches: a poison fill then costs milliseconds
    w = tj.Workers(W)
    yield w
    w.close()


@pytest.fixture(scope="module")
def locked(oracle):
    return tj.LockedOracle(oracle)


def settled(hmm, start, jobs, what):
    """After the rounds: every block is back, and the jobs once more on this thread take nothing from the driver and give the serial bits."""
    assert tj.in_use(hmm) == start, "%s: (device, pinned) blocks in use %s, %s before" % (what, tj.in_use(hmm), start)
    allocs = hmm.hipstr_debug_driver_allocs()
    bad = []
    for j in jobs:
        j.compare(j.run(), "main", "after", bad)
    assert not bad, bad[:5]
    assert hmm.hipstr_debug_driver_allocs() == allocs, "%s: a serial pass after the rounds took %d blocks from the driver" % (what, hmm.hipstr_debug_driver_allocs() - allocs)
    assert tj.in_use(hmm) == start, what


def two_rounds(hmm, workers, jobs, what):
    """The jobs dealt to the workers, then in reverse order, poison before each round."""
    start = tj.in_use(hmm)
    serial = tj.serial_pass(jobs)
    limit = tj.limit_of(serial)
    bad = []
    for rnd in range(2):
        tj.poison(hmm, rnd)
        order = jobs if rnd == 0 else jobs[::-1]
        tj.threaded(workers, [order[t::W] for t in range(W)], rnd, limit, bad)
    assert not bad, "%s: %d of %d threaded results differ or failed (thread, round, job, what): %s" % (what, len(bad), 2 * len(jobs), bad[:5])
    settled(hmm, start, jobs, what)
    print("%s: %d jobs, serial %.2f s, limit %.0f s" % (what, len(jobs), serial, limit))


# ====================================================================================================== 1. the resident chain, one thread per locus
def chain_job(name, run, gold, same_recs):
    """run() -> (dump, per-round records) of one locus on a backend of its own."""
    def same(a, b, what):
        assert a[0] == b[0], what + ": dump"             # 17 digits: equal text is equal bits
        same_recs(a[1], b[1], what)
    return tj.Job(name, run, lambda got: gold(got[0]), same)


def on_backend(make, run, *args):
    be = make(); recs = []
    try:
        out = run(*((args[0], be) + args[1:] + (recs,)))
        return out, recs
    finally:
        be.close()


def test_resident_chain_one_thread_per_locus(hmm, locked, workers):
    """tests/test_flow_chain_gpu.py::test_one_locus_per_batch_gives_the_same with the twelve loci in flight together: twelve fc.run([name])
    on eight threads, each on a backend of its own, twice."""
    names = list(fc.CASES)
    whole, _ = on_backend(lambda: fc.DeviceBackend(hmm), fc.run, names, locked)
    jobs = []
    for n in names:
        def run(n=n):
            out, recs = on_backend(lambda: fc.DeviceBackend(hmm), fc.run, [n], locked)
            return out[n], recs
        def gold(dump, n=n):
            assert dump == whole[n], n + ": alone against the one-batch run"
            fc.against_gold(dump, n)
        jobs.append(chain_job("chain " + n, run, gold, lambda a, b, what: same_rounds(a, b, ROUND_KEYS, what)))
    two_rounds(hmm, workers, jobs, "resident chain")


def test_stepped_chain_one_thread_per_locus(hmm, locked, workers):
    """The chain through hipstr_alleles_step / hipstr_alleles_apply (tests/flow_chain_step.py, host=False): the twelve no-flank loci and the
    six flank loci, one per thread."""
    names, flank_names = list(fc.CASES), list(ff.CASES)
    whole, _ = on_backend(lambda: fc.DeviceBackend(hmm), fs.run, names, locked, hmm, False)
    flank_whole, _ = on_backend(lambda: ff.DeviceBackend(hmm), fs.run_flanks, flank_names, locked, hmm, False)
    jobs = []
    for n in names + flank_names:
        flank = n in ff.CASES
        def run(n=n, flank=flank):
            if flank:
                out, recs = on_backend(lambda: ff.DeviceBackend(hmm), fs.run_flanks, [n], locked, hmm, False)
            else:
                out, recs = on_backend(lambda: fc.DeviceBackend(hmm), fs.run, [n], locked, hmm, False)
            return out[n], recs
        def gold(dump, n=n, flank=flank):
            assert dump == (flank_whole if flank else whole)[n], n + ": alone against the one-batch run"
            (ff if flank else fc).against_gold(dump, n)
        jobs.append(chain_job("stepped chain " + n, run, gold, same_flank_rounds if flank else (lambda a, b, what: same_rounds(a, b, ROUND_KEYS, what))))
    two_rounds(hmm, workers, jobs, "stepped chain")


def hapgen_front_job(hmm, n):
    """hipstr_hapgen_batch -> hipstr_pool_batch -> upload / align -> fetch for one locus of the fixtures, from its reads alone."""
    import hapgen_cases as hc
    from test_flow_chain_hapgen import check_batch
    from test_readmat_gpu import upload_and_align
    inp = fh.inputs(n); loci = [fh.locus_of(inp)]
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci, give_stop=False)
    def front(ptr=None):
        hb = capi.HapgenBatch(hmm, b.ptr, rq, 0) if ptr is None else None
        pb = dev = None
        try:
            pb = capi.PooledBatch(hmm, hb.ptr if hb else ptr, 0)
            dev = upload_and_align(hmm, pb)
            n_reads, n_out, _ = capi.batch_dims(pb.ptr)
            ll = np.zeros(max(n_out, 1)); seeds = np.zeros(max(n_reads, 1), np.int32)
            assert hmm.hipstr_hmm_fetch(dev, ll.ctypes.data_as(capi._f64p), seeds.ctypes.data_as(capi._i32p)) == 0, hmm.hipstr_last_error().decode()
            out = dict(ll=ll[:n_out], seeds=seeds[:n_reads], pool_index=pb.pool_index.copy())
            if hb:
                out.update(locus=hb.locus, status=hb.status, **{"batch_" + k: v for k, v in hb.arrays().items()})
            return out
        finally:
            if dev:
                hmm.hipstr_hmm_free(dev)
            if pb:
                pb.close()
            if hb:
                hb.close()
    def check(got):
        hb = capi.HapgenBatch(hmm, b.ptr, rq, 0)
        try:
            check_batch(hb, [inp])                                    # the three blocks the reference left in the fixture
        finally:
            hb.close()
        fixture = fh.fixture_batch([inp])
        want = front(fixture.ptr)                                     # the same calls on the batch built from the fixture's own blocks
        same_bits({k: got[k] for k in want}, want, n + ": from the reads alone against the fixture's blocks")
    return tj.Job("hapgen front " + n, front, check)


def test_hapgen_front_one_thread_per_locus(hmm, workers):
    """tests/flow_chain_hapgen.py's front of the chain: hipstr_hapgen_batch -> hipstr_pool_batch -> upload / align -> fetch from the reads
    alone, each of the eighteen loci on a thread of its own."""
    two_rounds(hmm, workers, [hapgen_front_job(hmm, n) for n in fh.NAMES], "hapgen front")


# ====================================================================================================== 2. every stage call beside every other
@pytest.fixture(scope="module")
def table(hmm, oracle, workers):
    assert not tj.STUCK
    return tj.stage_table(hmm, oracle)


def test_every_stage_call_beside_every_other(hmm, workers, table):
    """Three rounds; in round r worker t walks the whole table from offset (5 t + r) with a stride coprime to its length, so that the
    workers are in different stages at any time and every pair of stages meets."""
    jobs = table[0]; n = len(jobs)
    start = tj.in_use(hmm)
    serial = tj.serial_pass(jobs)
    limit = tj.limit_of(W * serial)                              # every worker runs the whole table
    strides = [s for s in range(1, n) if math.gcd(s, n) == 1][:3]
    bad = []
    for rnd, stride in enumerate(strides):
        tj.poison(hmm, rnd)
        lists = [[jobs[(5 * t + rnd + i * stride) % n] for i in range(n)] for t in range(W)]
        assert all(len({j.name for j in L}) == n for L in lists)
        tj.threaded(workers, lists, rnd, limit, bad)
    assert not bad, "%d of %d threaded results differ or failed (thread, round, job, what): %s" % (len(bad), 3 * W * n, bad[:5])
    settled(hmm, start, jobs, "stage mix")
    print("stage mix: %d jobs x %d workers x 3 rounds, serial pass %.2f s (%s), limit %.0f s" % (
        n, W, serial, ", ".join("%s %.0f ms" % (j.name, 1e3 * j.seconds) for j in jobs), limit))


# ====================================================================================================== 3. per-thread records stay per thread
def flank_counts(hmm, n_tasks):
    return {k: (np.asarray(v) if isinstance(v, np.ndarray) else v) for k, v in capi.flank_last(hmm, n_tasks).items()}


def test_last_call_records_and_last_error_are_the_calling_threads(hmm, oracle, workers, table):
    """Four workers make hipstr_pool_reads, hipstr_hapgen, hipstr_alleles_apply and hipstr_flank_assemble_dev on inputs of different locus
    counts, meet at a barrier, and only then read the four `last call` records: each must hold the counts of that thread's own calls (the
    timing fields are not read).  Beside them one worker makes refused calls in a loop — every one decided on the host before a launch —
    and finds its own message in hipstr_last_error(); three more make stage calls that succeed."""
    import alleles_checks as chk
    import flank_cases as fk
    import hapgen_cases as hc
    import pool_cases as pc
    import stage_route_cases as sc
    from test_readmat_gpu import upload_and_align
    jobs, k, rmc = table
    start = tj.in_use(hmm)
    hap_loci = []
    for nm in sorted(hc.BATCHES):
        hap_loci += hc.load_golden(nm)[0]
    four = []; lasts = []
    for w in range(4):
        mine = [tj.pool_job(hmm, pc.fuzz_loci(7 + w, 2 + w, max_reads=60, max_len=80), "pool_reads/%d" % w),
                tj.hapgen_job(hmm, hap_loci[:3 + 2 * w], "hapgen/%d" % w),
                tj.alleles_job(hmm, list(chk.golden("unit")[0])[:3 + w], "alleles_apply/%d" % w),
                tj.flank_job(hmm, fk.unit_loci()[:1 + w], "flank_assemble_dev/%d" % w)]
        rec = {}
        for j, last in zip(mine, (lambda: capi.pool_last(hmm), lambda: capi.hapgen_last(hmm), lambda: capi.alleles_last(hmm), None)):
            t0 = time.perf_counter()
            j.want = j.run()
            j.seconds = time.perf_counter() - t0
            rec[j.name.split("/")[0]] = flank_counts(hmm, j.n_tasks) if last is None else last()      # this thread's record, right behind the call
            j.check(j.want)
        four.append(mine); lasts.append(rec)
    assert len({r["pool_reads"]["device_loci"] + r["pool_reads"]["host_loci"] for r in lasts}) == 4
    assert len({r["hapgen"]["device_loci"] + r["hapgen"]["host_loci"] for r in lasts}) == 4
    assert len({r["alleles_apply"]["device_loci"] + r["alleles_apply"]["host_loci"] + r["alleles_apply"]["identity_loci"] for r in lasts}) == 4
    assert len({r["flank_assemble_dev"]["tasks"] for r in lasts}) == 4

    N = sc.limits(hmm)["nw"]
    def refusals():
        """alleles_checks.refusals, the two size refusals of hipstr_nw_align and a pool index hipstr_rm_scatter finds outside the batch: each
        raises with hipstr_last_error() of this thread, which must be that call's own message."""
        dev = upload_and_align(hmm, rmc.b)
        try:
            for _ in range(3):
                chk.refusals(hmm, host=False)
                for pairs, msg in sc.nw_refused(N):
                    with pytest.raises(RuntimeError, match=msg):
                        capi.run_nw(hmm, "hipstr_", pairs, False)
                rm = capi.ReadMatrix(hmm, rmc.A, rmc.ro, rmc.bad_pool, rmc.mates)
                try:
                    with pytest.raises(RuntimeError, match="pool_index outside"):
                        rm.scatter(dev)
                finally:
                    rm.close()
        finally:
            hmm.hipstr_hmm_free(dev)
        return True
    t0 = time.perf_counter()
    assert any("longer than 1536" in msg for _, msg in sc.nw_refused(N))
    refusals()                                                    # once on this thread first
    beside = [j for j in jobs if j.name in ("forward_interrupted", "trace_ex_device_assembly", "post_run", "post_assign", "em_train", "read_matrix", "nw_align")]
    assert len(beside) == 7
    # a round: the sixteen record calls once, the refusals once, the seven calls beside them twice on each of three threads
    t_serial = sum(j.seconds for mine in four for j in mine) + (time.perf_counter() - t0) + 6 * tj.serial_pass(beside)
    limit = tj.limit_of(t_serial)

    bad = []
    for rnd in range(2):
        tj.poison(hmm, rnd)
        barrier = threading.Barrier(4)
        def recorder(w):
            def go():
                try:
                    outs = [j.run() for j in four[w]]
                except BaseException:
                    barrier.abort(); raise
                barrier.wait(limit)                               # all four threads have made all four calls
                got = dict(pool_reads=capi.pool_last(hmm), hapgen=capi.hapgen_last(hmm), alleles_apply=capi.alleles_last(hmm),
                           flank_assemble_dev=flank_counts(hmm, four[w][3].n_tasks))
                for j, o in zip(four[w], outs):
                    j.compare(o, w, rnd, bad)
                for key in got:
                    try:
                        same_bits(got[key], lasts[w][key], "the last-call record of %s on thread %d" % (key, w))
                    except AssertionError as e:
                        bad.append((w, rnd, key + " last", str(e)[:300]))
            return ("records/%d" % w, go)
        def succeed(t):
            def go():
                for i in range(2 * len(beside)):
                    j = beside[(i + 3 * t) % len(beside)]
                    j.compare(j.run(), t, rnd, bad)
            return ("stage calls beside the refusals/%d" % t, go)
        lists = [[recorder(w)] for w in range(4)] + [[("refusals", refusals)]] + [[succeed(t)] for t in (5, 6, 7)]
        for t, out in enumerate(workers.round(lists, limit)):
            for name, _, err in out:
                if err:
                    bad.append((t, rnd, name, err))
    assert not bad, bad[:5]
    assert tj.in_use(hmm) == start, "blocks in use %s, %s before: a refused call kept one" % (tj.in_use(hmm), start)
    print("records and refusals: serial %.2f s, limit %.0f s" % (t_serial, limit))


# ====================================================================================================== 4. handles handed between threads
def test_handles_made_on_one_thread_and_used_on_others(hmm, oracle, workers, table):
    """include/hipstr_hmm.h: a hipstr_trace_dev_t `is read-only once created — several consumer calls may use it, also at once`, and every
    object made after hipstr_hmm_init `may be used from any thread`.  Worker A makes a trace handle and a launched posterior run; B, C and D
    then call hipstr_post_census_dev, hipstr_assign_trace_stats_dev and hipstr_trace_dev_fetch (all groups) on them five times each, at the
    same moment, while A runs hipstr_em_train_dev on them; A frees them after all are done.  Second form: E makes a read matrix and
    scatters into it; F then uploads a posterior run on hipstr_rm_dev_log_aln_probs, launches and fetches it — nothing is being scattered
    while F launches (the caller's duty)."""
    import test_census_gpu as tc
    import test_trace_assemble_gpu as tta
    import test_trace_resident_gpu as ttr
    import util
    from test_readmat_gpu import upload_and_align
    k = table[1]
    start = tj.in_use(hmm)
    keys = tc.KEYS + ("cand",)
    strip = lambda g: {x: (g[x] if x == "cand" else np.asarray(g[x])) for x in keys}
    tables = ttr.chain_stats_tables(k)
    REP = 5

    # ---- the calls, each usable from any thread once the handles exist
    def make(h, asg):
        h["pd"] = hmm.hipstr_post_upload(k.pb.ptr, None); assert h["pd"], hmm.hipstr_last_error().decode()
        assert hmm.hipstr_post_launch(h["pd"], None) == 0, hmm.hipstr_last_error().decode()
        if asg is None:
            asg = capi.run_assign(hmm, h["pd"], k.seeds, pool_index=k.pool, pool_off=k.pool_off, rule=capi.ASSIGN_RETRACE, n_reads=k.n, n_samp=4)
            assert asg["rc"] == 0 and asg["n_req"] > 0
        h["td"] = capi.run_trace_resident(hmm, k.b.ptr, asg["req_read"], asg["req_allele"], capi.hap_aln_info(hmm, "hipstr_", k.b.ptr))
        return asg
    def drop(h):
        if h.get("td"):
            h["td"].close()
        if h.get("pd"):
            hmm.hipstr_post_free(h["pd"])
    census = lambda h, asg: strip(capi.run_census(hmm, h["pd"], k.b.ptr, k.seeds, asg["read_req"], asg["req_read"], None, hap_to_allele=k.h2a, n_samp=4, min_frac=0.01, td=h["td"]))
    stats = lambda h, asg: capi.assign_trace_stats_dev(hmm, k.pb, asg["read_req"], h["td"], asg["best_hap"], *tables)
    fetch = lambda h, asg: capi.trace_dev_fetch(hmm, h["td"], capi.TRACE_F_ALL)
    train = lambda h, asg: tuple(np.asarray(x) for x in capi.em_train_dev(hmm, h["pd"], 2, k.b.ptr, k.seeds, asg["read_req"], asg["req_read"], h["td"]))
    def matrix_then_posteriors(rm):
        pb = capi.PostBatch(log_aln_probs=None, **k.kw)
        pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error().decode()
        try:
            assert hmm.hipstr_post_launch(pd, None) == 0, hmm.hipstr_last_error().decode()
            S = int(pb.samp_off[-1])
            post = np.zeros(int(pb.post_off[-1])); tot = np.zeros(S); gt = np.zeros(2 * S, np.int32); ltot = np.zeros(2)
            assert hmm.hipstr_post_fetch(pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p),
                                         ltot.ctypes.data_as(capi._f64p)) == 0, hmm.hipstr_last_error().decode()
        finally:
            hmm.hipstr_post_free(pd)
        return post, tot, gt.reshape(-1, 2), ltot
    def scattered():
        dev = upload_and_align(hmm, k.b)
        try:
            rm = capi.ReadMatrix(hmm, k.A, k.read_off, k.pool)
            try:
                rm.scatter(dev)
            except BaseException:
                rm.close(); raise
            return rm
        finally:
            hmm.hipstr_hmm_free(dev)

    # ---- once on this thread, held to the host forms of the same calls
    t0 = time.perf_counter()
    h = {}
    try:
        asg = make(h, None)
        n = int(asg["n_req"])
        want = dict(census=census(h, asg), stats=stats(h, asg), fetch=fetch(h, asg), train=train(h, asg))
    finally:
        drop(h)
    rm = scattered()
    try:
        want["post"] = matrix_then_posteriors(rm)
    finally:
        rm.close()
    serial = time.perf_counter() - t0
    tr = capi.run_trace(hmm, "hipstr_hmm_", k.b.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=capi.hap_aln_info(hmm, "hipstr_", k.b.ptr), unpack=False,
                        cap=1 << 16, flags=0)
    tta.assert_raw_equal(want["fetch"], tr, n, "the fetched handle against hipstr_hmm_trace")
    tc.compare(dict(want["census"], rc=0), tc.chain_want(k, asg, tr), "census on the handle")
    for g, w_, nm in zip(want["stats"], capi.run_assign_trace_stats(hmm, k.pb, asg["read_req"], tr, asg["best_hap"], *tables), ("n_stutter", "n_flank_indel", "ml_bp")):
        assert np.array_equal(g, w_), nm
    batch = capi.em_batch_from_traces(hmm, k.pb, k.b.ptr, k.seeds, asg["read_req"], asg["req_read"], tr)
    ekw = dict(period=k.b.arrays["period"], n_samples=k.kw["n_samples"], read_off=batch["read_off"], sample_label=batch["sample_label"], num_bps=batch["num_bps"],
               log_p1=batch["log_p1"], log_p2=batch["log_p2"])
    for g, w_ in zip(want["train"][:4], capi.run_em(hmm, "hipstr_", **ekw)):
        assert np.array_equal(g, w_), "hipstr_em_train_dev against hipstr_em_train on the host-built batch"
    assert np.array_equal(want["train"][4], batch["read_off"])
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_posteriors(oracle, "oracle_", k.pb)
    util.assert_arrays_exact(want["post"], capi.run_posteriors(oracle, "oracle_", k.pb), cr, "posteriors of the resident matrix")

    # ---- across threads
    limit = tj.limit_of(4 * REP * serial)
    bad = []
    same_of = dict(census=same_bits, stats=same_bits, train=same_bits, post=same_bits, fetch=lambda a, b, what: tta.assert_raw_equal(a, b, n, what))
    def judge(key, got, t, rnd):
        try:
            same_of[key](got, want[key], key)
        except AssertionError as e:
            bad.append((t, rnd, key, str(e)[:300]))
    for rnd in range(2):
        tj.poison(hmm, rnd)
        made, used = threading.Barrier(4), threading.Barrier(4)
        shared = {}
        def maker():
            try:
                make(shared, asg)
            except BaseException:
                made.abort(); drop(shared); raise
            try:
                made.wait(limit)
                for _ in range(REP):
                    judge("train", train(shared, asg), 0, rnd)
            finally:
                try:
                    used.wait(limit)                              # freed only after every consumer is done (include/hipstr_hmm.h)
                finally:
                    drop(shared)
        def consumer(key, call, t):
            def go():
                made.wait(limit)
                try:
                    for _ in range(REP):
                        judge(key, call(shared, asg), t, rnd)
                finally:
                    used.wait(limit)
            return (key + " on another thread's handles", go)
        ready, fetched = threading.Barrier(2), threading.Barrier(2)
        box = {}
        def scatterer():
            try:
                box["rm"] = scattered()
            except BaseException:
                ready.abort(); raise
            try:
                ready.wait(limit)
                fetched.wait(limit)
            finally:
                box["rm"].close()
        def reader():
            ready.wait(limit)
            try:
                judge("post", matrix_then_posteriors(box["rm"]), 5, rnd)
            finally:
                fetched.wait(limit)
        lists = [[("handles made and freed, hipstr_em_train_dev", maker)], [consumer("census", census, 1)], [consumer("stats", stats, 2)], [consumer("fetch", fetch, 3)],
                 [("read matrix made and scattered", scatterer)], [("posteriors of another thread's read matrix", reader)]]
        for t, out in enumerate(workers.round(lists, limit)):
            for name, _, err in out:
                if err:
                    bad.append((t, rnd, name, err))
    assert not bad, bad[:5]
    assert tj.in_use(hmm) == start, "blocks in use %s, %s before" % (tj.in_use(hmm), start)
    print("handles between threads: serial %.2f s, limit %.0f s" % (serial, limit))
