"""Helper (not a test module) of tests/test_threads_gpu.py: the long-lived worker threads, the oracle behind a lock, and one job per stage
call of include/hipstr_hmm.h — the inputs, a closure that makes the call and returns its arrays, and the stage's own check of the serial
result.  The closures and case makers are the stage tests' (most of them the `run` of a poisoned-cache test); nothing is restated here.

Every job is built and run once on the main thread before a worker starts (signatures bound, fixtures read, the oracle's tables made), and
that serial result — held to the oracle, the golden records or the restatement by `check` — is what every threaded result must equal bit
for bit.  A job's closure never touches a process-global switch: no environment variable, no hipstr_debug_* setter, no trim."""
import ctypes as C
import os
import queue
import threading
import time
import traceback

import numpy as np

from hipstr_amd import capi
import route_cases as rc
from test_poison_gpu import same_bits

W = 8                                   # worker threads: each gets its own pair of streams in the library, for the life of the process
POISON = (0xFF, 0x7F, 0x80)             # between rounds, in turn
FILL = -3.25
STUCK = []                              # the jobs that never came back; once non-empty every later test of the module fails at once


def limit_of(serial_seconds):
    """How long the main thread waits for a round whose jobs took serial_seconds on one thread."""
    return max(60.0, 20.0 * serial_seconds)


class Workers:
    """W daemon threads fed from queues.  round() hands every worker a list of (name, callable) and waits for all of them."""

    def __init__(self, n=W):
        self.n = n
        self.inq = [queue.Queue() for _ in range(n)]
        self.done = queue.Queue()
        self.now = [None] * n
        self.threads = [threading.Thread(target=self._loop, args=(t,), daemon=True, name="hipstr-worker-%d" % t) for t in range(n)]
        for th in self.threads:
            th.start()

    def _loop(self, t):
        while True:
            jobs = self.inq[t].get()
            if jobs is None:
                return
            out = []
            for name, fn in jobs:
                self.now[t] = name
                try:
                    out.append((name, fn(), None))
                except BaseException as e:      # noqa: BLE001 - reported by the main thread
                    out.append((name, None, "%r\n%s" % (e, traceback.format_exc(limit=6))))
            self.now[t] = None
            self.done.put((t, out))

    def round(self, lists, limit):
        """lists[t]: worker t's (name, callable) in order -> per worker the list of (name, result, error text or None)."""
        assert not STUCK, STUCK
        assert len(lists) <= self.n
        busy = set()
        for t, jobs in enumerate(lists):
            if jobs:
                self.inq[t].put(list(jobs)); busy.add(t)
        res = [[] for _ in lists]
        deadline = time.monotonic() + limit
        while busy:
            try:
                t, out = self.done.get(timeout=max(0.0, deadline - time.monotonic()))
            except queue.Empty:
                STUCK.extend("worker %d in %s" % (t, self.now[t]) for t in sorted(busy))
                raise AssertionError("no answer within %.0f s: %s" % (limit, STUCK))
            res[t] = out; busy.discard(t)
        return res

    def close(self):
        if STUCK:
            return                      # (daemon threads: a stuck one goes with the process)
        for q in self.inq:
            q.put(None)
        for th in self.threads:
            th.join(5.0)


class LockedOracle:
    """The oracle library behind one lock per call: oracle/hipstr_oracle.c keeps file-scope state (its lazily built tables, g_cr_math, the
    g_dbg_* probes) and is test code, not the code under test.  Never wrapped around the product library."""

    def __init__(self, lib):
        self._lib, self._lock = lib, threading.Lock()

    def __getattr__(self, name):
        fn = getattr(self._lib, name); lock = self._lock
        def call(*a):
            with lock:
                return fn(*a)
        return call


class Job:
    def __init__(self, name, run, check=None, same=same_bits):
        self.name, self.run, self.check, self.same = name, run, check, same
        self.want = None; self.seconds = 0.0

    def serial(self):
        t0 = time.perf_counter()
        self.want = self.run()
        self.seconds = time.perf_counter() - t0
        if self.check:
            self.check(self.want)
        return self

    def compare(self, got, t, rnd, bad):
        """A threaded result against the serial one; a difference goes to `bad` as (thread, round, job, first differing array)."""
        try:
            self.same(got, self.want, self.name)
        except AssertionError as e:
            bad.append((t, rnd, self.name, str(e)[:300]))


def serial_pass(jobs):
    """Every job once on the calling thread -> the wall time of the pass."""
    t0 = time.perf_counter()
    for j in jobs:
        j.serial()
    return time.perf_counter() - t0


def threaded(workers, lists, rnd, limit, bad):
    """lists[t]: worker t's jobs.  Runs them, compares on the worker, collects (thread, round, job, what) into bad."""
    def wrap(j, t):
        def go():
            j.compare(j.run(), t, rnd, bad)
        return (j.name, go)
    res = workers.round([[wrap(j, t) for j in jobs] for t, jobs in enumerate(lists)], limit)
    for t, out in enumerate(res):
        for name, _, err in out:
            if err:
                bad.append((t, rnd, name, err))


def in_use(hmm):
    """(device blocks, pinned blocks) that are out of the calling thread's context's caches."""
    o = (C.c_int64 * 12)()
    assert hmm.hipstr_debug_cache_stats(o) == 0
    return int(o[2]), int(o[6])


def poison(hmm, rnd):
    filled = hmm.hipstr_debug_cache_poison(POISON[rnd % len(POISON)])
    assert filled > 0, hmm.hipstr_last_error().decode()


def as_arrays(d):
    """A dict of numpy arrays, ctypes string buffers, bytes and scalars with the buffers and bytes as uint8 arrays (for same_bits)."""
    out = {}
    for k, v in d.items():
        if isinstance(v, (bytes, bytearray)):
            v = np.frombuffer(bytes(v), np.uint8)
        elif isinstance(v, C.Array):
            v = np.frombuffer(v.raw, np.uint8)
        out[k] = v
    return out


# ====================================================================================================================== the stage table
def forward_jobs(hmm, oracle):
    """Two loci of tests/test_hmm_gpu.py::test_one_locus_calls_from_many_host_threads: a plain one, and one with inherited interruptions
    (kernel _rp on the thread's side stream).  The synthesiser reads its switches when the batch is made, here, on the main thread."""
    out = []
    for name, inherit, imperfect, kw in (("forward_interrupted", 2, "0.0", dict(reads_per_locus=40, n_str_alleles=32)),
                                         ("forward_plain", 0, "0.05", dict(reads_per_locus=50, n_str_alleles=4))):
        with rc.environ({"HIPSTR_SYNTH_INHERIT": str(inherit), "HIPSTR_SYNTH_IMPERFECT": imperfect}):
            sb = capi.SynthBatch(n_loci=1, seed=900 + len(out), **kw)
        want = capi.run_align(oracle, "oracle_", sb.ptr, fill=FILL)
        def check(got, want=want, name=name):
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), name + " against the oracle"
        out.append(Job(name, lambda sb=sb: capi.run_align(hmm, "hipstr_hmm_", sb.ptr, fill=FILL), check))
    return out


def trace_jobs(hmm, oracle):
    """hipstr_hmm_trace (host replay) and hipstr_hmm_trace_ex(TRACE_ASSEMBLE_DEVICE) on one small case of tests/stage_route_cases.py
    that takes its workspace budget from no environment variable."""
    import stage_route_cases as sc
    import test_trace_assemble_gpu as tta
    import util
    call = sc.trace_single_class(sc.limits(hmm)["trace"], 2)
    assert call.ws_mib is None
    h2r = sc.h2r_of(oracle, call); n = len(call.rr)
    want = capi.run_trace(oracle, "oracle_", call.batch.ptr, call.rr, call.aa, h2r, cap=1 << 21, req_seed=call.seeds)
    def make(flags):
        run = lambda: capi.run_trace(hmm, "hipstr_hmm_", call.batch.ptr, call.rr, call.aa, h2r, cap=1 << 21, unpack=False, req_seed=call.seeds, flags=flags)
        check = lambda got: util.assert_traces_equal(capi.unpack_trace(got, n), want, "trace %s flags %d" % (call.name, flags))
        return run, check, (lambda a, b, what: tta.assert_raw_equal(a, b, n, what))
    return [Job("trace_host_replay", *make(0)), Job("trace_ex_device_assembly", *make(capi.TRACE_ASSEMBLE_DEVICE))]


def resident_chain_job(hmm, oracle):
    """tests/test_trace_resident_gpu.py's poisoned-cache chain: forward -> rm_scatter -> posteriors -> post_assign(RETRACE) ->
    hipstr_hmm_trace_resident -> hipstr_post_census_dev -> hipstr_assign_trace_stats_dev -> hipstr_trace_dev_fetch(FLANKS) -> free."""
    import test_census_gpu as tc
    import test_trace_resident_gpu as ttr
    k = tc.chain_inputs(hmm, oracle)
    keys = tc.KEYS + ("cand",)
    strip = lambda g: {x: (g[x] if x == "cand" else np.asarray(g[x])) for x in keys}
    def run():
        got, asg, extra = ttr.run_chain_resident(hmm, k, stats=True)
        return as_arrays(dict(strip(got), read_req=asg["read_req"], req_read=asg["req_read"], **extra))
    def check(out):
        want, asg, tr = tc.run_chain(hmm, k)                    # the host path of the same chain, and the restatement of the census
        same_bits(strip(want), {x: out[x] for x in keys}, "resident chain against run_chain")
        tc.compare(dict(want, rc=0), tc.chain_want(k, asg, tr), "resident chain")
        pb = capi.PostBatch(log_aln_probs=None, **k.kw)
        st = capi.run_assign_trace_stats(hmm, pb, asg["read_req"], tr, asg["best_hap"], *ttr.chain_stats_tables(k))
        for g, w, nm in zip((out["n_stutter"], out["n_flank_indel"], out["ml_bp"]), st, ("n_stutter", "n_flank_indel", "ml_bp")):
            assert np.array_equal(g, w), nm
    return Job("resident_trace_chain", run, check), k


def nw_job(hmm, oracle):
    from nw_cases import nw_pairs
    pairs = nw_pairs(41, n=80)
    want = capi.run_nw(oracle, "oracle_", pairs, False)
    def check(got):
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "nw pair %d" % i
    return Job("nw_align", lambda: capi.run_nw(hmm, "hipstr_", pairs, False), check)


def posterior_jobs(hmm, oracle):
    """hipstr_post_run on one case of the route table; hipstr_post_upload / _launch / _extract on the smallest golden fixture."""
    import stage_route_cases as sc
    import test_genotypes_gpu as tg
    import test_stage_routes_gpu as tsr
    import util
    call = sc.post_calls(sc.limits(hmm)["post"])[0]
    def check_post(got):
        def cr():
            with capi.oracle_cr_math(oracle):
                return capi.run_posteriors(oracle, "oracle_", call.pb)
        util.assert_arrays_exact(got, capi.run_posteriors(oracle, "oracle_", call.pb), cr, "posteriors " + call.name)
    path = min(tg.FIXTURES, key=os.path.getsize)
    pb, nv, h2a, exp = util.load_gt_fixture(path)
    def check_gt(got):
        def cr():
            with capi.oracle_cr_math(oracle):
                return capi.run_gt_extract(oracle, "oracle_", pb, nv, h2a)
        util.assert_genotypes_exact(got, exp, cr, os.path.basename(path), verify=(oracle, pb, nv, h2a))
    return [Job("post_run", lambda: tsr._post(hmm, call.pb), check_post),
            Job("post_extract", lambda: capi.run_gt_extract(hmm, "hipstr_", pb, nv, h2a, calc_gls=True, calc_pls=True, calc_phased_gls=True), check_gt)]


def assign_job(hmm, oracle):
    import test_assign_gpu as ta
    sizes = ta.EDGE_SIZES["workgroup_per_unit"]
    pb, LL, seed, reverse = ta.edges_inputs(sizes)
    n = int(pb.a["read_off"][-1])
    pool = ((np.arange(n) * 5) % 7).astype(np.int32); pool_off = np.array([0, 7], np.int32)
    mg = ta.oracle_map(oracle, pb)
    kw = dict(reverse=reverse, pool_index=pool, pool_off=pool_off, rule=capi.ASSIGN_RETRACE)
    def check(got):
        assert got["rc"] == 0
        ta.check(got, pb, LL, mg, seed, "post_assign edges", requests=True, **kw)
    return Job("post_assign", lambda: capi.run_assign(hmm, pb, seed, **kw), check)


def em_jobs(hmm, oracle):
    """hipstr_em_train on the smallest golden fixture; hipstr_em_train_dev on the case of tests/test_em_from_traces_gpu.py's poisoned-cache
    test, the posterior run uploaded and the trace handle made by the calling thread."""
    import test_em_from_traces_gpu as tef
    import test_em_gpu as te
    import test_em_oracle as teo
    path = min(teo.FIXTURES, key=os.path.getsize)
    kw, d = teo.load(path)
    check_em = lambda got: te._exact(got, (d["expect_trained"], d["expect_stutter"], d["expect_n_iter"], d["expect_final_ll"]), oracle, kw, "EM " + os.path.basename(path))
    c = tef.main_case()
    def run_dev():
        with tef.Resident(hmm, c) as R:
            return tuple(np.asarray(x) for x in R.train()) + tuple(np.asarray(v) for k, v in sorted(R.fetch().items()) if k != "route")
    def check_dev(got):
        want, _ = tef.check_equal(hmm, oracle, c, "em_train_dev, 6 loci")
        same_bits(got[:6], tuple(np.asarray(x) for x in want), "em_train_dev against check_equal's run")
    return [Job("em_train", lambda: capi.run_em(hmm, "hipstr_", **kw), check_em), Job("em_train_dev", run_dev, check_dev)]


class ReadMatCase:
    """The small case of tests/test_readmat_gpu.py's refusal test: A = 3 and 4, 5 and 2 pools, 9 reads, three mate pairs; then a remap that
    drops a column of locus 1 and permutes the others."""

    def __init__(self, hmm):
        import test_readmat_gpu as trm
        self.trm = trm
        self.b = trm.pooled_batch(trm.SHAPES1[1:3], [5, 2], [None, None])
        self.A = [3, 4]; self.ro = [0, 7, 9]; self.pool = [0, 1, 2, 3, 4, 4, 0, 0, 1]; self.mates = [0, 1, 0, 0, 0, 1, 0, 0, 1]; self.po = [0, 5, 7]
        self.new_A = [3, 4]; self.mapping = [2, 0, 1, 1, 3, -1, 0]
        self.bad_pool = [0, 1, 2, 3, 5, 4, 0, 0, 1]                 # pool 5 of a locus with 5 pools: hipstr_rm_scatter refuses it on the host


def readmat_job(hmm):
    """hipstr_rm_create / scatter / fetch / remap / fetch / free."""
    c = ReadMatCase(hmm); trm = c.trm
    def run():
        dev = trm.upload_and_align(hmm, c.b); rm = None
        try:
            rm = capi.ReadMatrix(hmm, c.A, c.ro, c.pool, c.mates)
            rm.scatter(dev)
            m1, s1 = rm.fetch()
            rm.remap(c.new_A, c.mapping)
            m2, s2 = rm.fetch()
            return m1.copy(), s1.copy(), m2.copy(), s2.copy()
        finally:
            if rm:
                rm.close()
            hmm.hipstr_hmm_free(dev)
    def check(got):
        ll, sd = capi.run_align(hmm, "hipstr_hmm_", c.b.ptr, fill=trm.FILL)
        want = np.full(7 * 3 + 2 * 4, trm.UNALIGNED); seeds = np.full(9, -1, np.int32)
        trm.host_scatter(want, seeds, c.A, c.ro, c.pool, c.mates, np.ones(9, bool), ll, sd, c.po, [None, None])
        trm.same(got[0], want, "read matrix after the scatter"); assert np.array_equal(got[1], seeds)
        trm.same(got[2], trm.host_remap(want, c.A, c.ro, c.new_A, c.mapping), "read matrix after the remap"); assert np.array_equal(got[3], seeds)
    return Job("read_matrix", run, check), c


def pool_job(hmm, loci=None, name="pool_reads"):
    import pool_cases as pc
    if loci is None:
        T = capi.pool_plan(hmm, pc.batch_of([]).ptr)["thresholds"]
        loci = pc.named_loci(T["HS_POOL_NET"], T["HS_POOL_HASH_STEP"])["counts"]
    b = pc.batch_of(loci)
    check = lambda got: pc.assert_pooled(got, pc.restate(loci), name)
    j = Job(name, lambda: capi.run_pool(hmm, b.ptr), check, same=pc.assert_same)
    j.n_loci = len(loci)
    return j


def hapgen_job(hmm, loci=None, name="hapgen"):
    import hapgen_cases as hc
    if loci is None:
        loci = []
        for nm in sorted(hc.BATCHES):
            loci += hc.load_golden(nm)[0]
        loci += hc.no_flagged_loci()
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    def check(got):
        hc.assert_result(got, hc.expectation(loci), name)
        hc.assert_same(got, capi.run_hapgen(hmm, b.ptr, rq, host=True), name + ", device against host twin")
    j = Job(name, lambda: capi.run_hapgen(hmm, b.ptr, rq), check, same=hc.assert_same)
    j.n_loci = len(loci)
    return j


def flank_job(hmm, loci=None, name="flank_assemble_dev"):
    """hipstr_flank_assemble_dev with every task on the device (the compiled caps); the posterior run and the trace handle are the calling
    thread's own."""
    import flank_cases as fk
    import test_flank_gpu as tfg
    c = fk.build(fk.unit_loci() if loci is None else loci)
    def run():
        with tfg.Resident(hmm, c) as R:
            return as_arrays(R.run()["raw"])
    def check(got):
        with tfg.Resident(hmm, c) as R:
            dev = R.run(); last = capi.flank_last(hmm); host = R.host_form()
        assert last["host_tasks"] == 0 and last["tasks"] == 2 * int(c.samp_off[-1]), last
        fk.same_bytes(dev, host, name + ": device against hipstr_flank_assemble")
        same_bits(as_arrays(dev["raw"]), got, name + ", second run")
    j = Job(name, run, check)
    j.n_tasks = 2 * int(c.samp_off[-1])
    return j


def alleles_job(hmm, cases=None, name="alleles_apply"):
    """hipstr_alleles_apply on the device: by default the `unit` batch plus wide_1000 (a full table) and old_haps_over (the host code inside
    the device call) of `edges`."""
    import alleles_cases as ac
    import alleles_checks as chk
    capi._alleles_sigs(hmm)
    recs = dict(chk.golden("unit")[1]); recs.update(chk.golden("edges")[1])
    if cases is None:
        by = {c["name"]: c for c in chk.golden("edges")[0]}
        cases = list(chk.golden("unit")[0]) + [by["wide_1000"], by["old_haps_over"]]
    def run():
        a = chk.apply_cases(hmm, cases, host=False)
        try:
            return a.arrays()
        finally:
            a.free()
    def check(got):
        a = chk.apply_cases(hmm, cases, host=False)
        try:
            chk.check_golden(a, cases, recs)
            same_bits(a.arrays(), got, name + ", second run")
        finally:
            a.free()
    j = Job(name, run, check)
    j.n_loci = len(cases)
    return j


def stage_table(hmm, oracle):
    """One job per stage call -> (jobs, the resident chain's inputs, the read matrix case)."""
    chain, k = resident_chain_job(hmm, oracle)
    rm, rmc = readmat_job(hmm)
    jobs = forward_jobs(hmm, oracle) + trace_jobs(hmm, oracle) + [chain, nw_job(hmm, oracle)] + posterior_jobs(hmm, oracle) + [assign_job(hmm, oracle)]
    jobs += em_jobs(hmm, oracle) + [rm, pool_job(hmm), hapgen_job(hmm), flank_job(hmm), alleles_job(hmm)]
    assert len({j.name for j in jobs}) == len(jobs)
    return jobs, k, rmc
