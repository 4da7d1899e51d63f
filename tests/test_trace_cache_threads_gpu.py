"""GPU: eight host threads, each with a trace cache of its own (hipstr_trace_cache_*, include/hipstr_hmm.h), through two rounds, a remap, a
third round, the view and a compaction — against the same calls made one after another.

tests/test_threads_gpu.py's protocol and mechanics (tests/thread_jobs.py): every job runs once on the main thread before a worker starts,
that result is checked against the stage's own yardstick (a round's handle is the fresh hipstr_hmm_trace_resident of its list; the entries
are the numpy bookkeeping of tests/trace_cache_cases.py), and every threaded result must equal it bit for bit; two rounds, the jobs dealt
to the workers and then in reverse order, the caches' free blocks poisoned before each; afterwards every block is back and a serial pass
takes nothing from the driver.  A cache belongs to one thread at a time; the caches, their segments (one resident handle per round that
missed) and the gathered handles all come from the context's shared block caches."""
import numpy as np
import pytest

from hipstr_amd import capi
import thread_jobs as tj
import trace_cache_cases as tcc
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


def cache_job(hmm, S, t):
    """Job t: its own slice of the reads, its own cache.  Round A (alleles 0 and 1 of half its reads), round B (alleles 0, 1, 2 of all of
    them: hits and misses), a remap that drops haplotype 1 and moves the others, round C on the keys the remap freed, the view, a
    compaction, the view again."""
    reads = S.reads[t::W]
    ra, aa = S.requests([0, 1], reads[::2]); rb, ab = S.requests([0, 1, 2], reads)
    new_A, mapping = [4, 4], [2, -1, 0, 3, 2, -1, 0, 3]
    rc_, ac = S.requests([1], reads)                   # haplotype 1 is free after the remap (0 -> 2, 2 -> 0, 3 stays)
    steps = (("A", ra, aa), ("B", rb, ab), ("C", rc_, ac))

    def run():
        out = {}
        tc = capi.TraceCache(hmm, S.pool_off, S.n_alleles)
        try:
            for name, rr, al in steps:
                if name == "C":
                    tc.remap(new_A, mapping)
                    out["entries_remapped"] = list(tc.entries())
                td, st = tc.round(S.ptr, rr, al, hap_to_ref=S.h2r)
                try:
                    n, tot, c = tcc.handle_content(hmm, td)
                finally:
                    td.close()
                out[name] = dict(n=n, totals=tot, stats=st, **{k: np.frombuffer(v, np.uint8) for k, v in c.items()})
            for name in ("view", "view_compacted"):
                td = tc.view()
                try:
                    n, tot, c = tcc.handle_content(hmm, td)
                finally:
                    td.close()
                out[name] = dict(n=n, totals=tot, stats=tc.stats(), entries=list(tc.entries()), **{k: np.frombuffer(v, np.uint8) for k, v in c.items()})
                tc.compact()
        finally:
            tc.close()
        return out

    def check(out):
        book = tcc.Book(S.pool_off, S.n_alleles)
        for name, rr, al in steps:
            if name == "C":
                book.remap(new_A, mapping)
                er, ea = book.entries()
                assert np.array_equal(out["entries_remapped"][0], er) and np.array_equal(out["entries_remapped"][1], ea)
            miss, ins = book.round(rr, al)
            td = capi.run_trace_resident(hmm, S.ptr, rr, al, S.h2r)
            try:
                n, tot, c = tcc.handle_content(hmm, td)
            finally:
                td.close()
            got = out[name]
            assert got["n"] == n and np.array_equal(got["totals"], tot), name
            for k, v in c.items():
                assert got[k].tobytes() == v, "job %d round %s: %s" % (t, name, k)
            assert got["stats"]["n_misses"] == len(miss) and got["stats"]["n_inserted"] == ins and got["stats"]["n_hits"] == len(rr) - len(miss), name
            for k, v in book.state().items():
                assert got["stats"][k] == v, (name, k)
        assert out["C"]["stats"]["n_dead"] > 0 and out["B"]["stats"]["n_hits"] > 0 and out["B"]["stats"]["n_misses"] > 0
        er, ea = book.entries()
        for name in ("view", "view_compacted"):
            assert np.array_equal(out[name]["entries"][0], er) and np.array_equal(out[name]["entries"][1], ea), name
        a, b = out["view"], out["view_compacted"]
        assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("stats", "entries")), "the compaction changed the view"
        assert b["stats"]["n_dead"] == 0 and b["stats"]["n_segments"] == 1 and a["stats"]["n_segments"] == 3

    return tj.Job("trace cache %d" % t, run, check)


def test_eight_caches_on_eight_threads(hmm, oracle, workers):
    S = tcc.Setup(hmm, oracle)
    try:
        jobs = [cache_job(hmm, S, t) for t in range(W)]
        two_rounds(hmm, workers, jobs, "trace caches")
    finally:
        S.close()
