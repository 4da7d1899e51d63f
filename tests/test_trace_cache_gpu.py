"""GPU: the trace cache — hipstr_trace_cache_* (include/hipstr_hmm.h; hipstr_amd/csrc/trace_cache.hip), SeqStutterGenotyper's trace_cache_
(seq_stutter_genotyper.cpp:805-841, :401-409, :1579) for a batch of loci.

Nothing here has a yardstick of its own.  A round's handle must be, byte for byte, a fresh hipstr_hmm_trace_resident of the round's full
request list (the traceback of a request does not depend on the other requests of the call); which requests a round traces, what the cache
lists and what it counts must be the numpy bookkeeping of tests/trace_cache_cases.py (Book: a dictionary, restated from the reference's
lines above); the consumers must give the same outputs on a round's handle and on the fresh one.  The batch: tests/trace_cache_cases.py.
No case provokes a fault: every refusal is decided on the host before a launch."""
import numpy as np
import pytest

from hipstr_amd import capi
import test_assign_gpu as ta
import test_census_gpu as tcen
import trace_cache_cases as tcc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(hmm, oracle):
    s = tcc.Setup(hmm, oracle)
    s.fresh = {}
    yield s
    s.close()


def fresh(hmm, S, rr, aa, seeds=None):
    """hipstr_hmm_trace_resident of a full list, fetched: (n, totals, content).  Computed once per list."""
    key = (tuple(int(x) for x in rr), tuple(int(x) for x in aa), None if seeds is None else tuple(seeds))
    if key not in S.fresh:
        td = capi.run_trace_resident(hmm, S.ptr, rr, aa, S.h2r, req_seed=seeds)
        try:
            S.fresh[key] = tcc.handle_content(hmm, td)
        finally:
            td.close()
    return S.fresh[key]


def new_cache(hmm, S):
    return capi.TraceCache(hmm, S.pool_off, S.n_alleles), tcc.Book(S.pool_off, S.n_alleles)


def one_round(hmm, S, tc, book, rr, aa, takes=None, seeds=None, what=""):
    """A round on the cache and on the book: the handle equals the fresh trace of the full list, the counts equal the book's."""
    miss, ins = book.round(rr, aa, takes)
    td, st = tc.round(S.ptr, rr, aa, hap_to_ref=S.h2r, req_seed=seeds, locus_takes=takes)
    try:
        n, tot, got = tcc.handle_content(hmm, td)
    finally:
        td.close()
    wn, wtot, want = fresh(hmm, S, rr, aa, seeds)
    assert n == wn == len(rr) and np.array_equal(tot, wtot), what
    tcc.assert_same(got, want, what)
    assert st["n_misses"] == len(miss) and st["n_hits"] == len(rr) - len(miss) and st["n_inserted"] == ins, (what, st)
    same_state(tc, book, what, st)
    return st


def same_state(tc, book, what, st=None):
    st = tc.stats() if st is None else st
    for k, v in book.state().items():
        assert st[k] == v, (what, k, st, book.state())
    er, ea = tc.entries(); wr, wa = book.entries()
    assert np.array_equal(er, wr) and np.array_equal(ea, wa), what


def view_equals_fresh(hmm, S, tc, what):
    """hipstr_trace_cache_view: the entries' records, which are the fresh tracebacks of the entries."""
    er, ea = tc.entries()
    td = tc.view()
    try:
        n, tot, got = tcc.handle_content(hmm, td)
    finally:
        td.close()
    wn, wtot, want = fresh(hmm, S, er, ea)
    assert n == wn and np.array_equal(tot, wtot), what
    tcc.assert_same(got, want, what)
    return got


def test_subset_then_superset_then_the_same_again(hmm, S):
    tc, book = new_cache(hmm, S)
    ra, aa = S.requests([1, 3], S.reads[::3])
    rb, ab = S.requests([0, 1, 3])
    new_keys = len(set(zip(rb.tolist(), ab.tolist())) - set(zip(ra.tolist(), aa.tolist())))
    st = one_round(hmm, S, tc, book, ra, aa, what="round A")
    assert st["n_misses"] == len(ra) and st["n_hits"] == 0 and st["n_segments"] == 1
    st = one_round(hmm, S, tc, book, rb, ab, what="round B")
    assert st["n_misses"] == new_keys and st["n_hits"] == len(ra) and 0 < new_keys < len(rb) and st["n_segments"] == 2
    st = one_round(hmm, S, tc, book, rb, ab, what="round B again")
    assert st["n_misses"] == 0 and st["n_hits"] == len(rb) and st["n_segments"] == 2 and st["n_dead"] == 0
    view_equals_fresh(hmm, S, tc, "view after three rounds")
    # a key twice in one list is traced once; an empty list gives a valid empty handle
    tc2, book2 = new_cache(hmm, S)
    st = one_round(hmm, S, tc2, book2, np.repeat(ra[:5], 2), np.repeat(aa[:5], 2), what="repeated keys")
    assert st["n_misses"] == 5 and st["n_hits"] == 5
    st = one_round(hmm, S, tc2, book2, [], [], what="empty list")
    assert st["n_misses"] == 0 and st["n_hits"] == 0
    tc.close(); tc2.close()


def test_a_locus_that_does_not_take(hmm, S):
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([0, 2])
    in1 = int((rr >= S.pool_off[1]).sum())
    st = one_round(hmm, S, tc, book, rr, aa, takes=[1, 0], what="locus 1 does not take")
    assert st["n_misses"] == len(rr) and st["n_inserted"] == len(rr) - in1 and st["n_dead"] == in1 and in1 > 0
    assert np.all(tc.entries()[0] < S.pool_off[1])
    st = one_round(hmm, S, tc, book, rr, aa, takes=[1, 0], what="the same round again")
    assert st["n_misses"] == in1 and st["n_inserted"] == 0 and st["n_segments"] == 1       # the same misses; a segment nobody takes from is not kept
    st = one_round(hmm, S, tc, book, rr, aa, what="now it takes")
    assert st["n_misses"] == in1 and st["n_inserted"] == in1
    st = one_round(hmm, S, tc, book, rr, aa, takes=[0, 0], what="nothing left to miss")
    assert st["n_misses"] == 0
    tc.close()


def test_remap_compaction_and_clear(hmm, S):
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([0, 1, 2, 3])
    one_round(hmm, S, tc, book, rr[aa != 2], aa[aa != 2], what="first round")
    one_round(hmm, S, tc, book, rr, aa, what="second round")
    before = view_equals_fresh(hmm, S, tc, "view before the remap")
    # locus 0: a permutation with haplotype 1 dropped and a new haplotype 0 in front (0 -> 3, 2 -> 1, 3 -> 2); locus 1: 3 dropped, the rest kept
    new_A, mapping = [4, 3], [3, -1, 1, 2, 0, 1, 2, -1]
    dropped = sum(1 for (l, p, h) in book.keys if mapping[4 * l + h] == -1)
    tc.remap(new_A, mapping); book.remap(new_A, mapping)
    same_state(tc, book, "after the remap")
    st = tc.stats()
    assert st["n_dead"] == dropped and dropped > 0 and st["n_segments"] == 2
    # the records follow their keys: the view is the old view's records under the new keys
    er, ea = tc.entries()
    td = tc.view()
    try:
        n, _, got = tcc.handle_content(hmm, td)
    finally:
        td.close()
    inv = [{mapping[4 * l + h]: h for h in range(4) if mapping[4 * l + h] != -1} for l in range(2)]
    old = [inv[book.locus(r)][int(a)] for r, a in zip(er, ea)]
    wn, _, want = fresh(hmm, S, er, old)
    assert n == wn == len(er)
    tcc.assert_same(got, want, "view after the remap")
    # a round in the new numbering: what was dropped misses again (here the batch is unchanged, so haplotype h of the batch is asked under
    # the keys the remap left free; the handle must still be the fresh trace of the list asked)
    free = [(l, p, h) for l in range(2) for p in sorted({k[1] for k in book.keys if k[0] == l}) for h in range(3) if (l, p, h) not in book.keys]
    assert len(free) > 0
    r2 = np.array([S.pool_off[l] + p for l, p, h in free], np.int32); a2 = np.array([h for l, p, h in free], np.int32)
    st = one_round(hmm, S, tc, book, r2, a2, what="the freed keys")
    assert st["n_misses"] == len(free) and st["n_hits"] == 0 and st["n_segments"] == 3
    # compaction: no byte of the view, no later round's handle
    v1 = view_equals_fresh_or_same(hmm, tc)
    lists = [(r2, a2), (er, ea)]
    h1 = [round_content(hmm, S, tc, r, a) for r, a in lists]
    tc.compact(); book.compact()
    same_state(tc, book, "after the compaction")
    st = tc.stats()
    assert st["n_dead"] == 0 and st["n_segments"] == 1
    tcc.assert_same(view_equals_fresh_or_same(hmm, tc), v1, "view after the compaction")
    for (r, a), h in zip(lists, h1):
        tcc.assert_same(round_content(hmm, S, tc, r, a), h, "a round after the compaction")
    tc.compact()
    assert tc.stats()["n_segments"] == 1
    # entries with a cap that is too small: 3, the count, nothing written
    n = len(tc.entries()[0])
    with pytest.raises(RuntimeError) as e:
        tc.entries(cap=n - 1)
    assert tc.rc == 3 and tc.n_entries == n and "cap is too small" in str(e.value)
    # clear, per locus and for all
    tc.clear([0, 1]); book.clear([0, 1])
    same_state(tc, book, "locus 1 cleared")
    assert np.all(tc.entries()[0] < S.pool_off[1]) and tc.stats()["n_dead"] > 0
    in1 = (rr >= S.pool_off[1]) & (aa < 3)                                # (locus 0 still holds re-keyed records: only locus 1 is asked)
    st = one_round(hmm, S, tc, book, rr[in1], aa[in1], what="after the clear of locus 1")
    assert st["n_misses"] == int(in1.sum()) > 0
    tc.clear(); book.clear()
    same_state(tc, book, "all cleared")
    assert tc.stats() == dict(n_hits=0, n_misses=0, n_inserted=0, n_segments=0, n_live=0, n_dead=0)
    st = one_round(hmm, S, tc, book, rr[aa < 3], aa[aa < 3], what="after the clear of everything")
    assert st["n_hits"] == 0
    tc.close()
    assert len(before) > 0


def view_equals_fresh_or_same(hmm, tc):
    td = tc.view()
    try:
        return tcc.handle_content(hmm, td)[2]
    finally:
        td.close()


def round_content(hmm, S, tc, rr, aa):
    td, st = tc.round(S.ptr, rr, aa, hap_to_ref=S.h2r)
    try:
        assert st["n_misses"] == 0
        return tcc.handle_content(hmm, td)[2]
    finally:
        td.close()


def test_a_round_compacts_by_itself_past_the_segment_limit(hmm, S):
    """Every round asks one key more than the last: a segment per round until the seventeenth, which trace_cache_layout.h's rule turns into
    one; the handles stay the fresh traces of their lists throughout."""
    lim = capi.trace_cache_plan(hmm)["max_segments"]
    assert lim == tcc.MAX_SEGMENTS
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([3, 0, 2, 1])
    segs = []
    for i in range(lim + 2):
        st = one_round(hmm, S, tc, book, rr[:i + 1], aa[:i + 1], what="round %d" % i)
        assert st["n_misses"] == 1 and st["n_hits"] == i and st["n_dead"] == 0
        segs.append(st["n_segments"])
    assert segs == list(range(1, lim + 1)) + [1, 2]
    view_equals_fresh(hmm, S, tc, "view after the round's own compaction")
    tc.close()


def test_a_failed_trace_leaves_the_cache_as_it_was(hmm, S):
    """The miss list holds a request whose read has no seed (req_seed -1): hipstr_hmm_trace_resident refuses it.  Return value and message
    are those the full list gets; no message of the traceback call names a request index, so there is none to translate."""
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([0, 1])
    one_round(hmm, S, tc, book, rr[::2], aa[::2], seeds=[tcc.AUTO] * len(rr[::2]), what="first round")
    er, ea = tc.entries(); st0 = tc.stats()
    seeds = np.full(len(rr), tcc.AUTO, np.int32)
    bad = int(np.nonzero(np.arange(len(rr)) % 2 == 1)[0][3])            # a miss in the middle of the list
    seeds[bad] = -1
    with pytest.raises(RuntimeError) as full:
        capi.run_trace_resident(hmm, S.ptr, rr, aa, S.h2r, req_seed=seeds)
    with pytest.raises(RuntimeError) as e:
        tc.round(S.ptr, rr, aa, hap_to_ref=S.h2r, req_seed=seeds)       # (the wrapper asserts that *td is NULL)
    assert "read without a seed base cannot be traced" in str(e.value)
    assert str(e.value).split(": ", 1)[1] == str(full.value).split(": ", 1)[1] and tc.rc == 1
    er2, ea2 = tc.entries()
    assert np.array_equal(er, er2) and np.array_equal(ea, ea2) and tc.stats() == st0
    seeds[bad] = tcc.AUTO
    one_round(hmm, S, tc, book, rr, aa, seeds=[tcc.AUTO] * len(rr), what="the same list without the bad seed")
    tc.close()


def test_refusals(hmm, S):
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([0, 1])
    one_round(hmm, S, tc, book, rr[:20], aa[:20], what="first round")
    er, ea = tc.entries(); st0 = tc.stats()

    def refused(message, rr=rr, aa=aa, ptr=S.ptr, cache=tc):
        with pytest.raises(RuntimeError) as e:
            cache.round(ptr, rr, aa, hap_to_ref=S.h2r)
        assert message in str(e.value)
    refused("request names a read outside the batch", rr=np.concatenate([rr[:3], [S.sb.n_reads]]))
    refused("request names a read outside the batch", rr=np.concatenate([[-1], rr[:3]]), aa=aa[:4])
    refused("requests must be grouped by locus, in locus order (request %d)" % (len(rr) - 1), rr=np.concatenate([rr[:-1], rr[:1]]))
    refused("request names an allele outside its locus", aa=np.concatenate([aa[:-1], [S.A]]))
    refused("request names an allele outside its locus", aa=np.concatenate([[-1], aa[1:]]))
    one = capi.SynthBatch(**dict(tcc.BATCH, n_loci=1))
    refused("n_loci of the cache disagrees with the batch", ptr=one.ptr)
    other = capi.SynthBatch(**dict(tcc.BATCH, reads_per_locus=39))
    refused("the batch's read offsets differ from the cache's pool_off", ptr=other.ptr)
    with pytest.raises(RuntimeError) as e:
        tc.remap([S.A, S.A], [0, 1, 2, 4] + [0, 1, 2, 3])
    assert "allele_mapping entry out of range at locus 0" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        tc.remap([S.A, S.A], [0, 1, 2, 3] + [0, 1, 1, 3])
    assert "two old columns mapped to one new column at locus 1" in str(e.value)
    er2, ea2 = tc.entries()
    assert np.array_equal(er, er2) and np.array_equal(ea, ea2) and tc.stats() == st0
    one.close(); other.close(); tc.close()


def test_the_consumers_read_a_round_handle_as_a_fresh_one(hmm, S):
    """hipstr_post_census_dev and hipstr_assign_trace_stats_dev on the handle of a round that mixes hits and misses and on the fresh handle of
    the same list: a read per request, two samples per locus, the batch's own blocks (the setup of tests/test_trace_resident_gpu.py's
    census on a resident handle)."""
    tc, book = new_cache(hmm, S)
    rr, aa = S.requests([0, 1, 2])
    one_round(hmm, S, tc, book, rr[1::2], aa[1::2], what="first round")
    n = len(rr); n0 = int((rr < S.pool_off[1]).sum())
    b = S.ptr.contents
    nopts = [[int(x) for x in np.ctypeslib.as_array(b.blk_nopts, shape=(6,))[3 * l:3 * l + 3]] for l in range(2)]
    A = S.A
    rng = np.random.default_rng(5)
    rows = [(-float(rng.random()), -float(rng.random()), [-float(9 * rng.random()) for _ in range(A)]) for _ in range(n)]
    pb, _ = ta.make_pb([(A, [rows[:n0 // 2], rows[n0 // 2:n0]]), (A, [rows[n0:n0 + (n - n0) // 2], rows[n0 + (n - n0) // 2:]])])
    seed = np.full(n, 5, np.int32); read_req = np.arange(n, dtype=np.int32)
    h2a = [np.concatenate([np.asarray(tcen.gray_h2a(nopts[l])[k], np.int32) for l in range(2)]) for k in range(3)]
    blk = capi.batch_arrays(S.ptr)
    starts = [int(blk["blk_start"][3 * l + 1]) for l in range(2)]; stops = [int(blk["blk_end"][3 * l + 1]) for l in range(2)]
    bp = rng.integers(-12, 13, 2 * A).astype(np.int32)
    td_round, st = tc.round(S.ptr, rr, aa, hap_to_ref=S.h2r)
    td_fresh = capi.run_trace_resident(hmm, S.ptr, rr, aa, S.h2r)
    try:
        assert st["n_hits"] > 0 and st["n_misses"] > 0
        out = []
        for td in (td_round, td_fresh):
            cen = capi.run_census(hmm, pb, S.ptr, seed, read_req, rr, None, hap_to_allele=h2a, td=td, min_frac=0.01)
            assert cen["rc"] == 0
            stats = capi.assign_trace_stats_dev(hmm, pb, read_req, td, aa, np.concatenate([np.arange(A), np.arange(A)]), bp, [A, A], starts, stops)
            out.append((cen, stats))
        (c1, s1), (c2, s2) = out
        assert c1["cand"] == c2["cand"]
        for k in tcen.KEYS:
            assert np.array_equal(c1[k], c2[k]), k
        for g, w, nm in zip(s1, s2, ("n_stutter", "n_flank_indel", "ml_bp")):
            assert np.array_equal(g, w), nm
        assert c2["n_spanning"].sum() > 0 and (s2[2] != capi.NO_ML_BP).sum() > 0
    finally:
        td_round.close(); td_fresh.close(); tc.close()
