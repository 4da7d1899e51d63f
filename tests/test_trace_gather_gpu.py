"""GPU: hipstr_trace_dev_gather (include/hipstr_hmm.h; hipstr_amd/csrc/trace_cache.hip) — a new resident handle whose record q is record
out_idx[q] of src[out_src[q]].

Yardstick: hipstr_trace_dev_fetch(HIPSTR_TRACE_F_ALL) of the result against the sources' fetches re-ordered in numpy
(tests/trace_cache_cases.py: reorder), byte for byte: every scalar array, the seven offset arrays with their leading zeros, the ten pool
arrays, hipstr_trace_dev_sizes.  The sources' bytes must be what they were afterwards.

Sources: two hipstr_hmm_trace_resident handles on the batch of tests/trace_cache_cases.py — A (every other read, all alleles) with the
hap_to_ref strings, B (the reads between) without them (every cigar and alignment-string piece of B is empty) — and an empty handle.  test_the_sources_hold_short_and_long_pieces asserts what
they hold.  What a traceback cannot produce is not asserted: hap_aln always holds the seed's 'M' (no empty piece), and a read has a handful
of indel records, SNPs and CIGAR runs (no piece of more than 64 in the three pools with 32-bit arrays; their copy loop is the one the byte
pools take past 64 elements).

n_out = 0, 1, 32, 33, 63, 64, 65, 130 put the scan's carry on either side of a wavefront for the one-piece pools (64 pieces) and for the
flank pool (two pieces a record: 32 records).

A pool above INT32_MAX elements: test_a_pool_above_int32_max_is_refused repeats the record with the longest alignment string until the
pool's total passes 2^31 - 1.  The call refuses between the scan and the result's block, so what the case costs is the request lists and
the scan's scratch, no result.  Not run here: sources of two devices (the suite has one device).
No case provokes a fault: every refusal is decided on the host, from the arguments or from the pool totals the scan brought home, before
anything is written outside the call's own scratch."""
import numpy as np
import pytest

from hipstr_amd import capi
import trace_cache_cases as tcc

pytestmark = pytest.mark.gpu
N_OUT = [0, 1, 32, 33, 63, 64, 65, 130]


class Sources:
    def __init__(self, hmm, oracle):
        self.s = tcc.Setup(hmm, oracle)
        every = [0, 1, 2, 3]
        ra, aa = self.s.requests(every, self.s.reads[0::2]); rb, ab = self.s.requests(every, self.s.reads[1::2])
        self.tds = [capi.run_trace_resident(hmm, self.s.ptr, ra, aa, self.s.h2r), capi.run_trace_resident(hmm, self.s.ptr, rb, ab, None),
                    capi.run_trace_resident(hmm, self.s.ptr, [], [], self.s.h2r)]
        self.fetched = [tcc.fetch(hmm, td) for td in self.tds]          # (n, totals, keep): fetched once, never changed
        self.before = [tcc.content(n, keep) for n, _, keep in self.fetched]
        self.src = [(n, keep) for n, _, keep in self.fetched]
        self.n = [n for n, _, _ in self.fetched]

    def close(self):
        for td in self.tds:
            td.close()
        self.s.close()


@pytest.fixture(scope="module")
def S(hmm, oracle):
    s = Sources(hmm, oracle)
    yield s
    s.close()


def check(hmm, S, out_src, out_idx, what):
    td = capi.trace_dev_gather(hmm, S.tds, out_src, out_idx)
    try:
        n, tot, got = tcc.handle_content(hmm, td)
    finally:
        td.close()
    want_tot, want = tcc.reorder(S.src, list(out_src), list(out_idx))
    assert n == len(out_src), what
    assert np.array_equal(tot, want_tot), what
    tcc.assert_same(got, want, what)
    for i, td in enumerate(S.tds):                                      # a source is never modified
        m, _, now = tcc.handle_content(hmm, td)
        assert m == S.n[i]
        tcc.assert_same(now, S.before[i], what + ": source %d changed" % i)


def test_the_sources_hold_short_and_long_pieces(S):
    """A condition on the inputs, not on the code under test."""
    assert S.n[0] >= 130 and S.n[1] >= 130 and S.n[2] == 0
    lens = []
    for p, (off, per, _) in enumerate(tcc.POOLS):
        d = np.concatenate([np.diff(keep[off][:per * n + 1]) for n, keep in S.src[:2]])
        lens.append((int(d.min()), int(d.max())))
    empty = [lo == 0 for lo, _ in lens]; long_ = [hi > 64 for _, hi in lens]
    assert empty == [False, True, True, True, True, True, True], lens            # hap_aln: never empty
    assert long_ == [True, True, True, False, False, False, True], lens          # indel, snp, cigar: a handful per read
    assert lens[3][1] >= 1 and lens[4][1] >= 1 and lens[5][1] >= 2
    found = 0
    for n, keep in S.src[:2]:
        nostr = np.nonzero(keep["stutter_size"][:n] == tcc.NO_STR)[0]
        assert all(keep["str_seq_off"][q] == keep["str_seq_off"][q + 1] for q in nostr)
        found += len(nostr)
    assert found >= 1


@pytest.mark.parametrize("n_out", N_OUT)
def test_prefix_of_the_first_source(hmm, S, n_out):
    check(hmm, S, [0] * n_out, list(range(n_out)), "first %d" % n_out)


@pytest.mark.parametrize("n_out", N_OUT)
def test_alternating_sources_at_every_size(hmm, S, n_out):
    """Records drawn alternately from both sources, a stride through each so that short and long pieces meet at the carry."""
    src = [q % 2 for q in range(n_out)]; idx = [(7 * q) % S.n[q % 2] for q in range(n_out)]
    check(hmm, S, src, idx, "alternating %d" % n_out)


def test_identity(hmm, S):
    check(hmm, S, [0] * S.n[0], list(range(S.n[0])), "identity")


def test_reversed(hmm, S):
    check(hmm, S, [0] * S.n[0], list(range(S.n[0]))[::-1], "reversed")


def test_every_record_twice(hmm, S):
    check(hmm, S, [0] * (2 * S.n[0]), [q // 2 for q in range(2 * S.n[0])], "every record twice")


def test_everything_from_the_second_source_with_the_empty_handle_in_the_list(hmm, S):
    check(hmm, S, [1] * S.n[1], list(range(S.n[1])), "second source")


def test_an_empty_gather_of_no_sources(hmm):
    td = capi.trace_dev_gather(hmm, [], [], [])
    try:
        n, tot, keep = tcc.fetch(hmm, td)
        assert n == 0 and not tot.any()
        for off, _, _ in tcc.POOLS:
            assert int(keep[off][0]) == 0
    finally:
        td.close()


def test_a_gathered_handle_is_a_source(hmm, S):
    one = capi.trace_dev_gather(hmm, S.tds, [1, 0, 1], [5, 3, 0])
    try:
        two = capi.trace_dev_gather(hmm, [one, S.tds[0]], [0, 1, 0], [2, 9, 1])
        try:
            n, _, got = tcc.handle_content(hmm, two)
        finally:
            two.close()
    finally:
        one.close()
    _, want = tcc.reorder(S.src, [1, 0, 0], [0, 9, 3])
    assert n == 3
    tcc.assert_same(got, want, "gather of a gather")


@pytest.mark.parametrize("case, message", [
    ("n_src", "negative count"), ("n_out", "negative count"), ("null", "null source 1"), ("from_host", "source 1 lacks a group or was not made by the library"),
    ("src_hi", "out_src out of range at record 1"), ("src_lo", "out_src out of range at record 0"), ("idx_hi", "out_idx out of range at record 2"),
    ("idx_lo", "out_idx out of range at record 0"), ("idx_empty", "out_idx out of range at record 0"),
])
def test_refusals(hmm, S, case, message):
    srcs = list(S.tds); os_, oi, kw = [0, 1, 0], [0, 1, 2], {}
    fake = None
    if case == "n_src":
        kw = dict(n_src=-1)
    elif case == "n_out":
        kw = dict(n_out=-1)
    elif case == "null":
        srcs[1] = None
    elif case == "from_host":
        n, keep = S.src[1]
        fake = capi.trace_dev_from_host(hmm, {k: v for k, v in keep.items() if k != "str_seq"}, n)      # a handle that lacks a group
        srcs[1] = fake
    elif case == "src_hi":
        os_ = [0, 3, 0]
    elif case == "src_lo":
        os_ = [-1, 1, 0]
    elif case == "idx_hi":
        oi = [0, 1, S.n[0]]
    elif case == "idx_lo":
        oi = [-1, 1, 2]
    elif case == "idx_empty":
        os_ = [2, 1, 0]                                                 # the empty handle has no record 0
    try:
        with pytest.raises(RuntimeError) as e:
            capi.trace_dev_gather(hmm, srcs, os_, oi, **kw)             # (the wrapper asserts that *td is NULL after a refusal)
        assert message in str(e.value)
    finally:
        if fake is not None:
            fake.close()
    for i, td in enumerate(S.tds):
        tcc.assert_same(tcc.handle_content(hmm, td)[2], S.before[i], "source %d after a refusal" % i)


def test_a_pool_above_int32_max_is_refused(hmm, S):
    """The record of the first source with the longest alignment string, as often as it takes to pass INT32_MAX elements in that pool
    (repeats are allowed): the text of hipstr_hmm_trace_resident, no handle, the sources as they were.  The total is formed past 2^31
    by the scan's 64-bit carry; one below the count used here the pool would still fit."""
    n, keep = S.src[0]
    lens = np.diff(keep["aln_str_off"][:n + 1].astype(np.int64))
    i = int(lens.argmax()); length = int(lens[i])
    assert length > 64
    n_out = (2 ** 31 - 1) // length + 1
    assert (n_out - 1) * length <= 2 ** 31 - 1 < n_out * length and n_out < 2 ** 31 - 1
    with pytest.raises(RuntimeError) as e:
        capi.trace_dev_gather(hmm, S.tds, np.zeros(n_out, np.int32), np.full(n_out, i, np.int32))      # (the wrapper asserts that *td is NULL)
    assert "too many requests for one call; split the request list" in str(e.value)
    for k, td in enumerate(S.tds):
        m, _, now = tcc.handle_content(hmm, td)
        assert m == S.n[k]
        tcc.assert_same(now, S.before[k], "source %d after the refusal" % k)
    hmm.hipstr_hmm_trim()                                               # the scan's scratch (a gigabyte) goes back to the driver


def test_a_complete_handle_from_host_arrays_is_refused_too(hmm, S):
    """hipstr_debug_trace_dev_from_host checks nothing: its offsets may descend, so the gather does not read them."""
    n, keep = S.src[0]
    fake = capi.trace_dev_from_host(hmm, keep, n)
    try:
        with pytest.raises(RuntimeError) as e:
            capi.trace_dev_gather(hmm, [fake], [0], [0])
        assert "was not made by the library" in str(e.value)
    finally:
        fake.close()
