"""GPU: hipstr_post_census — the stutter-candidate alleles of a round and the called / spanned marks of its options, on the resident
posteriors (include/hipstr_hmm.h).

The yardstick is `restate` (tests/flow_chain.py, shared with the end-to-end chain): a line-by-line Python restatement of SeqStutterGenotyper::get_stutter_candidate_alleles (reference
src/seq_stutter_genotyper.cpp:843-879, with :582-584 for the order and the new haplotype count) and of get_unused_alleles (:229-315) — dicts,
sets, sorted(key=lambda s: (len(s), s)), and Python floats for the one division of :869 and the one fabs of :282.  LIMITATION: the compiled
reference cannot provide goldens for this stage — both functions are private members reached only from inside genotype() — so the expected
values come from this restatement and not from the reference's own binary (tests/test_assign_gpu.py does the same, for the same reason).
The restatement is fed the oracle's MAP pairs (test_assign_gpu.oracle_map).  Every comparison is exact: integers, bytes and flags.

Trace fields are plain arrays, so every case but the chained one fabricates them.

One case of the issue's list cannot be built: "sample labels interleaved, not sorted".  The census takes the sample of a read from the
posterior run, and hipstr_post_upload refuses a batch whose reads are not grouped by ascending sample label (genotyper.h:112-119), as
test_spanning_is_strict asserts; what can be interleaved — the requests of the samples, and the reads of a sample across the requests — is."""
import numpy as np
import pytest

from hipstr_amd import capi
import test_assign_gpu as ta
import test_readmat_gpu as trm

pytestmark = pytest.mark.gpu

NO_STR = -100000                      # HIPSTR_NO_STR_DATA
TOLERANCE = 1e-10                     # mathops.cpp:10
FILL = capi.CENSUS_FILL
DUMMY = dict(seq="A", qual="I", start=0, cigar=[("=", 1)])          # a pooled read: the census reads only read_off of the pooled batch
LFLANK, RFLANK = (60, 100, ["ACGTACGT"]), (120, 160, ["TTGACCGT"])
STR2 = (100, 120, ["ACAC", "ACACAC"])
SPAN, SHORT_L, SHORT_R = (50, 200), (100, 200), (50, 120)           # (aln_start, aln_stop) against a block of [100, 120)


# gray_h2a, Locus, Case (shared with the end-to-end chain): tests/flow_chain.py
from flow_chain import gray_h2a, Locus, Case, census_restate as restate  # noqa: E402,F401


def batch_of(loci):
    b = capi.Batch()
    for L in loci:
        b.add_locus(L.blocks, 4, [0.9, 0.05, 0.05, 0.9, 0.01, 0.01], [DUMMY] * L.n_pooled)
    return b.finalize()


def build(loci):
    c = Case(); c.loci = loci
    c.batch = batch_of(loci)
    c.pb, c.LL = ta.make_pb([(L.A, [[(r[0], r[1], r[2]) for r in s] for s in L.samples]) for L in loci], haploid=[L.haploid for L in loci])
    c.seed = np.array([r[3] for L in loci for s in L.samples for r in s], np.int32)
    pool_off = np.concatenate([[0], np.cumsum([L.n_pooled for L in loci])]); req_off = np.concatenate([[0], np.cumsum([len(L.reqs) for L in loci])])
    c.read_req = np.array([(-1 if r[4] < 0 else int(req_off[l]) + r[4]) for l, L in enumerate(loci) for s in L.samples for r in s], np.int32)
    c.req_read = np.array([int(pool_off[l]) + q[0] for l, L in enumerate(loci) for q in L.reqs], np.int32)
    qs = [q for L in loci for q in L.reqs]
    c.trace = capi.census_trace([q[1] for q in qs], [q[2] for q in qs], [q[3] for q in qs], [q[4] for q in qs])
    c.h2a = [np.array([v for L in loci for v in L.h2a[k]], np.int32) for k in range(3)]
    c.pool_off = pool_off
    return c


KEYS = ("cand_off", "cand_req", "new_n_haps", "n_spanning", "n_span_stutter", "called", "spanned")


def compare(got, want, what):
    assert got["rc"] == 0, what
    assert got["cand"] == want["cand"], "%s: candidates\n got %r\nwant %r" % (what, got["cand"], want["cand"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s\n got %r\nwant %r" % (what, k, got[k], want[k])


def run(hmm, c, h2a=None, dev_ll=None, pb=None, **kw):
    return capi.run_census(hmm, c.pb if pb is None else pb, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace,
                           hap_to_allele=c.h2a if h2a is None else h2a, dev_ll=dev_ll, **kw)


def check(hmm, oracle, c, what, **kw):
    mg = ta.oracle_map(oracle, c.pb)
    got = run(hmm, c, **kw)
    want = restate(c, mg, **{k: v for k, v in kw.items() if k in ("h2a", "uncallable", "min_reads", "min_frac")})
    compare(got, want, what)
    return got, want


def reads_of(A, fav, n, req, seed=5, p=(-0.5, -0.5)):
    """n reads that favour haplotype `fav`, all on request `req` (a list: cycled)."""
    reqs = req if isinstance(req, (list, tuple)) else [req]
    return [(p[0], p[1], [(-1.0 if k == fav else -30.0) - 0.01 * k for k in range(A)], seed, reqs[i % len(reqs)]) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------ 1. thresholds
RATIOS = [(1, 1), (2, 2), (2, 13), (2, 14), (3, 20), (3, 21), (6, 40)]


def thresholds_case():
    loci = []
    for cnt, n in RATIOS:
        reqs = [(0, SPAN[0], SPAN[1], -4, b"AC"), (1, SPAN[0], SPAN[1], 0, b"ACAC")]
        loci.append(Locus([LFLANK, STR2, RFLANK], [reads_of(2, 0, cnt, 0) + reads_of(2, 0, n - cnt, 1)], reqs))
    return build(loci)


@pytest.mark.parametrize("min_reads,min_frac,expect", [(0, 0.0, [0, 1, 1, 0, 1, 0, 1]), (3, 0.1, [0, 0, 0, 0, 1, 1, 1]), (1, 0.5, [1, 1, 0, 0, 0, 0, 0])],
                         ids=["defaults", "3_reads_a_tenth", "1_read_a_half"])
def test_thresholds(hmm, oracle, min_reads, min_frac, expect):
    """count / spanning of 1/1, 2/2, 2/13, 2/14, 3/20, 3/21, 6/40 — 3/20 and 6/40 are exactly the double 0.15 — one sample per locus."""
    assert 3 / 20 == 0.15 and 6 / 40 == 0.15 and 2 / 13 > 0.15 > 2 / 14 and 3 / 21 < 0.15
    c = thresholds_case()
    mg = ta.oracle_map(oracle, c.pb)
    got = run(hmm, c, min_reads=min_reads, min_frac=min_frac)
    want = restate(c, mg, min_reads=min_reads or 2, min_frac=min_frac or 0.15)
    compare(got, want, "thresholds")
    assert [len(x) for x in got["cand"]] == expect
    assert list(got["n_spanning"]) == [n for _, n in RATIOS] and list(got["n_span_stutter"]) == [k for k, _ in RATIOS]
    assert list(got["new_n_haps"]) == [2 + e for e in expect]


# ------------------------------------------------------------------------------------------------------------------ 2. content, not request
def content_case():
    two = [(0, SPAN[0], SPAN[1], -4, b"ACACACAC"), (1, SPAN[0], SPAN[1], 4, b"ACACACAC")]        # two pools, two haplotypes, one string
    same_sample = Locus([LFLANK, STR2, RFLANK], [reads_of(2, 0, 1, 0) + reads_of(2, 1, 1, 1)], two)
    two_samples = Locus([LFLANK, STR2, RFLANK], [reads_of(2, 0, 1, 0), reads_of(2, 1, 1, 1)], two)
    both_qualify = Locus([LFLANK, STR2, RFLANK], [reads_of(2, 0, 2, [0, 1]), reads_of(2, 1, 2, [1, 0])], two)
    return build([same_sample, two_samples, both_qualify])


def test_the_key_is_the_content_not_the_request(hmm, oracle):
    """Two requests of different pools with one str_seq, one read each: a candidate when the reads share a sample (a count of 2 — formed per
    request it would be 1 and 1), none when they do not; a string that qualifies in two samples appears once."""
    c = content_case()
    got, want = check(hmm, oracle, c, "content")
    assert got["cand"] == [[b"ACACACAC"], [], [b"ACACACAC"]] and list(got["cand_req"]) == [0, 4]
    assert list(got["n_spanning"]) == [2, 1, 1, 2, 2]


# ------------------------------------------------------------------------------------------------------------------ 3. string equality and order
def strings_case():
    opts = ["ACAC", "ACACAC", "ACACACACAC"]
    flank = (60, 100, ["ACGTACGT", "GGGTACGT"])
    big = b"AC" * 1023 + b"A"
    strs = [b"A" * 63 + b"C", b"C" + b"A" * 63, b"A" * 64, b"A" * 63 + b"G",        # equal lengths, first / last byte differs
            b"ACG", b"ACGT", b"", b"T", b"T" * 63, b"T" * 65, big, big[:-1] + b"C",
            b"ACAC", b"ACACACACAC", b"GGGTACGT",                                    # option 0, the last option (excluded); a flank option (kept)
            b"A" * 64, b"", big, b"ACG"]                                            # repeats at higher request numbers
    assert sorted({len(s) for s in strs} & {1, 63, 64, 65, 2047}) == [1, 63, 64, 65, 2047]
    reqs = [(i, SPAN[0], SPAN[1], 2 if i % 2 else -2, s) for i, s in enumerate(strs)]
    reads = reads_of(6, 0, 2 * len(strs), [i // 2 for i in range(2 * len(strs))])
    l0 = Locus([flank, (100, 120, opts), RFLANK], [reads], reqs)
    order = [b"AC", b"A", b"CA", b"AA"]
    l1 = Locus([LFLANK, STR2, RFLANK], [reads_of(2, 1, 8, [0, 0, 1, 1, 2, 2, 3, 3])], [(i, SPAN[0], SPAN[1], -2, s) for i, s in enumerate(order)])
    return build([l0, l1]), strs


def test_string_equality_and_order(hmm, oracle):
    c, strs = strings_case()
    got, want = check(hmm, oracle, c, "strings", min_frac=1e-6)
    assert got["cand"][1] == [b"A", b"AA", b"AC", b"CA"]
    kept = sorted(set(strs) - {b"ACAC", b"ACACACACAC"}, key=lambda s: (len(s), s))
    assert got["cand"][0] == kept and b"GGGTACGT" in kept and b"" in kept
    assert list(got["cand_req"][:len(kept)]) == [strs.index(s) for s in kept]                  # the lowest request with that content


# ------------------------------------------------------------------------------------------------------------------ 4. spanning is strict
def strict_case():
    reqs = [(0, SHORT_L[0], SHORT_L[1], -4, b"AC"),          # aln_start == blk_start: does not span
            (1, SHORT_R[0], SHORT_R[1], -4, b"AC"),          # aln_stop == blk_end: does not span
            (2, 99, 121, -4, b"AC"),                         # spans by one base either side, stutter
            (3, 99, 121, 0, b"ACAC"),                        # spans, no stutter: the denominator only
            (4, 99, 121, 2, b"ACACACAC")]
    # the reads of a sample interleave the requests; the requests interleave the samples
    s0 = reads_of(2, 0, 10, [2, 0, 3, 1, 2, 0, 3, 4, 3, 3])
    s1 = reads_of(2, 1, 9, [4, 2, 1, 4, 0, 3, 2, 4, 3])
    s1[1] = s1[1][:3] + (-1, 2)                              # seed < 0: counts nowhere
    s1[6] = s1[6][:4] + (-1,)                                # read_req == -1: counts nowhere
    return build([Locus([LFLANK, STR2, RFLANK], [s0, s1], reqs)])


def test_spanning_is_strict(hmm, oracle):
    c = strict_case()
    got, want = check(hmm, oracle, c, "strict")
    assert list(got["n_spanning"]) == [7, 5] and list(got["n_span_stutter"]) == [3, 3]
    assert got["cand"] == [[b"AC", b"ACACACAC"]]
    # the one case that cannot be built: reads of a locus not grouped by ascending sample label are refused at upload
    a = c.pb.a; lab = a["sample_label"].copy(); lab[[0, 12]] = lab[[12, 0]]
    bad = capi.PostBatch(a["n_alleles"], a["n_samples"], a["read_off"], lab, a["log_p1"], a["log_p2"], a["read_weight"], a["log_aln_probs"])
    assert not hmm.hipstr_post_upload(bad.ptr, None) and b"grouped by ascending sample label" in hmm.hipstr_last_error()


# ------------------------------------------------------------------------------------------------------------------ 5. called
def called_case():
    lf = (60, 100, ["ACGTACGT", "ACGAACGT"]); rf = (120, 160, ["TTGACCGT", "TTGACCGA", "TAGACCGT"])
    A = 12
    req = [(0, SPAN[0], SPAN[1], 0, b"ACAC")]
    inf = [(-0.2, -0.6, [-np.inf] * A, 5, 0) for _ in range(4)]
    samples = [reads_of(A, 3, 5, 0, seed=-1),                # every read without a seed
               reads_of(A, 7, 5, 0),                         # uncallable
               inf,                                          # no MAP pair
               reads_of(A, 10, 6, 0),                        # homozygous
               reads_of(A, 2, 4, 0) + reads_of(A, 9, 4, 0)]  # heterozygous
    return build([Locus([lf, STR2, rf], samples, req)])


def test_called(hmm, oracle):
    c = called_case()
    mg = ta.oracle_map(oracle, c.pb)
    assert tuple(mg[2]) == (-1, -1) and tuple(mg[3]) == (10, 10) and sorted(mg[4]) == [2, 9] and mg[0][0] >= 0
    unc = [0, 1, 0, 0, 0]
    got = run(hmm, c, sample_uncallable=unc)
    want = restate(c, mg, uncallable=unc)
    compare(got, want, "called, three blocks")
    h = c.loci[0].h2a
    marks = [sorted({h[k][x] for x in (10, 2, 9)}) for k in range(3)]
    assert [list(np.nonzero(got["called"][o:o + n])[0]) for o, n in ((0, 2), (2, 2), (4, 3))] == marks
    # every sample callable: the uncallable one's pair joins
    compare(run(hmm, c), restate(c, mg), "called, all callable")
    # a NULL block keeps its bytes: run_census pre-fills called / spanned with 0xAA
    h2a = [c.h2a[0], None, c.h2a[2]]
    got = run(hmm, c, h2a=h2a, sample_uncallable=unc)
    compare(got, restate(c, mg, h2a=h2a, uncallable=unc), "called, block 1 not wanted")
    assert np.all(got["called"][2:4] == FILL) and np.all(got["spanned"] == FILL) and np.all(got["called"][[0, 1, 4, 5, 6]] != FILL)


# ------------------------------------------------------------------------------------------------------------------ 6. spanned, the third rule
PROBES = [("haploid", (-0.2, -0.9, [-1.0, -3.0])), ("equal", (0.0, 0.0, [-1.0, -1.0])),
          ("+0.5e-10", (0.0, 0.0, [-1.0, -1.0 - 0.5e-10])), ("-0.5e-10", (0.0, 0.0, [-1.0 - 0.5e-10, -1.0])),
          ("+2e-10", (0.0, 0.0, [-1.0, -1.0 - 2e-10])), ("-2e-10", (0.0, 0.0, [-1.0 - 2e-10, -1.0])),
          ("hom", (-0.3, -0.1, [-1.0, -50.0]))]
PICK = dict([("haploid", 0), ("equal", 0), ("+0.5e-10", 0), ("-0.5e-10", 0), ("+2e-10", 0), ("-2e-10", 1), ("hom", 0)])


def spanned_case():
    """One locus per probe read: anchors without a trace fix the MAP pair, the probe is the only read with a spanning, stutter-free trace."""
    loci = []
    for name, (a, b, row) in PROBES:
        if name in ("haploid", "hom"):
            anchors = [(-1.0, -1.0, [-1.0, -50.0], 5, -1)] * 4
        else:
            anchors = [(x, y, r, 5, -1) for x, y, r in ta.ANCHORS]
        loci.append(Locus([LFLANK, STR2, RFLANK], [anchors + [(a, b, row, 5, 0)]], [(0, SPAN[0], SPAN[1], 0, b"ACAC")], haploid=1 if name == "haploid" else 0))
    return build(loci)


@pytest.mark.parametrize("where", ["host_array", "resident_matrix"])
def test_spanned_with_the_third_rule(hmm, oracle, where):
    c = spanned_case()
    mg = ta.oracle_map(oracle, c.pb)
    assert [tuple(x) for x in mg] == [(0, 0), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 0)]
    want = restate(c, mg)
    a = c.pb.a; n = len(c.seed)
    # the read on which retrace_alignments' rule and this one disagree: inside the tolerance with the second term not smaller
    probe = int(a["read_off"][4]) - 1
    assert PROBES[3][0] == "-0.5e-10"
    retrace = capi.run_assign(hmm, c.pb, c.seed, rule=capi.ASSIGN_RETRACE)
    assert retrace["best_hap"][probe] == 1 and PICK["-0.5e-10"] == 0
    if where == "host_array":
        got = run(hmm, c)
    else:
        rm = capi.ReadMatrix(hmm, a["n_alleles"], a["read_off"], np.zeros(n, np.int32), init_ll=c.LL, init_seeds=c.seed)
        try:
            pb = capi.PostBatch(a["n_alleles"], a["n_samples"], a["read_off"], a["sample_label"], a["log_p1"], a["log_p2"], a["read_weight"], None,
                                haploid=a["haploid"])
            got = run(hmm, c, pb=pb, dev_ll=rm.dev_ll)
        finally:
            rm.close()
    compare(got, want, "spanned, " + where)
    for l, (name, _) in enumerate(PROBES):
        sp = got["spanned"][4 * l + 1:4 * l + 3]                       # block 1's two options (identity map: one flank option each)
        assert list(sp) == ([1, 0] if PICK[name] == 0 else [0, 1]), name


# ------------------------------------------------------------------------------------------------------------------ 7. routes and size edges
def route_cases(hmm):
    """(name, requests, reads, route) from the library's own thresholds."""
    t = capi.census_plan(hmm, 0, 0)["thresholds"]
    wq, wr, lds, ri, wg = t["HS_CENSUS_WAVE_REQS"], t["HS_CENSUS_WAVE_READS"], t["HS_CENSUS_LDS_INTS"], t["HS_CENSUS_REQ_INTS"], t["HS_CENSUS_THREADS"]
    assert wr == wg                                                     # the wavefront route ends at the workgroup's width
    cases = [("reads_%d" % r, 3, r, "wave") for r in (0, 1, 63, 64, 65, wg)] + [("reads_%d" % (wg + 1), 3, wg + 1, "lds")]
    cases += [("requests_%d" % wq, wq, 10, "wave"), ("requests_%d" % (wq + 1), wq + 1, 10, "lds")]
    q = (lds - 1) // ri; r = lds - 1 - ri * q                           # the fullest LDS workspace in requests
    cases += [("lds_full_requests", q, r, "lds"), ("global_one_more_key", q, r + 1, "global"), ("global_one_more_request", q + 1, 0, "global")]
    r = lds - 1 - ri                                                    # ... and in reads, with one request
    cases += [("lds_full_reads", 1, r, "lds"), ("global_one_more_read", 1, r + 1, "global")]
    return cases


# hs_census_route has no other limit; what the cases cannot reach:
UNREACHABLE = (("too many (sample, request) pairs in a locus", "refused from 2^31 pairs on: a request list of that size does not fit a test"),)


def route_locus(n_req, n_reads, rng, n_samp=2):
    pool_strs = [b"AC", b"ACACAC", b"ACACACAC", b"A" * 40, b"A" * 39 + b"C", b"", b"ACAC"]
    reqs = []
    for i in range(n_req):
        st, sp = (SPAN if rng.random() < 0.8 else (SHORT_L if rng.random() < 0.5 else SHORT_R))
        reqs.append((i, st, sp, int(rng.choice([0, 0, -4, 4, 2])), pool_strs[int(rng.integers(len(pool_strs)))]))
    # the first three always bite: two requests with one content and stutter, one without stutter
    reqs[:3] = [(0, SPAN[0], SPAN[1], -4, b"ACACACAC"), (1, SPAN[0], SPAN[1], 0, b"ACAC"), (2, SPAN[0], SPAN[1], 4, b"ACACACAC")][:n_req]
    per = [n_reads // n_samp + (1 if s < n_reads % n_samp else 0) for s in range(n_samp)]
    samples = []
    for s in range(n_samp):
        rows = []
        for i in range(per[s]):
            fav = int(rng.integers(2))
            rows.append((-float(rng.random()), -float(rng.random()), [(-1.0 if k == fav else -9.0) - float(rng.random()) for k in range(2)],
                         -1 if rng.random() < 0.1 else 4, int(rng.integers(-1, n_req)) if n_req else -1))
        samples.append(rows)
    return Locus([LFLANK, STR2, RFLANK], samples, reqs, n_pooled=n_req)


def test_route_cases_name_every_route(hmm_host):
    cases = route_cases(hmm_host)
    assert {c[3] for c in cases} == set(capi.CENSUS_ROUTES) and len(UNREACHABLE) == 1
    for name, nq, nr, route in cases:
        assert capi.census_plan(hmm_host, nq, nr)["route"] == route, name


@pytest.mark.parametrize("idx", range(14))
def test_route_and_size_edges(hmm, oracle, idx):
    cases = route_cases(hmm)
    assert len(cases) == 14
    name, nq, nr, route = cases[idx]
    assert capi.census_plan(hmm, nq, nr)["route"] == route
    c = build([route_locus(nq, nr, np.random.default_rng(100 + idx))])
    got, want = check(hmm, oracle, c, name, min_frac=0.02)
    if nr >= 63:
        assert want["n_span_stutter"].sum() > 0 and (nq < 3 or want["spanned"][1:3].sum() > 0)


def mixed_case(hmm):
    """All three routes in one batch, with empty loci (no reads, no requests, no pooled reads) between and around them."""
    t = capi.census_plan(hmm, 0, 0)["thresholds"]
    rng = np.random.default_rng(7)
    shapes = [(0, 0), (5, 40), (0, 0), (t["HS_CENSUS_WAVE_REQS"] + 6, 300), (0, 0), ((t["HS_CENSUS_LDS_INTS"] - 1) // t["HS_CENSUS_REQ_INTS"] + 1, 70), (9, 33), (0, 0)]
    routes = [capi.census_plan(hmm, q, r)["route"] for q, r in shapes]
    assert routes == ["wave", "wave", "wave", "lds", "wave", "global", "wave", "wave"]
    return build([route_locus(q, r, rng) for q, r in shapes])


def test_mixed_routes_with_empty_loci(hmm, oracle):
    c = mixed_case(hmm)
    got, want = check(hmm, oracle, c, "mixed", min_frac=0.02)
    assert sum(len(x) for x in want["cand"]) >= 1 and [len(x) for x in want["cand"]][0] == 0


# ------------------------------------------------------------------------------------------------------------------ 8. chained
class Chain:
    pass


def chain_inputs(hmm, oracle):
    """Two small pooled loci (tests/test_readmat_gpu.py's builder), the oracle's likelihoods scattered on the host, the oracle's MAP pairs."""
    k = Chain()
    shapes = [(1, 4), (2, 3)]; reads = [26, 18]; k.n_pools = [9, 7]
    rng = np.random.default_rng(11)
    k.b = trm.pooled_batch(shapes, k.n_pools, [None, None])
    k.A = np.array([a * s for a, s in shapes], np.int32)
    k.read_off = np.concatenate([[0], np.cumsum(reads)]).astype(np.int32); k.pool_off = np.concatenate([[0], np.cumsum(k.n_pools)]).astype(np.int32)
    k.pool = np.concatenate([np.concatenate([np.arange(P), rng.integers(0, P, R - P)]) for P, R in zip(k.n_pools, reads)]).astype(np.int32)
    k.n = int(k.read_off[-1])
    lab = np.concatenate([np.sort(rng.integers(0, 2, r)) for r in reads]).astype(np.int32)
    k.kw = dict(n_alleles=k.A, n_samples=np.full(2, 2), read_off=k.read_off, sample_label=lab, log_p1=-rng.random(k.n), log_p2=-rng.random(k.n),
                read_weight=np.ones(k.n, np.int32))
    ll, seeds = capi.run_align(oracle, "oracle_", k.b.ptr)
    k.M = np.full(int((np.diff(k.read_off) * k.A).sum()), trm.UNALIGNED); k.seeds = np.full(k.n, -1, np.int32)
    trm.host_scatter(k.M, k.seeds, k.A, k.read_off, k.pool, np.zeros(k.n, np.uint8), np.ones(k.n, bool), ll, seeds, k.pool_off, [None, None])
    k.pb = capi.PostBatch(log_aln_probs=k.M, **k.kw)
    k.mg = ta.oracle_map(oracle, k.pb)
    # the restatement's view of the loci
    b = k.b.arrays; k.loci = []; o = 0
    for l in range(2):
        blocks = []
        for j in range(3):
            no = int(b["blk_nopts"][3 * l + j])
            blocks.append((int(b["blk_start"][3 * l + j]), int(b["blk_end"][3 * l + j]), [b["seq"][b["opt_off"][o + i]:b["opt_off"][o + i + 1]].decode() for i in range(no)]))
            o += no
        L = Locus(blocks, [[None] * int((lab[k.read_off[l]:k.read_off[l + 1]] == s).sum()) for s in range(2)], [], n_pooled=k.n_pools[l])
        k.loci.append(L)
    k.h2a = [np.array([v for L in k.loci for v in L.h2a[j]], np.int32) for j in range(3)]
    return k


def run_chain(hmm, k):
    """forward -> hipstr_rm_scatter -> posteriors -> hipstr_post_assign(RETRACE) -> hipstr_hmm_trace (flags 0) -> census, the matrix resident."""
    dev = trm.upload_and_align(hmm, k.b); rm = None; pd = None
    try:
        rm = capi.ReadMatrix(hmm, k.A, k.read_off, k.pool)
        rm.scatter(dev)
        pb = capi.PostBatch(log_aln_probs=None, **k.kw)
        pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error().decode()
        assert hmm.hipstr_post_launch(pd, None) == 0
        asg = capi.run_assign(hmm, pd, k.seeds, pool_index=k.pool, pool_off=k.pool_off, rule=capi.ASSIGN_RETRACE, n_reads=k.n, n_samp=4)
        assert asg["rc"] == 0 and asg["n_req"] > 0
        h2r = capi.hap_aln_info(hmm, "hipstr_", k.b.ptr)
        tr = capi.run_trace(hmm, "hipstr_hmm_", k.b.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, unpack=False, cap=1 << 16, flags=0)
        got = capi.run_census(hmm, pd, k.b.ptr, k.seeds, asg["read_req"], asg["req_read"], tr, hap_to_allele=k.h2a, n_samp=4, min_frac=0.01)
    finally:
        if pd:
            hmm.hipstr_post_free(pd)
        if rm:
            rm.close()
        hmm.hipstr_hmm_free(dev)
    return got, asg, tr


def chain_want(k, asg, tr):
    c = Case(); c.loci = k.loci; c.pb = k.pb; c.pool_off = k.pool_off; c.h2a = k.h2a
    return restate(c, k.mg, min_frac=0.01, LL=k.M, trace=tr, read_req=asg["read_req"], req_read=asg["req_read"], seed=k.seeds)


def test_chained_on_the_resident_matrix(hmm, oracle):
    k = chain_inputs(hmm, oracle)
    got, asg, tr = run_chain(hmm, k)
    want = chain_want(k, asg, tr)
    compare(got, want, "chained")
    assert want["n_spanning"].sum() > 0 and want["called"].sum() > 0 and want["spanned"].sum() > 0


# ------------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_the_device_usable(hmm, oracle):
    c = content_case()
    mg = ta.oracle_map(oracle, c.pb)
    want = restate(c, mg)
    ns = int(c.pb.samp_off[-1])
    pd = hmm.hipstr_post_upload(c.pb.ptr, None); assert pd
    def refused(word, pd=pd, **kw):
        a = dict(bptr=c.batch.ptr, seed=c.seed, read_req=c.read_req, req_read=c.req_read, trace=c.trace, hap_to_allele=c.h2a)
        a.update(kw)
        with pytest.raises(RuntimeError, match=word) as e:
            capi.run_census(hmm, pd, a["bptr"], a["seed"], a["read_req"], a["req_read"], a["trace"], hap_to_allele=a["hap_to_allele"], n_samp=ns)
        assert "rc=3" not in str(e.value)
    try:
        refused("hipstr_post_launch")                                    # before the posteriors
        assert hmm.hipstr_post_launch(pd, None) == 0
        fewer = build(c.loci[:2])
        refused("n_loci", bptr=fewer.batch.ptr)
        wider = batch_of([Locus([LFLANK, (100, 120, ["ACAC", "ACACAC", "AC"]), RFLANK], L.samples, L.reqs) for L in c.loci])
        refused("hap_off", bptr=wider.ptr)
        rr = c.read_req.copy(); rr[0] = len(c.req_read); refused("read_req", read_req=rr)
        rr = c.read_req.copy(); rr[0] = -2; refused("read_req", read_req=rr)
        rr = c.read_req.copy(); rr[0] = 2; refused("another locus", read_req=rr)
        refused("grouped by locus", req_read=c.req_read[[2, 3, 0, 1, 4, 5]])
        refused("outside the pooled reads", req_read=np.array([0, 1, 2, 3, 4, 6], np.int32))
        t = dict(c.trace); t["str_seq_off"] = c.trace["str_seq_off"].copy(); t["str_seq_off"][2] = 3; refused("str_seq_off", trace=t)
        h = [x.copy() for x in c.h2a]; h[1][3] = 2; refused("hap_to_allele", hap_to_allele=h)
        h = [x.copy() for x in c.h2a]; h[0][0] = -1; refused("hap_to_allele", hap_to_allele=h)
        t = dict(c.trace); t["stutter_size"] = [-4, NO_STR, -4, 4, -4, 4]; refused("without STR data", trace=t)
        t = dict(c.trace); t["aln_stop"] = None; refused("aln_stop", trace=t)
        refused("null", pd=None)
        # a request without STR data that does not span, or that no read with a seed uses, is not looked at
        t = dict(c.trace); t["stutter_size"] = [-4, NO_STR, -4, 4, -4, 4]; t["aln_start"] = [50, 100, 50, 50, 50, 50]
        ok = capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, t, hap_to_allele=c.h2a, n_samp=ns)
        assert ok["rc"] == 0 and list(ok["n_spanning"]) == [1, 1, 1, 2, 2]
        # the same object, after all that
        good = capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=ns)
        compare(good, want, "after the refused calls")
        # one slot too few: 3 with cand_off usable, and the retry with what it says succeeds
        need = int(want["cand_off"][-1]); chars = sum(len(s) for x in want["cand"] for s in x)
        assert need == 2 and chars == 16
        small = capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=ns, cap_cand=need - 1)
        assert small["rc"] == 3 and np.array_equal(small["cand_off"], want["cand_off"]) and b"too small" in hmm.hipstr_last_error()
        small = capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=ns, cap_cand=need, cap_chars=chars - 1)
        assert small["rc"] == 3 and np.array_equal(small["cand_off"], want["cand_off"]) and b"too small" in hmm.hipstr_last_error()
        again = capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=ns,
                                cap_cand=int(small["cand_off"][-1]), cap_chars=chars)
        compare(again, want, "exact room")
    finally:
        hmm.hipstr_post_free(pd)


# ------------------------------------------------------------------------------------------------------------------ 10. poisoned cache blocks
def test_poisoned_cache_blocks_and_no_driver_allocation(hmm, oracle):
    """Cases 2, 7 (the mixed batch) and 8 after hipstr_debug_cache_poison with 0xFF, 0x7F, 0x80 and 0x00: identical results, equal to the
    restatement, and no block fresh from the driver (tests/test_poison_gpu.py's protocol and counter)."""
    import test_poison_gpu as tp
    c2 = content_case(); c7 = mixed_case(hmm); k = chain_inputs(hmm, oracle)
    w2 = restate(c2, ta.oracle_map(oracle, c2.pb)); w7 = restate(c7, ta.oracle_map(oracle, c7.pb), min_frac=0.02)
    def strip(g):
        return {x: (g[x] if x == "cand" else np.asarray(g[x])) for x in KEYS + ("cand",)}
    for what, fn, want in (("content", lambda: strip(run(hmm, c2)), w2), ("mixed", lambda: strip(run(hmm, c7, min_frac=0.02)), w7)):
        out = tp.poisoned(hmm, fn, "census, " + what)
        compare(dict(out[0], rc=0), want, "poisoned " + what)
    def chain():
        got, asg, tr = run_chain(hmm, k)
        return dict(strip(got), read_req=asg["read_req"], req_read=asg["req_read"], start=tr["aln_start"], stop=tr["aln_stop"], stutter=tr["stutter_size"],
                    soff=tr["str_seq_off"], sseq=tr["str_seq"].raw[:int(tr["str_seq_off"][len(asg["req_read"])])])
    out = tp.poisoned(hmm, chain, "census, chained")
    got, asg, tr = run_chain(hmm, k)
    tp.same_bits(strip(got), {x: out[0][x] for x in KEYS + ("cand",)}, "chained, unpoisoned against poisoned")
    compare(got, chain_want(k, asg, tr), "poisoned chained")
