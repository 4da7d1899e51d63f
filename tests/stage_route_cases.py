"""The launch routes of the traceback, Needleman-Wunsch and posterior stages and the size thresholds between them (DESIGN.md section 3,
"Routes of the other device stages").

Like tests/route_cases.py for the forward pass: every case is deterministic (fixed seeds, no dependence on time or environment), sits on
the two or three sides of one threshold the library reports (hipstr_debug_trace_plan / _nw_plan / _post_plan: limits are read from the
library, never repeated here) and names what the plan must show.  tests/test_stage_routes.py checks the plans on the host,
tests/test_stage_routes_gpu.py runs the same inputs on the device against the oracle.
"""
import collections

import numpy as np

from hipstr_amd import capi
import util


def _rng(tag):
    return np.random.default_rng(sum(map(ord, tag)) * 7919)


def _seq(rng, n):
    return "".join(rng.choice(list("ACGT"), n))


def limits(lib):
    """The three stages' compiled limits, from plans of empty inputs."""
    b = capi.Batch(); util.simple_locus("ACGTACGTAC", ["CAG" * 4], "TGCATGCATG", 3, [], batch=b); b.finalize()
    pb = capi.PostBatch([], [], [0], [], [], [], [], np.zeros(0))
    return dict(trace=capi.trace_plan(lib, b.ptr, [], [])["thresholds"], nw=capi.nw_plan(lib, [])["thresholds"],
                post=capi.post_plan(lib, pb)["thresholds"])


def routes(lib):
    b = capi.Batch(); util.simple_locus("ACGTACGTAC", ["CAG" * 4], "TGCATGCATG", 3, [], batch=b); b.finalize()
    pb = capi.PostBatch([], [], [0], [], [], [], [], np.zeros(0))
    return dict(trace=set(capi.trace_plan(lib, b.ptr, [], [])["routes"]), nw=set(capi.nw_plan(lib, [])["routes"]),
                post=set(capi.post_plan(lib, pb)["routes"]))


# =================================================================================================== traceback
# A call: one-locus batch (the oracle traces one locus), requests with caller seeds (a read of length L with seed s has sides s and
# L - s - 1), the HIPSTR_TRACE_WS_MIB it runs under (None: the call's default) and what its plan must show.
TraceCall = collections.namedtuple("TraceCall", "name batch rr aa seeds ws_mib check")
STRS = ("CAG" * 10, "CAG" * 4 + "CTG" + "CAG" * 5, "CAG" * 12, "CAG" * 3 + "CAA" + "CAG" * 2 + "CTG" + "CAG" * 4, "CAG" * 9)     # pure and interrupted repeats


def _quals(n, i):
    return "".join(chr(ord("5") + (7 * j + 3 * i) % 40) for j in range(n))


def trace_locus(tag, lf, rf, reads, strs=STRS):
    """One locus with random flanks of lf / rf bases; reads: (haplotype offset, length, source STR option) — the haplotype's bases from the
    offset on (beyond its end the read goes on with seeded random bases: an overhang), one substitution in every read of 60 bases and more."""
    rng, b = _rng(tag), capi.Batch()
    L, R = _seq(rng, lf), _seq(rng, rf)
    rds = []
    for i, (off, n, src) in enumerate(reads):
        hap = L + strs[src % len(strs)] + R
        s = hap[off:off + n]
        s += _seq(rng, n - len(s)) if len(s) < n else ""
        if n >= 60:
            at = n // 3
            s = s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]
        rds.append((s, _quals(n, i), off, True))
    util.simple_locus(L, list(strs), R, 3, rds, batch=b)
    return b.finalize()


def side_pairs(T):
    """(left, right) side lengths that put every class edge 64 k | 64 k + 1 of the static classes, the edges between the long kernels, 1
    and the longest side on the left and on the right of some request."""
    C, S, fill = T["HS_MAX_COLS"], T["HS_TRACE_STATIC_CLASSES"], T["fill_cols"]
    edges = [1]
    for cl in range(1, C):
        if cl <= S or fill[cl - 1] != fill[cl]:
            edges += [64 * cl, 64 * cl + 1]
    edges.append(T["max_side"])
    pairs = [(a, b) for a, b in zip(edges, reversed(edges))]
    return edges, pairs


def trace_boundary_sides(T):
    """Sides of 1, 64 | 65, ..., 384 | 385 (static to dynamic LDS), 512 | 513, 768 | 769 and the longest side, each on the left and on the
    right of a request, against a pure and two interrupted alleles; reads that span the STR block, a read inside the left flank and one
    inside the right flank (they never enter the STR row)."""
    edges, pairs = side_pairs(T)
    lf = rf = 700
    reads, seeds = [], []
    for i, (a, b) in enumerate(pairs):
        n = a + b + 1
        off = max(0, lf - 9 - a)                # the seed base 9 bases in front of the STR block where the left side allows it
        reads.append((off, n, (0, 2, 4)[i % 3])); seeds.append(a)
    reads += [(5, 300, 0), (lf + len(STRS[0]) + 20, 200, 0)]; seeds += [129, 64]          # flank-only reads
    batch = trace_locus("trace_boundary_sides", lf, rf, reads)
    rr, aa, ss = [], [], []
    for r in range(len(reads)):
        for k in (0, 1, 3):
            rr.append(r); aa.append(k); ss.append(seeds[r])
    def check(plan, T):
        got_l = {q[0] for c in plan["chunks"] for q in c["requests"]}; got_r = {q[1] for c in plan["chunks"] for q in c["requests"]}
        assert set(edges) <= got_l and set(edges) <= got_r, (sorted(got_l), sorted(got_r))
        names = {k for c in plan["chunks"] for k, _ in c["launch"]}
        assert {"hs_trace_fill_mixed"} | {"hs_trace_fill_long<%d>" % c for c in set(T["fill_cols"][T["HS_TRACE_STATIC_CLASSES"]:])} <= names, names
    return TraceCall("boundary_sides", batch, rr, aa, ss, None, check)


def trace_single_class(T, cl):
    """Every side of the call in class cl, at the class's two ends (64 (cl - 1) + 1 and 64 cl): hs_trace_fill<cl> itself runs."""
    lo, hi = 64 * (cl - 1) + 1, 64 * cl
    lf = rf = 420
    reads = [(max(0, lf - 9 - a), a + b + 1, src) for (a, b), src in (((lo, hi), 0), ((hi, lo), 2), ((hi, hi), 4), ((lo, lo), 0))]
    batch = trace_locus("trace_single_class%d" % cl, lf, rf, reads)
    rr = [0, 0, 1, 1, 2, 3]; aa = [0, 1, 3, 2, 1, 3]; ss = [hi if r in (1, 2) else lo for r in rr]
    def check(plan, T):
        assert len(plan["chunks"]) == 1
        c = plan["chunks"][0]
        assert not c["mixed"] and [k for k, _ in c["launch"]] == ["hs_trace_fill<%d>" % cl, "hs_trace_walk"], c["launch"]
        assert c["launch"][0][1] == 2 * len(rr) == c["classes"][cl - 1]
    return TraceCall("single_class_%d" % cl, batch, rr, aa, ss, None, check)


def trace_many_requests(T, d):
    """HS_TRACE_MIXED_MAX_REQ + d requests of two classes, short reads: one mixed launch up to the limit, the per-class kernels beyond."""
    n = T["HS_TRACE_MIXED_MAX_REQ"] + d
    reads = [(20 + i, 30 + 2 * i, (0, 2, 4)[i % 3]) for i in range(7)] + [(0, 100, 0)]
    batch = trace_locus("trace_many_requests", 40, 40, reads, strs=STRS[:3])
    rr = [q % 8 for q in range(n)]; aa = [(q // 8) % 3 for q in range(n)]
    lens = [r[1] for r in reads]
    ss = [(70 if r == 7 else 1 + (q // 24) % (lens[r] - 2)) for q, r in enumerate(rr)]       # the long read: sides 70 | 29; the others: every seed in turn
    def check(plan, T):
        assert len(plan["chunks"]) == 1
        c = plan["chunks"][0]
        assert c["q1"] - c["q0"] == n and c["classes"][0] > 0 and c["classes"][1] > 0 and sum(c["classes"][2:]) == 0
        assert c["mixed"] == (d <= 0)
        want = ["hs_trace_fill_mixed"] if d <= 0 else ["hs_trace_fill<1>", "hs_trace_fill<2>"]
        assert [k for k, _ in c["launch"]] == want + ["hs_trace_walk"], c["launch"]
    return TraceCall("requests_%+d" % d, batch, rr, aa, ss, None, check)


def walk_rows(T):
    """Flank rows + 1 of the walk cases' alleles: a divisor of HS_WALK_LDS near 384, so a side can hold exactly HS_WALK_LDS bytes."""
    W = T["HS_WALK_LDS"]
    return next(r for k in range(200) for r in (384 - k, 384 + k) if W % r == 0)


def trace_walk_limit(lib, T):
    """Requests whose sides sit at, below and above HS_WALK_LDS bytes of decisions (rows x columns; rows taken from the plan), the two sides
    of a request on opposite sides of it both ways round, and a second left-flank option that moves the limit's column count."""
    rows = walk_rows(T)
    lf = (rows - 1) // 2; rf = rows - 1 - lf
    n0 = T["HS_WALK_LDS"] // rows
    sides = [(n0, n0), (n0, n0 + 1), (n0 + 1, n0), (n0 + 1, n0 + 1), (n0 - 1, n0 + 1), (n0 + 1, n0 - 1), (n0 - 1, n0 - 1)]
    reads = [(max(0, lf - 9 - a), a + b + 1, (0, 2, 4)[i % 3]) for i, (a, b) in enumerate(sides)]
    rng, b = _rng("trace_walk_limit"), capi.Batch()
    L, R = _seq(rng, lf), _seq(rng, rf)
    rds = []
    for i, (off, n, src) in enumerate(reads):
        s = (L + STRS[src] + R)[off:off + n]
        rds.append((s + _seq(rng, n - len(s)), _quals(n, i), off, True))
    short = T["HS_WALK_LDS"] // (n0 + 1)                   # rows under which n0 + 1 columns fit again: a shorter left-flank option
    _, A = util.simple_locus(L, list(STRS), R, 3, rds, batch=b, lf_opts=[L[rows - short:]])
    b.finalize()
    rr = [r for r in range(len(reads)) for _ in range(3)]; aa = [k for _ in reads for k in (0, 1, 3)]; ss = [sides[r][0] for r in rr]
    probe = capi.trace_plan(lib, b.ptr, [0, 0], [0, A - 1], [sides[0][0]] * 2)["chunks"][0]["requests"]
    assert probe[0][2] == rows and probe[1][2] == short, probe             # (which alleles carry the shorter flank: from the plan)
    rr += [1, 2]; aa += [A - 1, A - 1]; ss += [sides[1][0], sides[2][0]]      # n0 + 1 columns of `short` rows: under the limit again
    def check(plan, T):
        W = T["HS_WALK_LDS"]
        seen = set()
        for c in plan["chunks"]:
            for nl, nr, rw, wl, wr in c["requests"]:
                assert wl == (rw * nl <= W) and wr == (rw * nr <= W)
                seen |= {(rw * nl - W, wl), (rw * nr - W, wr)}
                seen.add(("opposite", wl, wr))
        assert (0, 1) in seen and (rows, 0) in seen and (-rows, 1) in seen, sorted(map(str, seen))
        assert ("opposite", 1, 0) in seen and ("opposite", 0, 1) in seen and ("opposite", 0, 0) in seen and ("opposite", 1, 1) in seen
        assert (short * (n0 + 1) - W, 1) in seen                 # the shorter flank: n0 + 1 columns fit again
    return TraceCall("walk_limit", b, rr, aa, ss, None, check)


def trace_repack(d):
    """Ten reads of 40 bases; 4 + d of them requested: twice the requested bases below the batch's (the reads are re-packed for the
    upload) or not."""
    reads = [(10 + i, 40, (0, 2, 4)[i % 3]) for i in range(10)]
    batch = trace_locus("trace_repack", 40, 40, reads, strs=STRS[:3])
    k = 4 + d
    rr = [q // 2 for q in range(2 * k)]; aa = [q % 3 for q in range(2 * k)]; ss = [12 + 2 * r for r in rr]
    def check(plan, T):
        assert plan["wanted_bases"] * 2 - plan["total_bases"] == (-40 * 2 if d <= 0 else 0)
        assert plan["compact_reads"] == (d <= 0)
    return TraceCall("repack_%+d" % d, batch, rr, aa, ss, None, check)


def trace_chunking(ws_mib):
    """A request whose two matrices are exactly 1 MiB (1024 rows x 512 columns twice), two small ones, the large one again: under
    HIPSTR_TRACE_WS_MIB = 1 three chunks — the first full to the byte, class 8 present, absent, present again — and one chunk without."""
    lf, rf = 511, 512
    reads = [(0, 1025, 0), (lf - 30, 80, 2), (lf - 20, 90, 4)]
    batch = trace_locus("trace_chunking", lf, rf, reads, strs=STRS[:3])
    rr = [0, 1, 2, 0]; aa = [0, 1, 2, 1]; ss = [512, 25, 30, 512]
    def check(plan, T):
        if ws_mib is None:
            assert len(plan["chunks"]) == 1
            return
        assert [(c["q0"], c["q1"]) for c in plan["chunks"]] == [(0, 1), (1, 3), (3, 4)]
        assert plan["chunks"][0]["bytes"] == plan["budget"] == ws_mib << 20
        assert [c["classes"][7] for c in plan["chunks"]] == [2, 0, 2] and [c["classes"][0] for c in plan["chunks"]] == [0, 4, 0]
    return TraceCall("chunking_%s" % (ws_mib or "whole"), batch, rr, aa, ss, ws_mib, check)


def trace_over_budget():
    """One column more than fills 1 MiB: refused under HIPSTR_TRACE_WS_MIB = 1."""
    batch = trace_locus("trace_chunking", 511, 512, [(0, 1026, 0)], strs=STRS[:3])
    return TraceCall("over_budget", batch, [0], [0], [512], 1, None)


TraceRefusal = collections.namedtuple("TraceRefusal", "name batch rr aa seeds message")


def trace_refusals(T):
    """Request lists the call refuses from the batch and the list alone, one read and one or two alleles each, with the call's message.
    Every one gets past validate_tables ("haplotype block without options" does not: that one is validate_tables' own)."""
    m = T["max_side"]
    def locus(lf, strs, rf, n=40, period=3, lf_opts=None):
        b = capi.Batch()
        util.simple_locus(lf, strs, rf, period, [(("ACGT" * (n // 4 + 1))[:n], None, 0, True, [("M", n)])], batch=b, lf_opts=lf_opts)
        return b.finalize()
    L, S, R = "ACGTTGCAAC" * 3, "CAG" * 8, "TGCATTGACA" * 3
    plain = locus(L, [S, S + "CAG"], R)
    return [TraceRefusal("period_10", locus(L, [S], R, period=10), [0], [0], [20], "STR period must be in [1,9] (stutter_model.h:38)"),
            TraceRefusal("str_2048", locus(L, [S, "CA" * 1024], R), [0], [1], [20], "STR allele longer than 2047 bp is not supported"),
            TraceRefusal("flanks_4095", locus("A" * 2047, [S], "C" * 2048), [0], [0], [20], "flanks longer than 4094 bases in total are not supported"),
            TraceRefusal("empty_str", locus(L, [S, ""], R), [0], [1], [20], "empty STR allele is not supported"),
            TraceRefusal("empty_flank", locus(L, [S], R, lf_opts=[""]), [0], [1], [20], "empty flank sequence"),
            TraceRefusal("read_outside", plain, [1], [0], [20], "request names a read outside the batch"),
            TraceRefusal("allele_outside", plain, [0], [2], [20], "request names an allele outside its locus"),
            TraceRefusal("seed_0", plain, [0], [0], [0], "seed base must leave at least one base on either side (HapAligner.cpp:316)"),
            TraceRefusal("seed_last", plain, [0], [1], [39], "seed base must leave at least one base on either side (HapAligner.cpp:316)"),
            TraceRefusal("side_over", locus(L, [S], R, n=m + 3), [0], [0], [m + 1], "traceback of a read side longer than %d bases is not supported" % m)]


def trace_calls(lib, T):
    calls = [trace_boundary_sides(T)] + [trace_single_class(T, cl) for cl in range(1, T["HS_TRACE_STATIC_CLASSES"] + 1)]
    calls += [trace_many_requests(T, 0), trace_many_requests(T, 1), trace_walk_limit(lib, T), trace_repack(0), trace_repack(1),
              trace_chunking(None), trace_chunking(1)]
    return calls


# (calls that share requests and differ only in the route the batch composition gives them: the shared requests' results must be identical)
TRACE_TWINS = [("requests_+0", "requests_+1"), ("repack_+0", "repack_+1"), ("chunking_whole", "chunking_1")]


def plan_of_trace(lib, call):
    return capi.trace_plan(lib, call.batch.ptr, call.rr, call.aa, call.seeds, float(call.ws_mib or 0))


def h2r_of(oracle, call):
    return util.synthetic_hap_to_ref(oracle, call.batch.ptr)


# =================================================================================================== Needleman-Wunsch
NwCall = collections.namedtuple("NwCall", "name pairs ws_mib check")


def _mutated(rng, s, n):
    """n bases that follow s with a substitution, an insertion or a deletion every 40 bases or so (cyclically extended)."""
    out, i = [], 0
    while len(out) < n:
        c = s[i % len(s)]; i += 1
        u = rng.random()
        if u < 0.012:
            continue
        if u < 0.024:
            out.append("ACGT"[int(rng.integers(4))])
        out.append(c if u > 0.05 else "ACGT"[int(rng.integers(4))])
    return "".join(out[:n])


def nw_rung_lengths(N):
    """Read lengths on both sides of every rung of the rows-per-lane ladder, 1 and the limit."""
    ls = [1]
    for r in N["rows"][:-1]:
        ls += [64 * r, 64 * r + 1]
    return ls + [N["HS_NW_MAX_READ"]]


def nw_rungs(N):
    """A read of every rung-edge length against a reference window of similar size (random sequence with substitutions and indels), then
    homopolymers and all-N sequences at the same lengths (every cell ties: bestIndex decides the walk)."""
    rng = _rng("nw_rungs")
    pairs = []
    for L2 in nw_rung_lengths(N):
        L1 = min(N["HS_NW_MAX_REF"], L2 + 40 + L2 // 8)
        ref = _seq(rng, L1)
        pairs.append((ref, _mutated(rng, ref[20:], L2)))
    for L2 in nw_rung_lengths(N):
        pairs.append(("A" * min(N["HS_NW_MAX_REF"], L2 + 7), "A" * L2))
        pairs.append(("N" * max(1, L2 - 3), "N" * L2))
    pairs.append(("ACGT" * 50, "a" * 65)); pairs.append(("acgtn" * 30, "ACGTN" * 26))           # lower case, N against bases
    def check(plan, N):
        assert plan["n_chunks"] == 1
        got = plan["chunks"][0]["rungs"]
        want = [0] * len(N["rows"])
        for _, q in pairs:
            want[next(i for i, r in enumerate(N["rows"]) if (len(q) + 63) // 64 <= r)] += 1
        assert got == want and min(got) >= 6, (got, want)
        assert [k for k, _ in plan["chunks"][0]["launch"]] == ["hs_nw_fill<%d>" % r for r in N["rows"]]
    return NwCall("rungs", pairs, None, check)


def nw_ref_lengths(N):
    """References of 1 base, of the limit, and the limit against the longest read."""
    rng = _rng("nw_ref_lengths")
    big = _seq(rng, N["HS_NW_MAX_REF"])
    pairs = [("A", "A"), ("C", "ACGT"), ("G", _seq(rng, 130)), (big, _mutated(rng, big[1000:], 150)), (big, "T"),
             (big, _mutated(rng, big[300:], N["HS_NW_MAX_READ"])), (_seq(rng, 300), _seq(rng, 1))]
    def check(plan, N):
        l1 = [len(r) for r, _ in pairs]
        assert 1 in l1 and N["HS_NW_MAX_REF"] in l1 and sum(plan["chunks"][0]["rungs"]) == len(pairs)
    return NwCall("ref_lengths", pairs, None, check)


def nw_over_budget(ws_mib):
    """A pair of more traceback bytes than HIPSTR_NW_WS_MIB = 1 between two small ones: it runs alone, over the budget."""
    rng = _rng("nw_over_budget")
    big = _seq(rng, 1300)
    pairs = [(_seq(rng, 90), _seq(rng, 70)), (big, _mutated(rng, big[50:], 1000)), (big[:200], _mutated(rng, big[10:], 150))]
    def check(plan, N):
        if ws_mib is None:
            assert plan["n_chunks"] == 1
            return
        assert [(c["p0"], c["p1"], c["over_budget"]) for c in plan["chunks"]] == [(0, 1, False), (1, 2, True), (2, 3, False)]
        assert plan["chunks"][1]["bytes"] > plan["budget"] == ws_mib << 20
    return NwCall("over_budget_%s" % (ws_mib or "whole"), pairs, ws_mib, check)


def nw_calls(N):
    return [nw_rungs(N), nw_ref_lengths(N), nw_over_budget(None), nw_over_budget(1)]


def nw_refused(N):
    """(pairs, message) just beyond the two limits; the accepted neighbours are in nw_rungs / nw_ref_lengths."""
    return [([("ACGT" * 30, "A" * (N["HS_NW_MAX_READ"] + 1))], "second sequence longer than %d" % N["HS_NW_MAX_READ"]),
            ([("C" * (N["HS_NW_MAX_REF"] + 1), "ACGT")], "reference longer than %d" % N["HS_NW_MAX_REF"])]


# =================================================================================================== posteriors
PostCall = collections.namedtuple("PostCall", "name pb n_shared check")


def post_batch(tag, units, haploid=None, prior=False, phased=True):
    """units: (alleles, reads) per single-sample locus.  Likelihood rows shaped like alignments (a best allele, the rest falling off),
    weights 0..2, phasing terms unless phased is False (then log_p1 == log_p2: the symmetric accumulation).  Every unit's numbers are
    drawn in turn, so two batches that start with the same units give those units the same inputs."""
    rng = _rng(tag)
    A = [a for a, _ in units]; R = [r for _, r in units]
    off = np.concatenate([[0], np.cumsum(R)]).astype(np.int32); n = int(off[-1])
    ll, p1, p2, w, pr = [], [], [], [], []
    for a, r in units:
        best = rng.integers(0, a, size=r)
        ll.append((-np.abs(np.arange(a)[None, :] - best[:, None]) * rng.uniform(0.3, 3.0, size=(r, 1)) - rng.random((r, a)) * 4).ravel())
        p1.append(-rng.random(r) * 3)
        p2.append(-rng.random(r) * 3 if phased else p1[-1])
        w.append(rng.integers(0, 3, size=r).astype(np.int32))
        pr.append(-rng.random(a * a) * 6)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return capi.PostBatch(A, [1] * len(A), off, np.zeros(n, np.int32), cat(p1, np.float64), cat(p2, np.float64), cat(w, np.int32),
                          cat(ll, np.float64), haploid=haploid, log_prior=cat(pr, np.float64) if prior else None)


def _unit(plan, i):
    return dict(zip(("A", "reads", "chunked", "rt", "tiles", "echunks", "empty"), plan["units"][i]))


def post_calls(Pl):
    T, E, Rg, W, U = Pl["HS_POST_THREADS"], Pl["HS_POST_ECHUNK"], Pl["HS_POST_REGS"], Pl["HS_POST_SPLIT_WGS"], Pl["HS_POST_SPLIT_MAX_UNITS"]
    a_split = int(np.floor(np.sqrt(T)))                    # A^2 <= threads: one workgroup's worth, never split (16 | 17)
    a_regs = int(np.floor(np.sqrt(T * Rg)))                # A^2 <= threads x registers: the register path (45 | 46)
    a_2e = int(np.floor(np.sqrt(2 * E)))                   # A^2 <= two chunks of exponentials (64 | 65)
    cap = lambda a: E // (2 * a + 1)                       # reads of a tile
    calls = []
    def add(name, pb, check, n_shared=0):
        calls.append(PostCall(name, pb, n_shared, check))
    # --- max_nd at the size limit of the split, few units
    for d in (0, 1):
        a = a_split + d
        def check(p, d=d, a=a):
            assert p["max_nd"] == a * a and (p["split"] > 1) == (d > 0)
            assert _unit(p, 0)["chunked"] == d and [k for k, _ in p["launch"]] == (["hs_posterior_kernel"] if d == 0 else ["hs_posterior_accumulate_kernel", "hs_posterior_finish_kernel"])
        add("split_size_%+d" % d, post_batch("pss%d" % d, [(a, 30), (3, 5), (a, 9)]), check)
        add("split_size_unphased_%+d" % d, post_batch("pssu%d" % d, [(a, 30), (5, 5)], phased=False), check)
    # --- the register path's limit and the chunks of exponentials, in a launch too large to split and in a split one
    filler = [(2, 3)] * (U - 1)
    for a, what in ((a_regs, "regs_+0"), (a_regs + 1, "regs_+1"), (a_2e, "echunk2_+0"), (a_2e + 1, "echunk2_+1")):
        def check(p, a=a):
            u = _unit(p, 0)
            assert p["split"] == 1 and p["n_units"] == U and u["chunked"] == (a * a > T * Rg) and u["echunks"] == (0 if a * a <= T * Rg else -(-a * a // E))
        add("unsplit_" + what, post_batch("pu" + what, [(a, 12)] + filler), check)
        def check_s(p, a=a):
            u = _unit(p, 0)
            assert p["split"] > 1 and u["chunked"] == 1 and u["echunks"] == -(-a * a // E)
        add("split_" + what, post_batch("ps" + what, [(a, 12), (a, 7)]), check_s)
    # --- reads per tile: below, at and above, for an A that is never split and for the largest A of the register path; the same reads
    # on the chunked path
    for a, pad in ((a_split, []), (a_regs, filler), (a_regs + 1, filler)):
        for d in (-1, 0, 1):
            r = cap(a) + d
            def check(p, a=a, d=d, r=r):
                u = _unit(p, 0)
                assert p["split"] == 1 and u["reads"] == r
                if a <= a_regs:
                    assert u["chunked"] == 0 and u["rt"] == min(r, cap(a)) and u["tiles"] == (1 if d <= 0 else 2)
                else:
                    assert u["chunked"] == 1
            add("tile_A%d_%+d" % (a, d), post_batch("pt%d%d" % (a, d), [(a, r)] + pad), check)
    def check_sym(p):
        assert _unit(p, 0)["tiles"] == 2 and _unit(p, 0)["chunked"] == 0, p["units"][0]
    add("tile_unphased_A%d" % a_regs, post_batch("ptu", [(a_regs, cap(a_regs) + 1)] + filler, phased=False), check_sym)
    # --- the unit count's limit: U - 1 units split by the large unit, U units do not; the first U - 1 units are shared
    head = [(a_split + 1, 20)] + [(2 + i % 3, i % 4) for i in range(U - 2)]
    for d in (-1, 0):
        def check(p, d=d):
            assert p["n_units"] == U + d and (p["split"] > 1) == (d < 0) and p["max_nd"] == (a_split + 1) ** 2
            if d < 0:
                assert p["split"] == min(-(-p["max_nd"] // T), -(-W // (U - 1)))
        add("units_%+d" % d, post_batch("punits", head + [(4, 6)] * (d + 1)), check, n_shared=U - 1)
    # --- one large unit among units of 1, 2 and 3 alleles, with and without reads, under a split launch: the small units' workgroups
    # beyond the first have an empty share.  Alone (split) and in front of U filler units (not split): the same bits.
    mixed = [(96, 40), (1, 4), (2, 5), (3, 6), (2, 0), (1, 0), (3, 0), (96, 0)]
    for name, kw in (("mixed", {}), ("mixed_haploid", dict(haploid=[0, 0, 1, 1, 0, 1, 0, 1])), ("mixed_prior", dict(prior=True))):
        for tail, sfx in ((0, "split"), (U, "unsplit")):
            units = mixed + [(2, 2)] * tail
            k2 = dict(kw)
            if "haploid" in k2:
                k2["haploid"] = k2["haploid"] + [0] * tail
            def check(p, tail=tail):
                assert (p["split"] > 1) == (tail == 0)
                if tail == 0:
                    assert p["split"] == min(-(-96 * 96 // T), -(-W // len(mixed))) and all(_unit(p, i)["empty"] == p["split"] - 1 for i in (1, 2, 3, 4, 5, 6))
                    assert _unit(p, 0)["empty"] == 0
            add("%s_%s" % (name, sfx), post_batch("p" + name, units, **k2), check, n_shared=len(mixed))
    return calls


POST_TWINS = [("units_-1", "units_+0"), ("mixed_split", "mixed_unsplit"), ("mixed_haploid_split", "mixed_haploid_unsplit"),
              ("mixed_prior_split", "mixed_prior_unsplit")]
