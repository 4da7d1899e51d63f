"""GPU: hipstr_post_assign — reads assigned to their sample's MAP haplotypes, the per-sample read counts of a VCF record and the
traceback request list, on the resident posteriors (include/hipstr_hmm.h).

The yardstick is `restate` (tests/flow_chain.py, shared with the end-to-end chain): a line-by-line Python restatement of the loop over the reads in SeqStutterGenotyper::write_vcf_record
(reference src/seq_stutter_genotyper.cpp:1079-1157), of the phase totals (:1355-1356) and of retrace_alignments' pick (:823-825), with
mathops.cpp:52-57 and :64-70 for the two log-sum-exps.  LIMITATION: the compiled reference cannot provide goldens for this stage
(write_vcf_record needs htslib, which the oracle build does not have), so the expected values come from this restatement and not from
the reference's own binary.  It evaluates exp / log with math.exp / math.log in Python loops — the host libm, one argument at a time;
numpy's vectorised exp is a different implementation and is not used.

Contract (tests/util.py: assert_arrays_exact, tolerance 1e-9): the integer outputs — best_hap, read_strand, the eight counters, n_req,
req_read, req_allele, read_req — equal the restatement always: no exp / log enters them.  The float outputs — log_phase_one, phase1_reads,
phase2_reads — equal it bit for bit (level 1), or else (level 2) equal bit for bit the same restatement evaluated with a host build of
hipstr_amd/csrc/cr_math.h (tests/cpp/libcr_math_test.so, built and loaded the way tests/test_cr_math.py does), which must be within 1e-9
of the libm one."""
import ctypes as C
import math

import numpy as np
import pytest

import util
from hipstr_amd import capi

pytestmark = pytest.mark.gpu

LOG_ONE_HALF = math.log(0.5)          # mathops.cpp: LOG_ONE_HALF = log(0.5)
TOLERANCE = 1e-10                     # mathops.cpp:10
INT_KEYS = ("best_hap", "read_strand") + capi.ASSIGN_COUNTERS
REQ_KEYS = ("req_read", "req_allele", "read_req")


# the restatement itself (and the two log-sum-exps it uses): tests/flow_chain.py, shared with the end-to-end chain
from flow_chain import _lse2, _lse_vec, assign_restate as restate  # noqa: E402,F401


_CR = []


def _cr_fns():
    """exp / log of hipstr_amd/csrc/cr_math.h compiled for the host (tests/test_cr_math.py's library), one argument at a time."""
    if not _CR:
        import test_cr_math
        lib = test_cr_math.build_lib()
        x = np.zeros(1); y = np.zeros(1)
        px, py = x.ctypes.data_as(capi._f64p), y.ctypes.data_as(capi._f64p)
        def mk(fn):
            def f(v):
                x[0] = v; fn(px, py, 1); return float(y[0])
            return f
        _CR.extend([mk(lib.cr_exp_batch), mk(lib.cr_log_batch)])
    return _CR


def check(got, pb, LL, map_gt, seed, what, requests=False, **kw):
    """The two-level contract of the module docstring; returns the libm restatement."""
    want = restate(pb, LL, map_gt, seed, **kw)
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s\n got %r\nwant %r" % (what, k, got[k], want[k])
    if requests:
        assert got["n_req"] == want["n_req"], "%s: n_req %d != %d" % (what, got["n_req"], want["n_req"])
        for k in REQ_KEYS:
            assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)
    live = want["best_hap"] >= 0
    assert np.all(np.isnan(got["log_phase_one"][~live])), "%s: log_phase_one of a skipped read was written" % what
    floats = lambda o: (o["log_phase_one"][live], o["phase1_reads"], o["phase2_reads"])
    def cr():
        e, l = _cr_fns()
        return floats(restate(pb, LL, map_gt, seed, exp=e, log=l, **kw))
    util.assert_arrays_exact(floats(got), floats(want), cr, what)
    return want


def oracle_map(oracle, pb):
    return capi.run_posteriors(oracle, "oracle_", pb)[2]


def make_pb(loci, haploid=None):
    """loci: list of (A, [reads per sample: list of (log_p1, log_p2, LL row)]) -> (PostBatch, flat LL)."""
    nA, nS, off, lab, p1, p2, LL = [], [], [0], [], [], [], []
    for A, samples in loci:
        nA.append(A); nS.append(len(samples))
        for s, reads in enumerate(samples):
            for (a, b, row) in reads:
                assert len(row) == A
                lab.append(s); p1.append(a); p2.append(b); LL.extend(row)
        off.append(len(lab))
    LL = np.array(LL, np.float64)
    return capi.PostBatch(nA, nS, off, lab, p1, p2, np.ones(len(lab), np.int32), LL if LL.size else np.zeros(1), haploid=haploid), LL


# ------------------------------------------------------------------------------------------------------------------ 1. chained from the device
def test_chained_from_device_alignments(hmm, oracle):
    """align -> posteriors -> assignment -> tracebacks with the likelihood matrix never leaving the device (no hipstr_hmm_fetch): checked
    against the restatement fed the oracle's likelihoods and the oracle's MAP pairs; the request list drives hipstr_hmm_trace."""
    nl, R = 6, 40
    sb = capi.SynthBatch(n_loci=nl, reads_per_locus=R, n_str_alleles=12, seed=77)
    dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev
    assert hmm.hipstr_hmm_align(dev, None) == 0
    A = np.diff(np.ctypeslib.as_array(sb.ptr.contents.hap_off, shape=(nl + 1,)))
    lab = np.tile(np.repeat(np.arange(4), R // 4), nl)
    rng = np.random.default_rng(3); n = nl * R
    kw = dict(n_alleles=A, n_samples=np.full(nl, 4), read_off=np.arange(nl + 1) * R, sample_label=lab, log_p1=-rng.random(n), log_p2=-rng.random(n),
              read_weight=np.ones(n, np.int32))
    seeds = np.zeros(n, np.int32)
    assert hmm.hipstr_calc_seed_bases(sb.ptr, seeds.ctypes.data_as(capi._i32p)) == 0           # host only: what seed_positions_ holds
    reverse = rng.integers(0, 2, n).astype(np.uint8)
    pool = np.tile(np.arange(R), nl); pool_off = np.arange(nl + 1) * R                        # every read its own pool: the batch IS the pooled batch
    try:
        got = capi.run_assign(hmm, capi.PostBatch(log_aln_probs=None, **kw), seeds, reverse=reverse, pool_index=pool, pool_off=pool_off,
                              dev_ll=hmm.hipstr_hmm_dev_aln_probs(dev))
    finally:
        hmm.hipstr_hmm_free(dev)
    assert got["rc"] == 0
    want_ll, want_seeds = capi.run_align(oracle, "oracle_", sb.ptr)
    assert np.array_equal(seeds, want_seeds)
    pb = capi.PostBatch(log_aln_probs=want_ll, **kw)
    want = check(got, pb, want_ll, oracle_map(oracle, pb), seeds, "chained", requests=True, reverse=reverse, pool_index=pool, pool_off=pool_off)
    assert want["n_req"] > 0
    tr = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, got["req_read"], got["req_allele"], unpack=False, cap=1 << 18)      # raises unless it returns 0
    fwd = [want_ll[sb.out_off[rr // R] + (rr % R) * A[rr // R] + al] for rr, al in zip(got["req_read"], got["req_allele"])]
    assert list(tr["ll"][:got["n_req"]]) == fwd


# ------------------------------------------------------------------------------------------------------------------ 2. wavefront / workgroup edges
EDGE_SIZES = {"workgroup_per_unit": (0, 1, 63, 64, 65, 257), "wavefront_per_unit": (0, 1, 63, 64, 65, 256)}


def edges_inputs(sizes):
    """One locus, A = 3, samples on either side of the 64-lane and 256-thread chunks (257 reads: a unit has the workgroup; 256: the
    launch gives every unit one wavefront); seeds < 0 scattered through, a sample whose reads are all skipped, skipped first and last reads.
    -> (PostBatch, flat LL, seed, reverse)."""
    rng = np.random.default_rng(5)
    samples = []
    for sz in sizes:
        reads = []
        for i in range(sz):
            row = list(-25 - 5 * rng.random(3))
            row[0 if i % 2 == 0 else 2] = -1 - rng.random()                         # reads alternate between haplotypes 0 and 2: the MAP pair is {0, 2}
            if i % 7 == 3:
                row[0] = row[2] = -1.5 - 0.05 * rng.random()                        # some inside the strand tolerance
            p = -rng.random(2) if i % 3 else (-0.3, -0.3)
            reads.append((float(p[0]), float(p[1]), row))
        samples.append(reads)
    pb, LL = make_pb([(3, samples)])
    off = np.concatenate([[0], np.cumsum(sizes)])
    seed = np.where(rng.random(off[-1]) < 0.2, -1, 10).astype(np.int32)
    seed[off[2]:off[3]] = -1                                                         # the 63-read sample: all skipped
    seed[off[3]] = -1; seed[off[4] - 1] = -1                                         # first and last read of the 64-read sample
    seed[off[4]] = -1; seed[off[6] - 1] = -1                                         # first of the 65-read sample, last of the largest
    reverse = rng.integers(0, 2, off[-1]).astype(np.uint8)
    return pb, LL, seed, reverse


@pytest.mark.parametrize("sizes", list(EDGE_SIZES.values()), ids=list(EDGE_SIZES))
def test_wavefront_and_workgroup_edges(hmm, oracle, sizes):
    pb, LL, seed, reverse = edges_inputs(sizes)
    mg = oracle_map(oracle, pb)
    for s in (3, 4, 5):
        assert sorted(mg[s]) == [0, 2]
    got = capi.run_assign(hmm, pb, seed, reverse=reverse)
    want = check(got, pb, LL, mg, seed, "edges %r" % (sizes,), reverse=reverse)
    assert want["n_aligned"][0] == 0 and want["n_aligned"][2] == 0 and got["phase1_reads"][2] == 0 and got["phase2_reads"][2] == 0
    assert want["uniq_one"].sum() > 0 and want["uniq_two"].sum() > 0 and want["rv_uniq_one"].sum() > 0


@pytest.mark.parametrize("n_big", [40, 257], ids=["wavefront_per_unit", "workgroup_per_unit"])
def test_a_sample_without_a_map_pair_is_skipped(hmm, oracle, n_big):
    """Three samples of one locus, A = 3; every likelihood of the middle one is -inf, so no diplotype of it is finite and its MAP pair is
    (-1, -1) (hs_assign_kernel's no_map branch).  Its reads come out as skipped reads do and its counts are zero; its neighbours (one padded to 257
    reads for the workgroup-per-unit launch) and the request list come out as from the batch without it."""
    rng = np.random.default_rng(17)
    def sample(n, h1, h2):
        out = []
        for i in range(n):
            row = list(-25 - 5 * rng.random(3)); row[h1 if i % 2 == 0 else h2] = -1 - rng.random()
            p = -rng.random(2) if i % 3 else (-0.3, -0.3)
            out.append((float(p[0]), float(p[1]), [float(x) for x in row]))
        return out
    first, last = sample(9, 0, 2), sample(n_big, 1, 1)
    middle = [(-0.2, -0.6, [-np.inf] * 3) for _ in range(5)]
    pb, LL = make_pb([(3, [first, middle, last])])
    n = 9 + 5 + n_big
    seed = np.full(n, 4, np.int32); seed[[2, 20]] = -1
    reverse = (np.arange(n) % 3 == 0).astype(np.uint8)
    pool = (np.arange(n) % 6).astype(np.int32); pool[9:14] = [5, 0, 3, 3, 1]         # the middle sample shares its neighbours' pools
    pool_off = np.array([0, 6], np.int32)
    mg = oracle_map(oracle, pb)
    assert tuple(mg[1]) == (-1, -1) and sorted(mg[0]) == [0, 2] and tuple(mg[2]) == (1, 1)
    assert capi.post_plan(hmm, pb)["units"][2][1] == n_big
    got = capi.run_assign(hmm, pb, seed, reverse=reverse, pool_index=pool, pool_off=pool_off)
    want = check(got, pb, LL, mg, seed, "no MAP pair, %d reads beside it" % n_big, requests=True, reverse=reverse, pool_index=pool, pool_off=pool_off)
    mid = slice(9, 14)
    for k in ("best_hap", "read_strand", "read_req"):
        assert np.all(got[k][mid] == -1) and np.all(want[k][mid] == -1), k
    assert np.all(np.isnan(got["log_phase_one"][mid]))                               # untouched: what run_assign put there
    for k in capi.ASSIGN_COUNTERS:
        assert got[k][1] == 0, k
    assert got["phase1_reads"][1] == 0 and got["phase2_reads"][1] == 0
    keep = np.r_[0:9, 14:n]
    pb2, _ = make_pb([(3, [first, last])])
    alone = capi.run_assign(hmm, pb2, seed[keep], reverse=reverse[keep], pool_index=pool[keep], pool_off=pool_off)
    assert alone["rc"] == 0 and got["n_req"] == alone["n_req"] > 0
    for k in ("best_hap", "read_strand", "read_req"):
        assert np.array_equal(got[k][keep], alone[k]), k
    assert np.array_equal(got["log_phase_one"][keep].view(np.uint64), alone["log_phase_one"].view(np.uint64))
    for k in capi.ASSIGN_COUNTERS:
        assert np.array_equal(got[k][[0, 2]], alone[k]), k
    for k in ("phase1_reads", "phase2_reads"):
        assert np.array_equal(got[k][[0, 2]].view(np.uint64), alone[k].view(np.uint64)), k
    assert np.array_equal(got["req_allele"], alone["req_allele"]) and np.array_equal(got["req_read"], alone["req_read"])


# ------------------------------------------------------------------------------------------------------------------ 3. every branch of :1096-1109
T01 = 0.1
ANCHORS = [(-0.4, -0.4, [-1.0, -40.0])] * 3 + [(-0.4, -0.4, [-40.0, -1.0])] * 3          # make (0, 1) the MAP pair; themselves far outside the tolerance


def _branch_batch():
    het = [  # (log_p1, log_p2, LL): v1 - v2 = LL[0] - LL[1] with log_p1 == log_p2 == 0
        (0.0, 0.0, [-T01, -2 * T01]),                          # v1 - v2 == +0.1 exactly (Sterbenz): not > tolerance
        (0.0, 0.0, [-2 * T01, -T01]),                          # == -0.1 exactly
        (0.0, 0.0, [np.nextafter(-T01, 0.0), -2 * T01]),       # +0.1 + 1 ulp
        (0.0, 0.0, [np.nextafter(-T01, -1.0), -2 * T01]),      # +0.1 - 1 ulp
        (0.0, 0.0, [-2 * T01, np.nextafter(-T01, 0.0)]),       # -(0.1 + 1 ulp)
        (0.0, 0.0, [-2 * T01, np.nextafter(-T01, -1.0)]),      # -(0.1 - 1 ulp)
        (0.0, 0.0, [-0.15, -0.2]), (0.0, 0.0, [-0.2, -0.15]), (0.0, 0.0, [-0.2, -0.2]),      # well inside
        (-0.5, -0.2, [-0.3, -0.3]), (-0.2, -0.5, [-0.3, -0.3]),                              # outside through the phasing terms, both ways
        (-0.3, -0.1, [-0.3, -0.3]),                                                          # |v1 - v2| = 0.2: inside a tolerance of 0.5 only
    ]
    v = [a + r[0] - (b + r[1]) for a, b, r in het]
    assert v[0] == T01 and v[1] == -T01 and v[2] == np.nextafter(T01, 1.0) and v[3] == np.nextafter(T01, 0.0) and v[4] == -v[2] and v[5] == -v[3]
    hom = [(-1.0, -1.0, [-1.0, -50.0])] * 4
    loci = [
        (2, [[(-0.2, -0.9, [-1.0, -50.0])] * 3 + [(-0.9, -0.2, [-1.0, -50.0])]]),                 # 0: haploid locus, phased reads
        (2, [hom + [(-0.5, -0.5, [-1.0, -50.0])]]),                                               # 1: homozygous MAP, log_p1 == log_p2
        (2, [hom + [(-0.5, -0.5 - 1.5e-10, [-1.0, -50.0]), (-0.5, -0.5 - 0.5e-10, [-1.0, -50.0]),  # 2: ... just above / just below 1e-10
                    (-3.0, -0.01, [-1.0, -50.0]), (-0.01, -3.0, [-1.0, -50.0])]]),                #    ... and far above, both ways
        (2, [ANCHORS + het]),                                                                     # 3: heterozygous MAP
    ]
    pb, LL = make_pb(loci, haploid=[1, 0, 0, 0])
    return pb, LL, len(ANCHORS), len(het)


@pytest.fixture(scope="module")
def branch_batch(oracle):
    pb, LL, na, nh = _branch_batch()
    mg = oracle_map(oracle, pb)
    assert [tuple(x) for x in mg] == [(0, 0), (0, 0), (0, 0), (0, 1)]
    n = int(pb.a["read_off"][-1])
    reverse = (np.arange(n) % 2).astype(np.uint8)
    return pb, LL, mg, np.full(n, 5, np.int32), reverse, na, nh


@pytest.mark.parametrize("rule", [capi.ASSIGN_VCF, capi.ASSIGN_RETRACE])
@pytest.mark.parametrize("tol", [0.0, 0.5, 0.05])
@pytest.mark.parametrize("with_reverse", [True, False])
def test_every_branch(hmm, branch_batch, rule, tol, with_reverse):
    pb, LL, mg, seed, reverse, na, nh = branch_batch
    rev = reverse if with_reverse else None
    got = capi.run_assign(hmm, pb, seed, reverse=rev, rule=rule, strand_tolerance=tol)
    want = check(got, pb, LL, mg, seed, "branches rule %d tol %g reverse %s" % (rule, tol, with_reverse), reverse=rev, rule=rule, tol=tol)
    r3 = int(pb.a["read_off"][3]) + na                                   # the hand-made heterozygous reads
    if tol == 0.0:
        # haploid / homozygous with equal phasing: never in the branch; homozygous with distinct phasing: in it only far above 1e-10 ...
        assert list(want["uniq_one"][:3] + want["uniq_two"][:3]) == [0, 0, 2] and list(want["n_snp"][:3]) == [4, 0, 3]
        # ... heterozygous: exactly 0.1 and one ulp below are inside, one ulp above is outside
        assert list(want["read_strand"][r3:r3 + 6]) == [0, 0, 0, 0, 1, 0]
        assert want["uniq_one"][3] == 3 + 1 + 1 and want["uniq_two"][3] == 3 + 1 + 2
    if tol == 0.5:
        assert want["uniq_one"][3] == 3 and want["uniq_two"][3] == 3     # only the anchors are outside
    if not with_reverse:
        assert want["rv_uniq_one"].sum() == 0 and want["rv_uniq_two"].sum() == 0
    else:
        assert want["rv_uniq_one"].sum() > 0 and want["rv_uniq_two"].sum() > 0


def test_rules_disagree_on_in_tolerance_heterozygous_reads(hmm, branch_batch):
    """The rule changes best_hap and nothing else, and only where write_vcf_record's tolerance keeps a heterozygous read on haplotype one
    although its second term is not smaller (:1098 not taken, :825 picks hap_b)."""
    pb, LL, mg, seed, reverse, na, nh = branch_batch
    g0 = capi.run_assign(hmm, pb, seed, reverse=reverse, rule=capi.ASSIGN_VCF)
    g1 = capi.run_assign(hmm, pb, seed, reverse=reverse, rule=capi.ASSIGN_RETRACE)
    for k in ("read_strand",) + capi.ASSIGN_COUNTERS:
        assert np.array_equal(g0[k], g1[k]), k
    for k in ("log_phase_one", "phase1_reads", "phase2_reads"):
        assert np.array_equal(g0[k].view(np.uint64), g1[k].view(np.uint64)), k
    a = pb.a; expect = []
    for l in range(4):
        for r in range(int(a["read_off"][l]), int(a["read_off"][l + 1])):
            row = LL[2 * r:2 * r + 2]; ha, hb = mg[l]
            v1 = a["log_p1"][r] + row[ha]; v2 = a["log_p2"][r] + row[hb]
            x1 = LOG_ONE_HALF + a["log_p1"][r] + row[ha]; x2 = LOG_ONE_HALF + a["log_p2"][r] + row[hb]
            expect.append(ha != hb and abs(v1 - v2) <= 0.1 and not (x1 > x2))
    differ = g0["best_hap"] != g1["best_hap"]
    assert list(differ) == expect and 3 <= differ.sum() < nh
    assert np.all(differ[:int(a["read_off"][3]) + na] == False)


# ------------------------------------------------------------------------------------------------------------------ 4. request list
def request_inputs(oracle):
    """Two loci whose request tables are a direct one (locus 0) and a hashed one (locus 1).
    -> (PostBatch, flat LL, the oracle's MAP pairs, seed, pool_index, pool_off)."""
    rng = np.random.default_rng(9)
    fav = lambda A, h: [(-1.0 if k == h else -30.0) - float(rng.random()) for k in range(A)]
    # locus 0, A = 3: three samples that settle on haplotypes 0, 1 and {0, 2}; the pools are shared across the samples
    l0 = [[(-0.5, -0.5, fav(3, 0)) for _ in range(6)],
          [(-0.5, -0.5, fav(3, 1)) for _ in range(6)],
          [(-0.2, -0.9, fav(3, 0 if i % 2 else 2)) for i in range(8)] + [(-0.5, -0.5, [-1.25, -33.0, -32.0])] * 70]     # + a pool of 70 identical reads
    pool0 = [0, 1, 2, 0, 1, 2] + [2, 1, 0, 0, 1, 2] + [0, 1, 2, 3, 3, 2, 1, 0] + [4] * 70
    # locus 1, A = 5, 1000 pools (5000 keys: a hashed table), two samples
    l1 = [[(-0.5, -0.5, fav(5, 4 if i % 3 else 1)) for i in range(30)], [(-0.7, -0.1, fav(5, 3)) for _ in range(20)]]
    pool1 = [int(x) for x in rng.integers(0, 1000, 30)] + [int(x) for x in rng.integers(0, 1000, 10)] * 2
    pb, LL = make_pb([(3, l0), (5, l1)])
    n = int(pb.a["read_off"][-1])
    seed = np.full(n, 3, np.int32); seed[[1, 13, 15, 100]] = -1
    return pb, LL, oracle_map(oracle, pb), seed, np.array(pool0 + pool1, np.int32), np.array([0, 5, 1005], np.int32)


@pytest.fixture(scope="module")
def request_batch(oracle):
    return request_inputs(oracle)


@pytest.mark.parametrize("rule", [capi.ASSIGN_VCF, capi.ASSIGN_RETRACE])
def test_request_list(hmm, request_batch, rule):
    pb, LL, mg, seed, pool, pool_off = request_batch
    assert [sorted(x) for x in mg[:3]] == [[0, 0], [1, 1], [0, 2]]
    got = capi.run_assign(hmm, pb, seed, pool_index=pool, pool_off=pool_off, rule=rule)
    want = check(got, pb, LL, mg, seed, "requests rule %d" % rule, requests=True, pool_index=pool, pool_off=pool_off, rule=rule)
    # shared pools picked different haplotypes; the 70 identical reads made one request; both loci contributed
    keys = list(zip(want["req_read"], want["req_allele"]))
    assert len(set(keys)) == len(keys) and len({a for r, a in keys if r == 0}) >= 2
    assert len(set(want["read_req"][20:90])) == 1 and (want["req_read"] >= 5).any() and want["n_req"] < (seed >= 0).sum()
    # one slot too few: 3 and the exact count; with room: the list
    small = capi.run_assign(hmm, pb, seed, pool_index=pool, pool_off=pool_off, rule=rule, cap_req=want["n_req"] - 1)
    assert small["rc"] == 3 and small["n_req"] == want["n_req"]
    assert b"too small" in hmm.hipstr_last_error()
    again = capi.run_assign(hmm, pb, seed, pool_index=pool, pool_off=pool_off, rule=rule, cap_req=want["n_req"])
    assert again["rc"] == 0
    check(again, pb, LL, mg, seed, "requests, exact room", requests=True, pool_index=pool, pool_off=pool_off, rule=rule)


def test_no_pool_index_leaves_the_request_outputs_untouched(hmm, request_batch):
    pb, LL, mg, seed, pool, pool_off = request_batch
    n = int(pb.a["read_off"][-1])
    _sig_out = capi.HipstrAssignOut
    capi.run_assign(hmm, pb, seed)                                       # (sets the signature)
    k = {f: np.full(n, capi.UNTOUCHED, np.int32 if t is capi._i32p else np.float64) for f, t in _sig_out._fields_[:-1]}
    o = _sig_out(*([k[f].ctypes.data_as(t) for f, t in _sig_out._fields_[:-1]] + [n]))
    sd = np.ascontiguousarray(seed)
    rq = capi.HipstrAssignRequest(sd.ctypes.data_as(capi._i32p), None, None, pool_off.ctypes.data_as(capi._i32p), 0, 0.0)
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd
    try:
        assert hmm.hipstr_post_launch(pd, None) == 0
        assert hmm.hipstr_post_assign(pd, C.byref(rq), C.byref(o)) == 0
    finally:
        hmm.hipstr_post_free(pd)
    for f in ("n_req", "req_read", "req_allele", "read_req"):
        assert np.all(k[f] == capi.UNTOUCHED), f
    assert np.array_equal(k["best_hap"], restate(pb, LL, mg, seed)["best_hap"])


# ------------------------------------------------------------------------------------------------------------------ 5. ordered sum
def test_phase_total_is_summed_in_read_order(hmm, oracle):
    """One sample of 300 reads whose log_phase_one span 40 nats: the exponentials must be added serially in read order — the same values
    added pairwise give another double for this input (asserted: the case bites)."""
    rng = np.random.default_rng(22)                       # (a seed for which the tree sum changes phase1_reads itself, not just the total under the log)
    d = np.concatenate([rng.uniform(-40, 40, 280), [40.0, -40.0], rng.uniform(30, 40, 18)]); rng.shuffle(d)    # LL[1] - LL[0] per read
    reads = [(-0.5, -0.5, [-45.0, -45.0 + float(x)]) for x in d]
    pb, LL = make_pb([(2, [reads])])
    mg = oracle_map(oracle, pb)
    assert tuple(mg[0]) == (0, 1)
    seed = np.full(300, 1, np.int32)
    got = capi.run_assign(hmm, pb, seed)
    want = check(got, pb, LL, mg, seed, "ordered sum")
    lpo = want["log_phase_one"]
    assert lpo.max() - lpo.min() >= 40
    tree = restate(pb, LL, mg, seed, pairwise=True)
    assert tree["phase1_reads"][0] != want["phase1_reads"][0], "the pairwise sum equals the serial one: this input does not tell them apart"
    e, l = _cr_fns()
    assert restate(pb, LL, mg, seed, pairwise=True, exp=e, log=l)["phase1_reads"][0] != got["phase1_reads"][0]


# ------------------------------------------------------------------------------------------------------------------ 6. mixed batch
def test_mixed_batch(hmm, oracle):
    """8 loci, A from 1 to 128, S from 1 to 1000 (one read per sample in the last), host likelihoods, one call."""
    rng = np.random.default_rng(33)
    As = [128, 64, 45, 16, 8, 3, 1, 2]; Ss = [1, 2, 3, 4, 5, 8, 16, 1000]
    loci = []; pool = []; pool_off = [0]; hap = []
    for li, (A, S) in enumerate(zip(As, Ss)):
        samples = []
        for s in range(S):
            nr = 1 if S == 1000 else int(rng.integers(0, 24))
            h1, h2 = int(rng.integers(0, A)), int(rng.integers(0, A))
            reads = []
            for i in range(nr):
                row = -20 - 10 * rng.random(A); row[h1 if i % 2 else h2] = -1 - rng.random()
                p = -rng.random(2) if rng.random() < 0.7 else (-0.4, -0.4)
                reads.append((float(p[0]), float(p[1]), [float(x) for x in row]))
            samples.append(reads)
        loci.append((A, samples))
        nr_l = sum(len(x) for x in samples); npool = 40 if li == 0 else max(1, nr_l // 2)        # 40 x 128 keys: a hashed table
        pool += [int(x) for x in rng.integers(0, npool, nr_l)]; pool_off.append(pool_off[-1] + npool); hap.append(1 if li == 4 else 0)
    pb, LL = make_pb(loci, haploid=hap)
    n = int(pb.a["read_off"][-1])
    seed = np.where(rng.random(n) < 0.1, -1, 7).astype(np.int32)
    reverse = rng.integers(0, 2, n).astype(np.uint8)
    got = capi.run_assign(hmm, pb, seed, reverse=reverse, pool_index=pool, pool_off=pool_off)
    check(got, pb, LL, oracle_map(oracle, pb), seed, "mixed batch", requests=True, reverse=reverse, pool_index=pool, pool_off=pool_off)


# ------------------------------------------------------------------------------------------------------------------ 7. errors
def test_errors_leave_the_device_usable(hmm, oracle, request_batch):
    pb, LL, mg, seed, pool, pool_off = request_batch
    n = int(pb.a["read_off"][-1]); ns = int(pb.samp_off[-1])
    capi.run_assign(hmm, pb, seed)                                       # (sets the signature)
    i32 = lambda m: np.full(m, capi.UNTOUCHED, np.int32)
    k = {f: (i32(max(n, ns)) if t is capi._i32p else np.zeros(max(n, ns))) for f, t in capi.HipstrAssignOut._fields_[:-1]}
    def out(**drop):
        return capi.HipstrAssignOut(*([None if f in drop else k[f].ctypes.data_as(t) for f, t in capi.HipstrAssignOut._fields_[:-1]] + [n]))
    p = lambda x: x.ctypes.data_as(capi._i32p)
    sd = np.ascontiguousarray(seed); bad_pool = pool.copy(); bad_pool[40] = 5; neg_pool = pool.copy(); neg_pool[3] = -1
    def rq(seed=sd, pool_index=pool, pool_off=pool_off, rule=0, tol=0.0):
        return capi.HipstrAssignRequest(None if seed is None else p(seed), None, None if pool_index is None else p(pool_index),
                                        None if pool_off is None else p(pool_off), rule, tol)
    def refused(pd, r, o, word):
        rc = hmm.hipstr_post_assign(pd, C.byref(r) if r is not None else None, C.byref(o) if o is not None else None)
        msg = hmm.hipstr_last_error().decode()
        assert rc != 0 and rc != 3 and word in msg, (rc, msg, word)
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd
    try:
        refused(pd, rq(), out(), "hipstr_post_launch")                   # before the posteriors
        assert hmm.hipstr_post_launch(pd, None) == 0
        refused(None, rq(), out(), "null"); refused(pd, None, out(), "null"); refused(pd, rq(), None, "null")
        refused(pd, rq(seed=None), out(), "null")
        refused(pd, rq(), out(best_hap=1), "null"); refused(pd, rq(), out(phase2_reads=1), "null"); refused(pd, rq(), out(n_req=1), "request-list")
        refused(pd, rq(pool_off=None), out(), "pool_off")
        refused(pd, rq(pool_index=bad_pool), out(), "pool_index"); refused(pd, rq(pool_index=neg_pool), out(), "pool_index")
        refused(pd, rq(rule=2), out(), "rule"); refused(pd, rq(rule=-1), out(), "rule")
        refused(pd, rq(tol=-0.1), out(), "strand_tolerance")
        good = capi.run_assign(hmm, pd, seed, pool_index=pool, pool_off=pool_off, n_reads=n, n_samp=ns)        # the same object, after all that
        check(good, pb, LL, mg, seed, "after the refused calls", requests=True, pool_index=pool, pool_off=pool_off)
    finally:
        hmm.hipstr_post_free(pd)
