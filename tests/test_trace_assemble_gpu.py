"""GPU: hipstr_hmm_trace_ex with HIPSTR_TRACE_ASSEMBLE_DEVICE — the records of a traceback (HapAligner.cpp:363-571, 642-707,
AlignmentTraceback.cpp:7-52, 55-144) assembled by hs_trace_assemble / hs_trace_scan / hs_trace_compact instead of host threads.  Every output is
an integer or a character, so every comparison is exact: against the compiled reference's golden records, and array by array and pool by pool
against the host replay (hipstr_hmm_trace_seeded) of the same requests."""
import glob
import os

import numpy as np
import pytest

from hipstr_amd import capi, shard
import stage_route_cases as src
import util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "trace_*.npz")))
DEVICE = capi.TRACE_ASSEMBLE_DEVICE
NO_STR = -100000                     # HIPSTR_NO_STR_DATA

SEEDED = [
    dict(reads_per_locus=50, n_str_alleles=4, seed=1),
    dict(reads_per_locus=40, n_str_alleles=8, n_flank_opts=2, seed=7),
    dict(reads_per_locus=20, n_str_alleles=16, read_len=250, flank_len=110, str_bp=100, seed=5),
    dict(reads_per_locus=60, n_str_alleles=12, read_len=100, flank_len=35, str_bp=30, seed=3),
    dict(reads_per_locus=24, n_str_alleles=6, read_len=250, flank_len=160, str_bp=60, seed=9),
]
LONG = [
    dict(reads_per_locus=8, n_str_alleles=3, read_len=640, flank_len=400, str_bp=40, seed=31),
    dict(reads_per_locus=6, n_str_alleles=3, read_len=900, flank_len=520, str_bp=36, seed=32),
    dict(reads_per_locus=8, n_str_alleles=2, read_len=1024, flank_len=600, str_bp=30, seed=33),
]

# (pool, its offset array, arrays that share the offsets)
POOLS = [("hap_aln_off", ("hap_aln",)), ("str_seq_off", ("str_seq",)), ("flank_seq_off", ("flank_seq",)), ("indel_off", ("indel_pos", "indel_size")),
         ("snp_off", ("snp_pos", "snp_base")), ("cigar_off", ("cigar_op", "cigar_len")), ("aln_str_off", ("aln_str",))]
SCALARS = ("ll", "max_index", "stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop")


def assert_raw_equal(got, want, n, what=""):
    """Two run_trace(..., unpack=False) results: every offset array, every scalar array, every pool's bytes up to its total."""
    for nm in SCALARS:
        assert np.array_equal(got[nm][:n], want[nm][:n]), "%s: %s differs" % (what, nm)
    for off, arrays in POOLS:
        m = (2 * n if off == "flank_seq_off" else n) + 1
        assert np.array_equal(got[off][:m], want[off][:m]), "%s: %s differs" % (what, off)
        total = int(want[off][m - 1])
        for nm in arrays:
            g, w = got[nm], want[nm]
            if isinstance(w, np.ndarray):
                assert np.array_equal(g[:total], w[:total]), "%s: pool %s differs" % (what, nm)
            else:
                assert g.raw[:total] == w.raw[:total], "%s: pool %s differs" % (what, nm)


def both_raw(hmm, bptr, rr, aa, h2r, seeds=None, cap=1 << 21, what=""):
    want = capi.run_trace(hmm, "hipstr_hmm_", bptr, rr, aa, h2r, cap=cap, unpack=False, req_seed=seeds)
    got = capi.run_trace(hmm, "hipstr_hmm_", bptr, rr, aa, h2r, cap=cap, unpack=False, req_seed=seeds, flags=DEVICE)
    assert_raw_equal(got, want, len(rr), what)
    return got


def _requests(oracle, sb, per_read, seed):
    _, seeds = capi.run_align(oracle, "oracle_", sb.ptr)
    A = sb.n_out // sb.n_reads
    rng = np.random.default_rng(seed)
    rr, aa = [], []
    for r in range(sb.n_reads):
        if seeds[r] >= 0:
            for k in rng.choice(A, size=min(A, per_read), replace=False):
                rr.append(r); aa.append(int(k))
    return rr, aa


# ------------------------------------------------------------------ goldens
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[6:-4] for p in FIXTURES])
def test_device_assembly_matches_golden(hmm, path):
    for b, rr, aa, h2r, exp in util.load_trace_fixture(path):
        got = capi.run_trace(hmm, "hipstr_hmm_", b.ptr, rr, aa, h2r, cap=1 << 20, flags=DEVICE)
        util.assert_traces_equal(got, exp, os.path.basename(path))


# ------------------------------------------------------------------ against the host path, raw
@pytest.mark.parametrize("kw", SEEDED + LONG, ids=lambda kw: "seed%d" % kw["seed"])
def test_device_assembly_equals_host_replay_on_seeded_loci(hmm, oracle, kw):
    sb = capi.SynthBatch(n_loci=1, **kw)
    rr, aa = _requests(oracle, sb, 3 if kw in SEEDED else 2, kw["seed"])
    h2r = util.synthetic_hap_to_ref(oracle, sb.ptr)
    both_raw(hmm, sb.ptr, rr, aa, h2r, cap=1 << 22, what=str(kw))


def test_device_assembly_equals_host_replay_on_boundary_sides(hmm, oracle):
    """Sides of 1, 64 | 65 ... 1024 columns, reads that miss the STR block, interrupted alleles (stage_route_cases' call)."""
    call = src.trace_boundary_sides(src.limits(hmm)["trace"])
    both_raw(hmm, call.batch.ptr, call.rr, call.aa, src.h2r_of(oracle, call), seeds=call.seeds, cap=1 << 22, what=call.name)


def _five_loci(oracle):
    sb = capi.SynthBatch(n_loci=5, reads_per_locus=30, n_str_alleles=6, n_flank_opts=2, seed=71)
    whole = util.synth_to_batch(sb)
    a = whole.arrays
    _, seeds = capi.run_align(oracle, "oracle_", sb.ptr)
    rng = np.random.default_rng(71)
    rr, aa, h2r_all, cuts = [], [], [], []
    for l in range(5):
        r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1])
        A = int(a["hap_off"][l + 1] - a["hap_off"][l])
        one = shard.batch_from_arrays(shard.subset_arrays(a, l, l + 1))
        h2r = util.synthetic_hap_to_ref(oracle, one.ptr)
        h2r_all += h2r
        lr = [r for r in range(r0, r1) if seeds[r] >= 0]
        la = [int(rng.integers(A)) for _ in lr]
        cuts.append((one, [r - r0 for r in lr], la, h2r))
        rr += lr; aa += la
    return sb, whole, rr, aa, h2r_all, cuts, rng


def test_device_assembly_of_many_loci_permuted_and_of_a_few_requests(hmm, oracle):
    sb, whole, rr, aa, h2r_all, cuts, rng = _five_loci(oracle)
    order = rng.permutation(len(rr))                 # requests need not be grouped by locus
    got = both_raw(hmm, whole.ptr, [rr[i] for i in order], [aa[i] for i in order], h2r_all, what="permuted")
    # (and the offsets really index the pools: unpacked, against the oracle locus by locus)
    want = []
    for one, lr, la, h2r in cuts:
        want += capi.run_trace(oracle, "oracle_", one.ptr, lr, la, h2r, cap=1 << 20)
    unpacked = capi.run_trace(hmm, "hipstr_hmm_", whole.ptr, [rr[i] for i in order], [aa[i] for i in order], h2r_all, cap=1 << 21, flags=DEVICE)
    util.assert_traces_equal(unpacked, [want[i] for i in order])
    # a few requests of a large batch: only the requested reads' bases travel (the compacted-reads route)
    a = whole.arrays
    few = [i for i in range(len(rr)) if rr[i] >= int(a["read_off"][4])][:7]
    few = few + few[:1]
    plan = capi.trace_plan(hmm, whole.ptr, [rr[i] for i in few], [aa[i] for i in few])
    assert plan["compact_reads"] is True
    both_raw(hmm, whole.ptr, [rr[i] for i in few], [aa[i] for i in few], h2r_all, what="few")


# ------------------------------------------------------------------ coverage, judged on the oracle's records
def hand_built_locus():
    """One locus through capi's locus builder: flank options with an insertion and a deletion against option 0 (so the oracle's
    hap_to_ref strings carry 'I' and 'D' in the flanks), reads with a flank insertion, a flank deletion, a flank mismatch of high and of
    low base quality, a read that ends inside the left flank, reads that start inside a flank insertion, and reads that overhang either end
    of the haplotype; caller seeds put the seed base into every block and at both ends of the haplotype."""
    rng = np.random.default_rng(20260)
    seq = lambda n: "".join(rng.choice(list("ACGT"), n))
    lf, rf = seq(48), seq(48)
    strs = ["CAG" * 8, "CAG" * 10, "CAG" * 6]
    lf_ins = lf[:20] + "TTGA" + lf[20:]; lf_del = lf[:30] + lf[34:]
    rf_ins = rf[:20] + "ACCT" + rf[20:]; rf_del = rf[:12] + rf[16:]
    hap = lf + strs[0] + rf
    reads = []       # (sequence, quals, offset, realign)
    def add(s, q=None, off=0):
        reads.append((s, q, off, True))
    add(hap[10:110])                                                        # 0 plain
    add((lf + strs[1] + rf)[10:116])                                        # 1 two more repeats
    add((lf + strs[2] + rf)[10:104])                                        # 2 two repeats fewer
    add(hap[5:25] + "GT" + hap[25:100], off=5)                              # 3 insertion in the left flank
    add(hap[5:22] + hap[26:100], off=5)                                     # 4 deletion in the left flank
    mm = hap[8:30] + ("A" if hap[30] != "A" else "C") + hap[31:100]
    add(mm, off=8)                                                          # 5 flank mismatch, high quality
    add(mm, "F" * 22 + "#" + "F" * (len(mm) - 23), off=8)                   # 6 the same base with quality 2
    add(hap[2:44], off=2)                                                   # 7 inside the left flank
    add(hap[len(lf) + 24 + 6:], off=len(lf) + 30)                           # 8 inside the right flank
    add(seq(12) + hap[:60], off=-12)                                        # 9 overhangs the left end
    add(hap[-60:] + seq(12), off=len(hap) - 60)                             # 10 overhangs the right end
    add((lf_ins + strs[0] + rf)[21:110], off=20)                            # 11 starts inside the left flank's insertion
    add((lf + strs[0] + rf_ins)[40:], off=40)                               # 12 covers the right flank's insertion
    add((lf_del + strs[0] + rf_del)[5:], off=5)                             # 13 the deletions' haplotype
    b, A = util.simple_locus(lf, strs, rf, 3, reads, lf_opts=[lf_ins, lf_del], rf_opts=[rf_ins, rf_del])
    b.finalize()
    rr, aa, ss = [], [], []
    for r, rd in enumerate(reads):
        n = len(rd[0])
        for k in range(A):
            for s in sorted({1, 12, n // 3, n // 2, (2 * n) // 3, n - 13, n - 2}):
                if 1 <= s <= n - 2:
                    rr.append(r); aa.append(k); ss.append(s)
    return b, rr, aa, ss


def block_lengths(oracle, bptr):
    """[F0, B, F2] of every allele of a one-locus batch."""
    import ctypes as C
    b = bptr.contents if hasattr(bptr, "contents") else (bptr._obj if hasattr(bptr, "_obj") else bptr)
    nopts = np.ctypeslib.as_array(b.blk_nopts, shape=(3,)).astype(np.int32)
    opt_off = np.ctypeslib.as_array(b.opt_off, shape=(int(nopts.sum()) + 1,))
    lens, cur = [], 0
    for k in range(3):
        lens.append([int(opt_off[cur + o + 1] - opt_off[cur + o]) for o in range(nopts[k])])
        cur += int(nopts[k])
    out, opts, i32p = [], np.zeros(3, np.int32), C.POINTER(C.c_int32)
    for k in range(int(np.prod(nopts))):
        oracle.oracle_allele_options(nopts.ctypes.data_as(i32p), k, opts.ctypes.data_as(i32p))
        out.append([lens[x][opts[x]] for x in range(3)])
    return out


def coverage(records, alleles, h2r, blens, into):
    """What the oracle's records of some requests show (records[i] is request i's, traced on allele alleles[i])."""
    for w, k in zip(records, alleles):
        F0, B, F2 = blens[k]
        H, mx, s = F0 + B + F2, w["max_index"], w["stutter_size"]
        into.add("stutter>0" if (s > 0 and s != NO_STR) else "stutter<0" if (s < 0 and s != NO_STR) else "stutter==0" if s == 0 else "no_str_data")
        into.add("seed_in_block_%d" % (0 if mx < F0 else 1 if mx < F0 + B else 2))
        if mx == 0 or mx == H - 1:
            into.add("seed_at_an_end")
        if w["flank_ins"] > 0:
            into.add("flank_ins")
        if w["flank_del"] > 0:
            into.add("flank_del")
        if "ID" in w["hap_aln"] or "DI" in w["hap_aln"]:
            into.add("ins_next_to_del")
        if w["snps"]:
            into.add("snp")
        # the seed's place in hap_to_ref: stitch_alignment_trace's walk (AlignmentTraceback.cpp:64-75)
        t, hi, i = h2r[k].decode(), mx, 0
        while hi > 0 and i < len(t):
            hi -= t[i] in "MI"; i += 1
        for ch in "ID":
            if ch in t[:i]:
                into.add("h2r_%s_left" % ch)
            if ch in t[i + 1:]:
                into.add("h2r_%s_right" % ch)
        lead = lambda x: len(x) - len(x.lstrip("S"))
        cig = w["cigar"]
        if cig and cig.lstrip("0123456789")[:1] == "S" and int(cig[:len(cig) - len(cig.lstrip("0123456789"))]) > lead(w["hap_aln"]):
            into.add("leading_I_to_S")


WANTED = {"stutter>0", "stutter<0", "stutter==0", "no_str_data", "seed_in_block_0", "seed_in_block_2", "seed_at_an_end",
          "flank_ins", "flank_del", "snp", "snp_suppressed", "h2r_I_left", "h2r_I_right", "h2r_D_left", "h2r_D_right", "leading_I_to_S"}


def covered_by_the_inputs(oracle):
    seen = set()
    for kw in SEEDED[:2]:
        sb = capi.SynthBatch(n_loci=1, **kw)
        rr, aa = _requests(oracle, sb, 3, kw["seed"])
        h2r = util.synthetic_hap_to_ref(oracle, sb.ptr)
        coverage(capi.run_trace(oracle, "oracle_", sb.ptr, rr, aa, h2r, cap=1 << 21), aa, h2r, block_lengths(oracle, sb.ptr), seen)
    b, rr, aa, ss = hand_built_locus()
    h2r = capi.hap_aln_info(oracle, "oracle_", b.ptr)
    rec = capi.run_trace(oracle, "oracle_", b.ptr, rr, aa, h2r, cap=1 << 22, req_seed=ss)
    coverage(rec, aa, h2r, block_lengths(oracle, b.ptr), seen)
    # reads 5 and 6 are one sequence; read 6's mismatching base has quality 2: the SNP the first records and the second does not
    by = {(r, k, s): w for r, k, s, w in zip(rr, aa, ss, rec)}
    if any(r == 5 and w["snps"] and not by[(6, k, s)]["snps"] and w["hap_aln"] == by[(6, k, s)]["hap_aln"] for (r, k, s), w in by.items()):
        seen.add("snp_suppressed")
    return seen, (b, rr, aa, ss, h2r, rec)


def test_hand_built_locus_and_the_coverage_of_the_inputs(hmm, oracle):
    """The cases the replay has to get right appear in the ORACLE's records of the inputs of this file (two seeded shapes and the hand-built
    locus): every entry of WANTED.  Not asserted: an insertion run directly followed by a deletion run.  retrace leaves an insertion only
    into a match and a deletion only into a match (HapAligner.cpp:536-566: from I the choices are I and M, from D they are D and M), so no
    operation string holds 'I' next to 'D' inside a flank and no input reaches the case; the STR block's artifact is bounded by matches on
    the flank side ("stutter block must be followed by a match").  Not asserted either: a seed position inside the STR block.
    compute_aln_logprob offers the flank positions only (HapAligner.cpp:184-222: the seed base is never aligned into the repeat), so max_index
    lies in block 0 or block 2 for every input; both are asserted, as is a seed at position 0 or H - 1."""
    seen, (b, rr, aa, ss, h2r, rec) = covered_by_the_inputs(oracle)
    assert WANTED <= seen, sorted(WANTED - seen)
    got = capi.run_trace(hmm, "hipstr_hmm_", b.ptr, rr, aa, h2r, cap=1 << 22, req_seed=ss, flags=DEVICE)
    util.assert_traces_equal(got, rec, "hand-built locus")
    both_raw(hmm, b.ptr, rr, aa, h2r, seeds=ss, cap=1 << 22, what="hand-built locus")


# ------------------------------------------------------------------ other behaviour
def _small(oracle, seed=21, reads=40, alleles=6, per_read=2):
    sb = capi.SynthBatch(n_loci=1, reads_per_locus=reads, n_str_alleles=alleles, seed=seed)
    rr, aa = _requests(oracle, sb, per_read, seed)
    return sb, rr, aa, util.synthetic_hap_to_ref(oracle, sb.ptr)


def test_without_reference_strings_the_stitched_fields_are_empty(hmm, oracle):
    sb, rr, aa, _ = _small(oracle, seed=12, reads=12, alleles=4)
    got = both_raw(hmm, sb.ptr, rr, aa, None, what="no hap_to_ref")
    n = len(rr)
    assert not got["cigar_off"][:n + 1].any() and not got["aln_str_off"][:n + 1].any()
    assert not got["aln_start"][:n].any() and not got["aln_stop"][:n].any()


def test_offsets_carry_across_chunks(hmm, oracle, monkeypatch):
    """HIPSTR_TRACE_WS_MIB counts whole MiB: 1 is the smallest budget, and 240 requests of about 18 KB of decisions each fill four of them."""
    sb, rr, aa, h2r = _small(oracle, per_read=6)
    whole = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=DEVICE)
    monkeypatch.setenv("HIPSTR_TRACE_WS_MIB", "1")
    assert len(capi.trace_plan(hmm, sb.ptr, rr, aa)["chunks"]) >= 3
    pieces = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=DEVICE)
    assert_raw_equal(pieces, whole, len(rr), "chunked")
    both_raw(hmm, sb.ptr, rr, aa, h2r, what="chunked, against the host path")


def test_one_host_thread(hmm, oracle, monkeypatch):
    sb, rr, aa, h2r = _small(oracle)
    whole = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=DEVICE)
    monkeypatch.setenv("HIPSTR_HOST_THREADS", "1")
    one = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=DEVICE)
    assert_raw_equal(one, whole, len(rr), "HIPSTR_HOST_THREADS=1")


def test_errors_flags_and_the_empty_call(hmm, oracle):
    sb = capi.SynthBatch(n_loci=1, reads_per_locus=4, n_str_alleles=2, seed=62)
    with pytest.raises(RuntimeError, match="allele outside"):
        capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, [0], [99], None, flags=DEVICE)
    with pytest.raises(RuntimeError, match="read outside"):
        capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, [99], [0], None, flags=DEVICE)
    with pytest.raises(RuntimeError, match=r"too small \(cap_chars\)"):
        capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, [0, 1, 2, 3], [0, 0, 0, 0], None, cap=64, flags=DEVICE)
    assert capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, [], [], None, flags=DEVICE) == []
    for bad in (2, 3, 1 << 31):
        with pytest.raises(RuntimeError, match="unknown flag"):
            capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, [0], [0], None, flags=bad)
    h2r = util.synthetic_hap_to_ref(oracle, sb.ptr)
    rr, aa = [0, 1, 2, 3, 0], [0, 1, 0, 1, 1]
    seeded = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, req_seed=[-2] * 5)      # HIPSTR_SEED_AUTO
    zero = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, unpack=False, flags=0)
    assert_raw_equal(zero, seeded, 5, "flags=0")
    # one walk over the request list behind the plans and the three calls: the refusals of tests/test_stage_routes.py, the plan's words
    for c in src.trace_refusals(capi.trace_plan(hmm, sb.ptr, [], [])["thresholds"]):
        with pytest.raises(RuntimeError) as planned:
            capi.trace_plan(hmm, c.batch.ptr, c.rr, c.aa, c.seeds)
        said = str(planned.value).split("failed: ", 1)[1]
        assert said == c.message
        for call in (lambda: capi.run_trace(hmm, "hipstr_hmm_", c.batch.ptr, c.rr, c.aa, None, req_seed=c.seeds, flags=0),
                     lambda: capi.run_trace(hmm, "hipstr_hmm_", c.batch.ptr, c.rr, c.aa, None, req_seed=c.seeds, flags=DEVICE),
                     lambda: capi.run_trace_resident(hmm, c.batch.ptr, c.rr, c.aa, None, req_seed=c.seeds)):
            with pytest.raises(RuntimeError) as e:
                call()
            assert str(e.value).endswith(said), (c.name, str(e.value))


def test_a_request_beyond_the_lds_threshold_reads_hbm(hmm, oracle):
    """The smallest read length (flanks 0.6 of it, as the long-side shapes) whose staging — ops of both sides, read, flags, flank bases,
    hap_to_ref, stitched string — crosses the plan's HS_ASM_LDS: its requests take the HBM route, one step shorter stays in LDS."""
    def shape(n):
        sb = capi.SynthBatch(n_loci=1, reads_per_locus=4, n_str_alleles=2, read_len=n, flank_len=(6 * n) // 10, str_bp=30, seed=35)
        rr, aa = _requests(oracle, sb, 2, 35)
        h2r = util.synthetic_hap_to_ref(oracle, sb.ptr)
        return sb, rr, aa, h2r, capi.trace_assemble_plan(hmm, sb.ptr, rr, aa, None, h2r)
    lim = shape(100)[4]["thresholds"]["HS_ASM_LDS"]
    n = 64
    while "assemble_hbm" not in shape(n)[4]["routes_hit"]:
        n += 64
        assert n <= 1024
    sb, rr, aa, h2r, plan = shape(n)
    assert any(q[5] > lim and q[6] == 0 for q in plan["requests"])
    assert shape(n - 64)[4]["routes_hit"] == ["assemble_lds"]
    both_raw(hmm, sb.ptr, rr, aa, h2r, cap=1 << 22, what="HBM route")
