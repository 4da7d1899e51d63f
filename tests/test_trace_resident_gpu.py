"""GPU: the resident traceback result — hipstr_hmm_trace_resident, hipstr_trace_dev_sizes / _fetch / _free — and its two consumers,
hipstr_post_census_dev and hipstr_assign_trace_stats_dev (include/hipstr_hmm.h).

Nothing here has a yardstick of its own: a resident result fetched whole must be the bytes hipstr_hmm_trace_ex writes (held to the compiled
reference's golden records and, raw, to the host replay), the census through the handle must be hipstr_post_census on the same arrays (and
tests/test_census_gpu.py's restatement, whose case builders are imported), the read counts must be hipstr_assign_trace_stats on the fetched
scalars.  Every comparison is exact: integers, bytes, flags and the bits of ll.  Every refusal is decided on the host before a launch or from
a flag a kernel wrote; no case provokes a fault."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from hipstr_amd import capi
import stage_route_cases as src
import test_assign_gpu as ta
import test_census_gpu as tc
import test_poison_gpu as tp
import test_readmat_gpu as trm
import test_trace_assemble_gpu as tta
import util

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "trace_*.npz")))
NO_STR = -100000                     # HIPSTR_NO_STR_DATA
ALL = capi.TRACE_F_ALL
SENT = capi.TRACE_SENTINEL
POOL_OFFS = ("hap_aln_off", "str_seq_off", "flank_seq_off", "indel_off", "snp_off", "cigar_off", "aln_str_off")     # hipstr_trace_dev_sizes' order


def raw_bytes(a):
    return a.tobytes() if isinstance(a, np.ndarray) else a.raw


def untouched(a):
    return raw_bytes(a) == bytes([SENT]) * len(raw_bytes(a))


def fetch_all(hmm, td):
    """Everything, with hipstr_trace_dev_sizes held to the last entries of the fetched offsets."""
    n, tot = td.sizes()
    keep = capi.trace_dev_fetch(hmm, td, ALL)
    for p, off in enumerate(POOL_OFFS):
        assert int(keep[off][(2 * n if p == 2 else n)]) == int(tot[p]) and int(keep[off][0]) == 0, off
    return keep, n


def resident(hmm, bptr, rr, aa, h2r, seeds=None):
    td = capi.run_trace_resident(hmm, bptr, rr, aa, h2r, req_seed=seeds)
    try:
        keep, n = fetch_all(hmm, td)
    finally:
        td.close()
    assert n == len(rr)
    return keep


def equals_host_replay(hmm, bptr, rr, aa, h2r, seeds=None, cap=1 << 22, what=""):
    want = capi.run_trace(hmm, "hipstr_hmm_", bptr, rr, aa, h2r, cap=cap, unpack=False, req_seed=seeds, flags=0)
    got = resident(hmm, bptr, rr, aa, h2r, seeds)
    tta.assert_raw_equal(got, want, len(rr), what)
    return got


# ------------------------------------------------------------------ 1. goldens
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[6:-4] for p in FIXTURES])
def test_resident_result_matches_golden(hmm, path):
    for b, rr, aa, h2r, exp in util.load_trace_fixture(path):
        keep = resident(hmm, b.ptr, rr, aa, h2r)
        util.assert_traces_equal(capi.unpack_trace(keep, len(rr)), exp, os.path.basename(path))


# ------------------------------------------------------------------ 2. raw equality with the existing calls
@pytest.mark.parametrize("kw", tta.SEEDED[:2] + tta.LONG[:1], ids=lambda kw: "seed%d" % kw["seed"])
def test_equals_host_replay_on_seeded_loci(hmm, oracle, kw):
    sb = capi.SynthBatch(n_loci=1, **kw)
    rr, aa = tta._requests(oracle, sb, 3 if kw in tta.SEEDED else 2, kw["seed"])
    equals_host_replay(hmm, sb.ptr, rr, aa, util.synthetic_hap_to_ref(oracle, sb.ptr), what=str(kw))


def test_equals_host_replay_on_the_hand_built_locus(hmm, oracle):
    b, rr, aa, ss = tta.hand_built_locus()
    equals_host_replay(hmm, b.ptr, rr, aa, capi.hap_aln_info(oracle, "oracle_", b.ptr), seeds=ss, what="hand-built locus")


def test_equals_host_replay_on_boundary_sides(hmm, oracle):
    call = src.trace_boundary_sides(src.limits(hmm)["trace"])
    equals_host_replay(hmm, call.batch.ptr, call.rr, call.aa, src.h2r_of(oracle, call), seeds=call.seeds, what=call.name)


def test_without_reference_strings_few_requests_and_a_repeated_request(hmm, oracle):
    sb, rr, aa, h2r = tta._small(oracle, seed=12, reads=12, alleles=4)
    got = equals_host_replay(hmm, sb.ptr, rr, aa, None, what="no hap_to_ref")
    n = len(rr)
    assert not got["cigar_off"][:n + 1].any() and not got["aln_str_off"][:n + 1].any()
    assert not got["aln_start"][:n].any() and not got["aln_stop"][:n].any()
    equals_host_replay(hmm, sb.ptr, [], [], h2r, what="n_req 0")
    equals_host_replay(hmm, sb.ptr, rr[:1], aa[:1], h2r, what="n_req 1")
    twice = equals_host_replay(hmm, sb.ptr, [rr[3], rr[0], rr[3]], [aa[3], aa[0], aa[3]], h2r, what="the same request twice")
    rec = capi.unpack_trace(twice, 3)
    assert rec[0] == rec[2]


# ------------------------------------------------------------------ census helpers
def census_both(hmm, c, td, pb=None, dev_ll=None, **kw):
    """hipstr_post_census_dev on the handle and hipstr_post_census on the case's host arrays: the same dict."""
    a = dict(hap_to_allele=c.h2a); a.update(kw)
    dev = capi.run_census(hmm, c.pb if pb is None else pb, c.batch.ptr, c.seed, c.read_req, c.req_read, None, dev_ll=dev_ll, td=td, **a)
    host = capi.run_census(hmm, c.pb if pb is None else pb, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, dev_ll=dev_ll, **a)
    assert dev["rc"] == host["rc"]
    assert dev["cand"] == host["cand"]
    for k in tc.KEYS:
        assert np.array_equal(dev[k], host[k]), k
    return dev


def case_handle(hmm, c):
    return capi.trace_dev_from_host(hmm, c.trace, len(c.req_read))


def census_case(hmm, oracle, c, what, **kw):
    """A fabricated case of tests/test_census_gpu.py through hipstr_debug_trace_dev_from_host + hipstr_post_census_dev, against that file's
    restatement and against hipstr_post_census."""
    td = case_handle(hmm, c)
    try:
        got = census_both(hmm, c, td, **kw)
    finally:
        td.close()
    r = {k: v for k, v in kw.items() if k in ("h2a", "min_reads", "min_frac")}
    if "sample_uncallable" in kw:
        r["uncallable"] = kw["sample_uncallable"]
    if "hap_to_allele" in kw:
        r["h2a"] = kw["hap_to_allele"]
    want = tc.restate(c, ta.oracle_map(oracle, c.pb), **r)
    tc.compare(got, want, what)
    return got, want


# ------------------------------------------------------------------ 3. chunks
def test_chunked_call_and_the_census_on_its_handle(hmm, oracle, monkeypatch):
    sb, rr, aa, h2r = tta._small(oracle, per_read=6)
    n = len(rr)
    whole = resident(hmm, sb.ptr, rr, aa, h2r)
    monkeypatch.setenv("HIPSTR_TRACE_WS_MIB", "1")
    assert len(capi.trace_plan(hmm, sb.ptr, rr, aa)["chunks"]) >= 3
    td = capi.run_trace_resident(hmm, sb.ptr, rr, aa, h2r)
    try:
        pieces, _ = fetch_all(hmm, td)
        tta.assert_raw_equal(pieces, whole, n, "chunked against one chunk")
        monkeypatch.delenv("HIPSTR_TRACE_WS_MIB")
        tta.assert_raw_equal(pieces, capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, rr, aa, h2r, cap=1 << 22, unpack=False, flags=0), n, "chunked against the host path")
        # the census on the chunked handle: a read per request, two samples, the batch's own blocks
        b = sb.ptr.contents
        nopts = [int(x) for x in np.ctypeslib.as_array(b.blk_nopts, shape=(3,))]
        A = nopts[0] * nopts[1] * nopts[2]
        rng = np.random.default_rng(5)
        rows = [(-float(rng.random()), -float(rng.random()), [-float(9 * rng.random()) for _ in range(A)]) for _ in range(n)]
        c = tc.Case()
        c.pb, c.LL = ta.make_pb([(A, [rows[:n // 2], rows[n // 2:]])])
        c.batch = sb; c.seed = np.full(n, 5, np.int32); c.read_req = np.arange(n, dtype=np.int32); c.req_read = np.asarray(rr, np.int32)
        c.trace = pieces; c.h2a = [np.asarray(x, np.int32) for x in tc.gray_h2a(nopts)]
        got = census_both(hmm, c, td, min_frac=0.01)
        assert got["n_spanning"].sum() > 0
    finally:
        td.close()


# ------------------------------------------------------------------ 4. selective fetch
def test_selective_fetch(hmm, oracle):
    sb, rr, aa, h2r = tta._small(oracle, seed=12, reads=12, alleles=4)
    td = capi.run_trace_resident(hmm, sb.ptr, rr, aa, h2r)
    try:
        everything, n = fetch_all(hmm, td)
        _, tot = td.sizes()
        assert all(int(t) > 0 for t in tot[[0, 1, 2, 5, 6]])
        for bit, arrays in capi.TRACE_GROUPS.items():
            mine = {nm for nm, _, _ in arrays}
            got = capi.trace_dev_fetch(hmm, td, bit, null_others=True)
            for nm, a in got.items():
                if nm in mine:
                    assert raw_bytes(a) == raw_bytes(everything[nm]), nm
                else:
                    assert untouched(a), "fetch of 0x%02x wrote %s" % (bit, nm)
            again = capi.trace_dev_fetch(hmm, td, bit)              # the others' arrays given, and still neither read nor written
            assert all(raw_bytes(again[nm]) == raw_bytes(got[nm]) for nm in got), "0x%02x fetched twice" % bit
            pools = sorted({p for _, _, p in arrays if p is not None})
            need = max([int(tot[p]) for p in pools], default=0)
            if need > 0:
                with pytest.raises(RuntimeError, match=r"too small \(cap_chars\)") as e:
                    capi.trace_dev_fetch(hmm, td, bit, cap=need - 1)
                assert all(untouched(a) for a in e.value.keep.values()), "a refused fetch wrote"
                exact = capi.trace_dev_fetch(hmm, td, bit, cap=need)
                assert all(raw_bytes(exact[nm]) == raw_bytes(got[nm]) for nm in got)
        # a chosen array that is NULL
        o = capi.HipstrTraceOut(); o.cap_chars = 1 << 20
        assert hmm.hipstr_trace_dev_fetch(td.h, capi.TRACE_F_SCALARS, C.byref(o)) != 0 and b"null output" in hmm.hipstr_last_error()
    finally:
        td.close()


# ------------------------------------------------------------------ 5. census
@pytest.mark.parametrize("min_reads,min_frac", [(0, 0.0), (3, 0.1), (1, 0.5)], ids=["defaults", "3_reads_a_tenth", "1_read_a_half"])
def test_census_thresholds(hmm, oracle, min_reads, min_frac):
    c = tc.thresholds_case()
    td = case_handle(hmm, c)
    try:
        got = census_both(hmm, c, td, min_reads=min_reads, min_frac=min_frac)
    finally:
        td.close()
    tc.compare(got, tc.restate(c, ta.oracle_map(oracle, c.pb), min_reads=min_reads or 2, min_frac=min_frac or 0.15), "thresholds")


def test_census_content_strings_and_strict_spanning(hmm, oracle):
    got, _ = census_case(hmm, oracle, tc.content_case(), "content")
    assert got["cand"] == [[b"ACACACAC"], [], [b"ACACACAC"]]
    c, strs = tc.strings_case()
    got, _ = census_case(hmm, oracle, c, "strings", min_frac=1e-6)
    assert b"" in got["cand"][0] and got["cand"][1] == [b"A", b"AA", b"AC", b"CA"]          # the empty string: a key and a candidate
    got, _ = census_case(hmm, oracle, tc.strict_case(), "strict")
    assert list(got["n_spanning"]) == [7, 5] and list(got["n_span_stutter"]) == [3, 3]


def test_census_called_and_spanned(hmm, oracle):
    c = tc.called_case()
    unc = [0, 1, 0, 0, 0]
    census_case(hmm, oracle, c, "called", sample_uncallable=unc)
    got, _ = census_case(hmm, oracle, c, "called, block 1 not wanted", hap_to_allele=[c.h2a[0], None, c.h2a[2]], sample_uncallable=unc)
    assert np.all(got["called"][2:4] == tc.FILL) and np.all(got["spanned"] == tc.FILL)
    c = tc.spanned_case()
    got, _ = census_case(hmm, oracle, c, "spanned, the third rule")
    for l, (name, _) in enumerate(tc.PROBES):
        assert list(got["spanned"][4 * l + 1:4 * l + 3]) == ([1, 0] if tc.PICK[name] == 0 else [0, 1]), name


@pytest.mark.parametrize("idx", range(14))
def test_census_route_and_size_edges(hmm, oracle, idx):
    cases = tc.route_cases(hmm)
    assert len(cases) == 14
    name, nq, nr, route = cases[idx]
    assert capi.census_plan(hmm, nq, nr)["route"] == route
    census_case(hmm, oracle, tc.build([tc.route_locus(nq, nr, np.random.default_rng(100 + idx))]), name, min_frac=0.02)


def test_census_mixed_routes_with_empty_loci(hmm, oracle):
    got, want = census_case(hmm, oracle, tc.mixed_case(hmm), "mixed", min_frac=0.02)
    assert sum(len(x) for x in want["cand"]) >= 1


def _outputs_untouched(e):
    o = e.value.outputs
    for nm in ("cand_off", "cand_req", "cand_seq_off", "new_n_haps", "n_spanning", "n_span_stutter"):
        assert np.all(o[nm] == capi.UNTOUCHED), nm
    assert np.all(o["called"] == tc.FILL) and np.all(o["spanned"] == tc.FILL) and not any(o["cand_seq"])


def test_census_capacities_and_the_refusals_decided_on_the_device(hmm, oracle):
    c = tc.content_case()
    want = tc.restate(c, ta.oracle_map(oracle, c.pb))
    need = int(want["cand_off"][-1]); chars = sum(len(s) for x in want["cand"] for s in x)
    assert need == 2 and chars == 16
    args = (c.pb, c.batch.ptr, c.seed, c.read_req, c.req_read, None)
    td = case_handle(hmm, c)
    try:
        small = capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td, cap_cand=need - 1)
        assert small["rc"] == 3 and np.array_equal(small["cand_off"], want["cand_off"]) and b"too small" in hmm.hipstr_last_error()
        small = capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td, cap_cand=need, cap_chars=chars - 1)
        assert small["rc"] == 3 and np.array_equal(small["cand_off"], want["cand_off"]) and b"too small" in hmm.hipstr_last_error()
        tc.compare(capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td, cap_cand=need, cap_chars=chars), want, "exact room")
    finally:
        td.close()
    # a decreasing str_seq_off: found by hs_census_check_kernel before any census kernel follows the offsets
    t = dict(c.trace); t["str_seq_off"] = c.trace["str_seq_off"].copy(); t["str_seq_off"][2] = 3
    td = capi.trace_dev_from_host(hmm, t, len(c.req_read))
    try:
        with pytest.raises(RuntimeError, match="str_seq_off must not decrease") as e:
            capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td)
        _outputs_untouched(e)
    finally:
        td.close()
    t = dict(c.trace); t["str_seq_off"] = c.trace["str_seq_off"].copy(); t["str_seq_off"][0] = -1
    td = capi.trace_dev_from_host(hmm, t, len(c.req_read))
    try:
        with pytest.raises(RuntimeError, match="str_seq_off must not be negative"):
            capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td)
    finally:
        td.close()
    # a spanning request without STR data, used by a read with a seed: the documented message, nothing in out
    t = dict(c.trace); t["stutter_size"] = [-4, NO_STR, -4, 4, -4, 4]
    td = capi.trace_dev_from_host(hmm, t, len(c.req_read))
    try:
        with pytest.raises(RuntimeError, match=r"a spanning request without STR data \(AlignmentTrace::stutter_size asserts\)") as e:
            capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td)
        assert "rc=3" not in str(e.value)
        _outputs_untouched(e)
        with pytest.raises(RuntimeError, match="without STR data"):
            capi.run_census(hmm, c.pb, c.batch.ptr, c.seed, c.read_req, c.req_read, t, hap_to_allele=c.h2a)
    finally:
        td.close()
    # ... one that does not span, or that no read with a seed uses, is not looked at
    t["aln_start"] = [50, 100, 50, 50, 50, 50]
    td = capi.trace_dev_from_host(hmm, t, len(c.req_read))
    try:
        ok = capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td)
        assert ok["rc"] == 0 and list(ok["n_spanning"]) == [1, 1, 1, 2, 2]
    finally:
        td.close()
    # a handle without the census' fields
    td = capi.trace_dev_from_host(hmm, dict(c.trace, aln_stop=None), len(c.req_read))
    try:
        with pytest.raises(RuntimeError, match="aln_stop"):
            capi.run_census(hmm, *args, hap_to_allele=c.h2a, td=td)
    finally:
        td.close()


def run_chain_resident(hmm, k, stats=False):
    """tests/test_census_gpu.py's run_chain with the traces resident: forward -> hipstr_rm_scatter -> posteriors -> hipstr_post_assign(RETRACE)
    -> hipstr_hmm_trace_resident -> hipstr_post_census_dev (-> hipstr_assign_trace_stats_dev -> fetch(FLANKS)) -> hipstr_trace_dev_free."""
    dev = trm.upload_and_align(hmm, k.b); rm = None; pd = None; td = None
    try:
        rm = capi.ReadMatrix(hmm, k.A, k.read_off, k.pool)
        rm.scatter(dev)
        pb = capi.PostBatch(log_aln_probs=None, **k.kw)
        pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error().decode()
        assert hmm.hipstr_post_launch(pd, None) == 0
        asg = capi.run_assign(hmm, pd, k.seeds, pool_index=k.pool, pool_off=k.pool_off, rule=capi.ASSIGN_RETRACE, n_reads=k.n, n_samp=4)
        assert asg["rc"] == 0 and asg["n_req"] > 0
        h2r = capi.hap_aln_info(hmm, "hipstr_", k.b.ptr)
        td = capi.run_trace_resident(hmm, k.b.ptr, asg["req_read"], asg["req_allele"], h2r)
        got = capi.run_census(hmm, pd, k.b.ptr, k.seeds, asg["read_req"], asg["req_read"], None, hap_to_allele=k.h2a, n_samp=4, min_frac=0.01, td=td)
        extra = None
        if stats:
            st = capi.assign_trace_stats_dev(hmm, pb, asg["read_req"], td, asg["best_hap"], *chain_stats_tables(k))
            fl = capi.trace_dev_fetch(hmm, td, capi.TRACE_F_FLANKS)
            m = 2 * asg["n_req"] + 1
            extra = dict(n_stutter=st[0], n_flank_indel=st[1], ml_bp=st[2], flank_off=fl["flank_seq_off"][:m], flank=fl["flank_seq"].raw[:int(fl["flank_seq_off"][m - 1])])
    finally:
        if td:
            td.close()
        if pd:
            hmm.hipstr_post_free(pd)
        if rm:
            rm.close()
        hmm.hipstr_hmm_free(dev)
    return got, asg, extra


def chain_stats_tables(k):
    """hap_to_allele (every haplotype its own variant), allele_bp_diff, n_variants, region_start, region_stop of the chain's two loci."""
    A = [int(x) for x in k.A]
    return (np.concatenate([np.arange(a) for a in A]), np.concatenate([3 * np.arange(a) - 3 for a in A]), A,
            [L.blocks[1][0] for L in k.loci], [L.blocks[1][1] for L in k.loci])


def test_census_chained_on_the_resident_matrix(hmm, oracle):
    k = tc.chain_inputs(hmm, oracle)
    want, asg_w, tr = tc.run_chain(hmm, k)
    got, asg, _ = run_chain_resident(hmm, k)
    assert np.array_equal(asg["req_read"], asg_w["req_read"]) and np.array_equal(asg["read_req"], asg_w["read_req"])
    tp.same_bits({x: (got[x] if x == "cand" else np.asarray(got[x])) for x in tc.KEYS + ("cand",)},
                 {x: (want[x] if x == "cand" else np.asarray(want[x])) for x in tc.KEYS + ("cand",)}, "resident chain against run_chain")
    tc.compare(got, tc.chain_want(k, asg_w, tr), "chained, resident")
    assert got["n_spanning"].sum() > 0 and got["spanned"].sum() > 0


# ------------------------------------------------------------------ 6. read counts
def _stats_pb(n_alleles, n_samples, read_off, sample_label):
    n = len(sample_label)
    return capi.PostBatch(n_alleles, n_samples, read_off, sample_label, np.zeros(n), np.zeros(n), np.ones(n, np.int32), None)


def stats_inputs():
    """Three loci with region_start 0, 4 and 5 and 2, 3 and 1 variants; samples of 0, 1, 64 and 65 reads (and of 130: three turns of the
    wavefront's loop); reads without a request; requests that span by the rule of :1152-1154 with and without STR data."""
    rng = np.random.default_rng(17)
    sizes = [[0, 1, 64, 65], [65, 0, 64], [130, 1]]
    A, V, starts = [3, 5, 2], [2, 3, 1], [0, 4, 5]
    stops = [s + 20 for s in starts]
    nq = 40
    lab, off = [], [0]
    for s in sizes:
        for i, m in enumerate(s):
            lab += [i] * m
        off.append(len(lab))
    n = len(lab)
    locus_of = np.repeat(np.arange(3), np.diff(off))
    # requests: starts around every bound (-1 lies below a bound of 0: the only start that does), stops around region_stop + 4
    tr = dict(ll=np.zeros(nq), max_index=np.zeros(nq, np.int32),
              stutter_size=rng.choice([NO_STR, NO_STR, 0, 0, -4, 2, 6], nq), flank_ins=rng.choice([0, 0, 0, 1, 3], nq), flank_del=rng.choice([0, 0, 2], nq),
              aln_start=rng.choice([-1, 0, 1, 2], nq), aln_stop=rng.choice([23, 24, 25, 28, 29, 30, 40], nq))
    tr["stutter_size"][:2] = [NO_STR, -4]; tr["aln_start"][:2] = -1; tr["aln_stop"][:2] = 40          # span at every locus, without and with STR data
    read_req = rng.integers(-1, nq, n).astype(np.int32)
    read_req[[off[0], off[1], off[2]]] = [0, 0, 1]
    best = np.array([-1 if read_req[r] < 0 else int(rng.integers(A[locus_of[r]])) for r in range(n)], np.int32)
    h2a = np.concatenate([rng.integers(0, v, a) for a, v in zip(A, V)]).astype(np.int32)
    bp = rng.integers(-12, 13, sum(V)).astype(np.int32)
    return _stats_pb(A, [len(s) for s in sizes], off, lab), read_req, tr, best, h2a, bp, V, starts, stops, nq


def test_read_counts_equal_the_host_loop(hmm):
    pb, read_req, tr, best, h2a, bp, V, starts, stops, nq = stats_inputs()
    td = capi.trace_dev_from_host(hmm, tr, nq)
    try:
        fetched = capi.trace_dev_fetch(hmm, td, capi.TRACE_F_SCALARS, null_others=True)
        for nm in ("stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop"):
            assert np.array_equal(fetched[nm][:nq], np.asarray(tr[nm], np.int32)), nm
        want = capi.run_assign_trace_stats(hmm, pb, read_req, fetched, best, h2a, bp, V, starts, stops)
        got = capi.assign_trace_stats_dev(hmm, pb, read_req, td, best, h2a, bp, V, starts, stops)
        for g, w, nm in zip(got, want, ("n_stutter", "n_flank_indel", "ml_bp")):
            assert np.array_equal(g, w), nm
        ml = want[2]
        assert want[0].sum() > 0 and want[1].sum() > 0 and (ml != capi.NO_ML_BP).sum() >= 3 and (ml == capi.NO_ML_BP).sum() > 0
        assert want[0][0] == 0 and want[1][0] == 0                                       # the sample without reads
        r0 = int(pb.a["read_off"][0])
        assert ml[r0] == bp[h2a[best[r0]]] + 0                                           # spans without STR data: no stutter added
        # an empty batch
        none = capi.PostBatch([], [], [0], [], [], [], [], None)
        e = capi.assign_trace_stats_dev(hmm, none, [], td, [], [], [], [], [], [])
        assert all(len(x) == 0 for x in e)
        # every host refusal of the original, and a request beyond the handle's
        good = dict(read_req=read_req, best_hap=best, hap_to_allele=h2a, allele_bp_diff=bp, n_variants=V, region_start=starts, region_stop=stops)
        def run(pb=pb, td=td, **kw):
            a = dict(good); a.update(kw)
            return capi.assign_trace_stats_dev(hmm, pb, a["read_req"], td, a["best_hap"], a["hap_to_allele"], a["allele_bp_diff"], a["n_variants"],
                                               a["region_start"], a["region_stop"])
        r = int(np.nonzero(read_req >= 0)[0][0])
        bad_best = best.copy(); bad_best[r] = 7
        neg_best = best.copy(); neg_best[r] = -1
        bad_h2a = h2a.copy(); bad_h2a[0] = V[0]
        bad_lab = pb.a["sample_label"].copy(); bad_lab[0] = 4
        beyond = read_req.copy(); beyond[r] = nq
        for kw, word in ((dict(best_hap=bad_best), "best_hap"), (dict(best_hap=neg_best), "best_hap"), (dict(hap_to_allele=bad_h2a), "hap_to_allele"),
                         (dict(n_variants=[0, 3, 1]), "inconsistent"), (dict(pb=_stats_pb(pb.a["n_alleles"], pb.a["n_samples"], pb.a["read_off"], bad_lab)), "sample_label"),
                         (dict(read_req=beyond), "read_req outside the trace handle")):
            with pytest.raises(RuntimeError, match=word):
                run(**kw)
        short = capi.trace_dev_from_host(hmm, dict(tr, aln_stop=None), nq)
        try:
            with pytest.raises(RuntimeError, match="aln_stop"):
                run(td=short)
        finally:
            short.close()
        again = run()
        assert all(np.array_equal(g, w) for g, w in zip(again, want))
    finally:
        td.close()


# ------------------------------------------------------------------ 7. handles
def test_handles(hmm, oracle):
    c = tc.content_case()
    want = tc.restate(c, ta.oracle_map(oracle, c.pb))
    nq = len(c.req_read); ns = int(c.pb.samp_off[-1])
    args = (c.batch.ptr, c.seed, c.read_req, c.req_read, None)
    td = case_handle(hmm, c)
    other = capi.trace_dev_from_host(hmm, dict(c.trace, str_seq_off=c.trace["str_seq_off"][:nq]), nq - 1)
    pd = hmm.hipstr_post_upload(c.pb.ptr, None); assert pd
    try:
        with pytest.raises(RuntimeError, match="hipstr_post_launch"):                   # a run that was not launched
            capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=td)
        assert hmm.hipstr_post_launch(pd, None) == 0
        with pytest.raises(RuntimeError, match="n_req differs"):
            capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=other)
        with pytest.raises(RuntimeError, match="rq->trace must be NULL"):
            capi.run_census(hmm, pd, c.batch.ptr, c.seed, c.read_req, c.req_read, c.trace, hap_to_allele=c.h2a, n_samp=ns, td=td)
        with pytest.raises(RuntimeError, match="does not hold"):                         # a group the handle lacks
            capi.trace_dev_fetch(hmm, td, capi.TRACE_F_FLANKS)
        # two handles alive at once, freed in either order
        for first in (0, 1):
            pair = [case_handle(hmm, c), case_handle(hmm, c)]
            tc.compare(capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=pair[1 - first]), want, "two handles")
            pair[first].close()
            tc.compare(capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=pair[1 - first]), want, "one freed")
            pair[1 - first].close()
            tc.compare(capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=td), want, "both freed")
        # the same handle, several consumer calls
        tc.compare(capi.run_census(hmm, pd, *args, hap_to_allele=c.h2a, n_samp=ns, td=td), want, "again")
    finally:
        hmm.hipstr_post_free(pd); td.close(); other.close()
    # a failing hipstr_hmm_trace_resident leaves no handle (run_trace_resident asserts *td == NULL) and the device usable
    sb, rr, aa, h2r = tta._small(oracle, seed=12, reads=12, alleles=4)
    with pytest.raises(RuntimeError, match="allele outside"):
        capi.run_trace_resident(hmm, sb.ptr, [0], [99], None)
    with pytest.raises(RuntimeError, match="read outside"):
        capi.run_trace_resident(hmm, sb.ptr, [99], [0], None)
    with pytest.raises(RuntimeError, match="unknown flag"):
        capi.run_trace_resident(hmm, sb.ptr, rr, aa, h2r, flags=1)
    equals_host_replay(hmm, sb.ptr, rr, aa, h2r, what="after the refused calls")


# ------------------------------------------------------------------ 8. poisoned cache blocks
def test_poisoned_cache_blocks_and_no_driver_allocation(hmm, oracle):
    """trace_resident -> census_dev -> stats_dev -> fetch(FLANKS) -> free after hipstr_debug_cache_poison with 0xFF, 0x7F, 0x80 and 0x00: the
    four results identical bit for bit and equal to the unpoisoned run, no block fresh from the driver (tests/test_poison_gpu.py's protocol)."""
    k = tc.chain_inputs(hmm, oracle)
    def strip(g):
        return {x: (g[x] if x == "cand" else np.asarray(g[x])) for x in tc.KEYS + ("cand",)}
    def chain():
        got, asg, extra = run_chain_resident(hmm, k, stats=True)
        return dict(strip(got), read_req=asg["read_req"], req_read=asg["req_read"], **extra)
    out = tp.poisoned(hmm, chain, "resident chain")
    tp.same_bits(chain(), out[0], "resident chain, unpoisoned against poisoned")
    # ... and what it computed is what the host path computes
    want, asg, tr = tc.run_chain(hmm, k)
    tp.same_bits(strip(want), {x: out[0][x] for x in tc.KEYS + ("cand",)}, "resident chain against run_chain")
    pb = capi.PostBatch(log_aln_probs=None, **k.kw)
    st = capi.run_assign_trace_stats(hmm, pb, asg["read_req"], tr, asg["best_hap"], *chain_stats_tables(k))
    for g, w, nm in zip((out[0]["n_stutter"], out[0]["n_flank_indel"], out[0]["ml_bp"]), st, ("n_stutter", "n_flank_indel", "ml_bp")):
        assert np.array_equal(g, w), nm
    m = 2 * asg["n_req"] + 1
    assert np.array_equal(out[0]["flank_off"], tr["flank_seq_off"][:m]) and out[0]["flank"] == tr["flank_seq"].raw[:int(tr["flank_seq_off"][m - 1])]
