"""CPU: the haplotype generator's host side (include/hipstr_hmm.h: hipstr_hapgen_host, hipstr_hapgen_batch(HIPSTR_HAPGEN_ON_HOST); the plan
of hipstr_hapgen, hipstr_debug_hapgen_plan) — the host twin (hipstr_amd/csrc/hapgen_host.cpp) against the blocks and the status the
REFERENCE's own HaplotypeGenerator gave for the five golden batches (tests/golden/hapgen_*.npz), byte for byte; against the python
restatement (tests/hapgen_cases.py), which must itself reproduce those records, for the reads' extracted runs, the distinct strings with
their counts and double sums (as bits) and the per-locus counts; every refusal; the documented locus without flagged reads; the plan on
either side of every cap; header, exports and ctypes structs; and the stand-alone sanitizer build of the host twin
(tests/cpp/hapgen_host_test.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import hapgen_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = sorted(hc.BATCHES)


@pytest.fixture(scope="module")
def golden():
    """name -> (loci, the reference's records, reads batch, request, restatement): built once, shared, never changed."""
    out = {}
    for name in BATCHES:
        loci, recs = hc.load_golden(name)
        out[name] = (loci, recs, hc.ReadsBatch(loci), hc.request_of(loci), hc.expectation(loci))
    return out


@pytest.mark.parametrize("name", BATCHES)
def test_golden_files_hold_the_batches_of_the_case_file(golden, name):
    loci, recs = golden[name][:2]
    assert hc.case_text(loci) == hc.case_text(hc.BATCHES[name]()) and list(recs) == [lc["name"] for lc in loci]


@pytest.mark.parametrize("name", BATCHES)
def test_restatement_reproduces_the_reference(golden, name):
    loci, recs = golden[name][:2]
    for lc in loci:
        e, r = hc.restate(lc), recs[lc["name"]]
        assert (e["status"], e["blocks"]) == (r["status"], r["blocks"]), lc["name"]
        assert r["message"] == capi.HAPGEN_STATUS[r["status"]]


@pytest.mark.parametrize("name", BATCHES)
def test_host_twin_equals_the_reference(hmm_host, golden, name):
    loci, recs, b, rq, _ = golden[name]
    got = capi.run_hapgen(hmm_host, b.ptr, rq, host=True)
    for l, lc in enumerate(loci):
        r = recs[lc["name"]]
        assert int(got["status"][l]) == r["status"], lc["name"]
        assert hmm_host.hipstr_hapgen_status_message(r["status"]).decode() == r["message"]
        assert hc.blocks_of(got, l) == (r["blocks"] or [(0, 0, [])] * 3), lc["name"]


@pytest.mark.parametrize("name", BATCHES)
def test_host_twin_equals_the_restatement(hmm_host, golden, name):
    loci, _, b, rq, want = golden[name]
    hc.assert_result(capi.run_hapgen(hmm_host, b.ptr, rq, host=True), want, name)
    # every optional output on its own, and none of them
    for skip in [(k,) for k in capi.HAPGEN_OPTIONAL] + [capi.HAPGEN_OPTIONAL]:
        hc.assert_result(capi.run_hapgen(hmm_host, b.ptr, rq, host=True, skip=skip), want, "%s without %s" % (name, skip))


def test_the_cases_bite(golden):
    """What the batches are there for, read off the reference's records and the restatement."""
    loci, recs = golden["unit_extract"][:2]
    nopt = {lc["name"]: len(recs[lc["name"]]["blocks"][1][2]) for lc in loci}
    for rejected, accepted in (("start_at_edge_rejected", "start_one_before_edge"), ("stop_at_edge_rejected_exclusive", "stop_one_beyond_exclusive"),
                               ("stop_at_edge_rejected_inclusive", "stop_one_beyond_inclusive"), ("insertion_before_the_region", "insertion_where_the_region_begins"),
                               ("insertion_after_the_region", "insertion_at_the_last_position"), ("unflagged_read_is_not_counted", "x_runs")):
        assert (nopt[rejected], nopt[accepted]) == (1, 2), (rejected, accepted)
    assert "" in recs["deletion_of_the_whole_padded_region"]["blocks"][1][2]
    assert nopt["lower_case_and_n"] == 3 and all(o == o.upper() for o in recs["lower_case_and_n"]["blocks"][1][2])
    lc = [x for x in loci if x["name"] == "unflagged_read_bounds_the_flanks"][0]
    blk = recs[lc["name"]]["blocks"]
    assert blk[0][0] == blk[1][0] - 35 < min(r["start"] for r in lc["reads"] if r["use"]) and blk[2][1] == blk[1][1] + 35
    loci, recs, _, _, want = golden["unit_thresholds"]
    by = {lc["name"]: hc.restate(lc) for lc in loci}
    strong = lambda n: by[n]["dist"][1][3]
    assert (strong("strong_2_of_10"), strong("not_strong_2_of_11"), strong("not_strong_1_of_1")) == (1, 0, 0)
    sel = {lc["name"]: len(recs[lc["name"]]["blocks"][1][2]) for lc in loci}
    for out, inn in (("not_strong_2_of_11", "strong_2_of_10"), ("reads_exactly_5_percent", "reads_one_more"), ("fraction_exactly_5_percent", "fraction_one_more")):
        assert (sel[out], sel[inn]) == (1, 2), (out, inn)
    e = by["reads_exactly_5_percent"]
    assert e["dist"][1][2] == 0.05 * e["n_spanning"] and e["dist"][1][4] == 0.05 * e["n_samples_spanning"]
    e = by["fraction_exactly_5_percent"]
    assert e["dist"][1][4] == 0.05 * e["n_samples_spanning"] and e["dist"][1][2] < 0.05 * e["n_spanning"]
    assert by["sample_without_spanning_reads"]["n_samples_spanning"] == 2 and by["sample_index_without_any_read"]["n_samples_spanning"] == 2
    fr = {n: hc.f64_bits(by[n]["dist"][1][4]) for n in by if n.startswith("four_denominators")}
    assert fr["four_denominators"] == fr["four_denominators_reads_reversed"] and len(set(fr.values())) == 2      # the order of the samples, not of the reads
    ref_of = lambda n: recs[n]["blocks"][1][2][0]
    assert by["reference_absent"]["n_distinct"] == 2 and sel["reference_absent"] == 3 and sel["reference_weak_only"] == 3 and ref_of("reference_weak_only")
    loci, recs = golden["unit_trim"][:2]
    trims = {lc["name"]: (hc.restate(lc)["left_trim"], hc.restate(lc)["right_trim"]) for lc in loci}
    assert trims["no_trim_short_reference"] == trims["no_trim_short_alternative"] == (0, 0)
    assert trims["prefix_2_suffix_5"] == (2, 5) and trims["prefix_5_suffix_1"] == (5, 1) and trims["prefix_0_suffix_0"] == (0, 0)
    assert trims["balancing_steps_on_both_sides"] == (3, 3) and trims["balancing_one_step"] == (5, 4) and trims["balancing_exact"] == (5, 5)
    assert trims["left_arm"] == (5, 2) and trims["left_arm_capped"] == (4, 2) and trims["right_arm"] == (1, 5) and trims["right_arm_capped"] == (1, 4)
    assert {lc["period"] for lc in loci} >= {1, 6}
    loci, recs = golden["unit_status"][:2]
    assert [recs[lc["name"]]["status"] for lc in loci] == [1, 0, 0, 1, 2, 0, 2, 0]
    loci = golden["random"][0]
    sizes = [len(lc["reads"]) for lc in loci]
    assert len(loci) == 40 and {63, 64, 65, 5, 130} <= set(sizes) and {lc["period"] for lc in loci} == set(range(1, 7)) and {lc["n_samples"] for lc in loci} == set(range(1, 7))
    assert max(len(golden["random"][1][lc["name"]]["blocks"][1][2]) for lc in loci) >= 5


def test_read_stop_null_is_start_plus_the_reference_runs(hmm_host, golden):
    for name in ("unit_trim", "random"):            # every read of these states the exclusive end
        loci, _, b, _, want = golden[name]
        hc.assert_result(capi.run_hapgen(hmm_host, b.ptr, hc.request_of(loci, give_stop=False), host=True), want, name)


def test_every_locus_alone_and_reads_in_front_of_the_first_locus(hmm_host, golden):
    loci = golden["unit_extract"][0] + golden["unit_status"][0]
    for lc in loci:
        hc.assert_result(capi.run_hapgen(hmm_host, hc.ReadsBatch([lc]).ptr, hc.request_of([lc]), host=True), hc.expectation([lc]), lc["name"])
    b = hc.ReadsBatch(loci, lead_reads=3); rq = hc.request_of(loci, lead_reads=3)
    hc.assert_result(capi.run_hapgen(hmm_host, b.ptr, rq, host=True), hc.expectation(loci, base_read=3), "three reads in front")
    raw = capi.run_hapgen(hmm_host, b.ptr, rq, host=True, raw=True)
    assert np.all(raw["ext_off"][:3] == capi.HAPGEN_FILL) and np.all(raw["ext_len"][:3] == capi.HAPGEN_FILL)
    # no loci at all
    e = capi.run_hapgen(hmm_host, hc.ReadsBatch([]).ptr, hc.request_of([]), host=True)
    assert e["opt_off"].tolist() == [0] and e["options"] == [] and e["untouched"]


def test_a_locus_without_flagged_reads_has_status_2(hmm_host):
    """The documented deviation: the reference computes INT_MAX + 5 there (undefined behaviour); the library does it in 64 bits."""
    loci = hc.no_flagged_loci()
    got = capi.run_hapgen(hmm_host, hc.ReadsBatch(loci).ptr, hc.request_of(loci), host=True)
    assert got["status"].tolist() == [2, 2] and got["blk_nopts"].tolist() == [0] * 6 and got["options"] == []
    assert got["min_aln_start"].tolist() == [hc.INT_MAX, 60] and got["max_aln_stop"].tolist() == [hc.INT_MIN, 161]
    assert np.all(got["ext_len"] == -1)
    hc.assert_result(got, hc.expectation(loci), "no flagged reads")
    txt = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read()
    assert "Deviation from the reference: a locus without a flagged read" in txt


# ------------------------------------------------------------------------------------------------------------------ the batch
def test_hapgen_batch_on_the_host(hmm_host, golden):
    loci = golden["unit_status"][0] + golden["unit_extract"][0][:4] + hc.no_flagged_loci()
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    want = [hc.restate(lc) for lc in loci]
    hb = capi.HapgenBatch(hmm_host, b.ptr, rq, capi.HAPGEN_ON_HOST)
    keep = [l for l, e in enumerate(want) if e["status"] == 0]
    assert hb.status.tolist() == [e["status"] for e in want] and hb.locus.tolist() == keep and 0 < len(keep) < len(loci)
    ref = capi.Batch()
    for l in keep:
        reads = [dict(seq=r["seq"], qual="F" * len(r["seq"]), start=r["start"], cigar=r["cigar"]) for r in loci[l]["reads"]]
        ref.add_locus(want[l]["blocks"], loci[l]["period"], hc.STUTTER, reads)
    ref.finalize()
    got = hb.arrays()
    for k in ("blk_start", "blk_end", "blk_nopts", "period", "stutter", "opt_off", "hap_off", "read_off", "base_off", "read_start", "cigar_off", "cigar_len"):
        assert np.array_equal(got[k], ref.arrays[k]), k
    for k in ("seq", "bases", "quals", "cigar_op"):
        assert bytes(got[k]) == ref.arrays[k][:-1], k
    assert got["realign_hap"].size == 0 and got["realign_read"].size == 0
    hb.close()
    # a batch of failures only, and none at all
    fails = hc.no_flagged_loci()
    hb = capi.HapgenBatch(hmm_host, hc.ReadsBatch(fails).ptr, hc.request_of(fails), capi.HAPGEN_ON_HOST)
    assert hb.ptr.contents.n_loci == 0 and hb.status.tolist() == [2, 2]
    hb.close()


# ------------------------------------------------------------------------------------------------------------------ the plan
def layout_constants():
    txt = open(os.path.join(ROOT, "hipstr_amd", "csrc", "hapgen_layout.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (HS_HAPGEN_[A-Z_]+) (\d+)\b", txt, flags=re.M)}


def test_plan_thresholds_are_the_headers(hmm_host):
    h = layout_constants()
    p = capi.hapgen_plan(hmm_host, hc.ReadsBatch([]).ptr, hc.request_of([]))
    t = p["thresholds"]
    assert t == {k: h[k] for k in t} and len(t) == 10
    assert p["routes"] == list(capi.HAPGEN_ROUTES) and p["chunks"] == [] and p["routes_hit"] == []
    assert p["budget_bytes"] == t["HS_HAPGEN_WS_MIB"] << 20
    assert 64 * 1024 < p["max_lds_bytes"] <= 160 * 1024               # the grouping workgroup at its caps fits a CU's LDS


def test_plan_routes_on_either_side_of_every_cap(hmm_host):
    rng = np.random.default_rng(2)
    t = capi.hapgen_plan(hmm_host, hc.ReadsBatch([]).ptr, hc.request_of([]))["thresholds"]
    cap, scap = t["HS_HAPGEN_LDS_READS"], t["HS_HAPGEN_MAX_SAMPLES"]
    hit = set()
    for n, dev in ((cap - 1, 1), (cap, 1), (cap + 1, 0)):
        lc = hc.cap_locus(rng, n)
        p = capi.hapgen_plan(hmm_host, hc.ReadsBatch([lc]).ptr, hc.request_of([lc]))
        c = p["chunks"][0]
        assert (c["device_loci"], c["host_loci"], c["reads"]) == (dev, 1 - dev, n * dev), n
        assert p["routes_hit"] == (["device"] if dev else ["host"])
        assert not dev or c["lds_bytes"] <= p["max_lds_bytes"]
        hit |= set(p["routes_hit"])
    for s, dev in ((scap - 1, 1), (scap, 1), (scap + 1, 0)):
        lc = hc.cap_locus(rng, 40, n_samples=s)
        c = capi.hapgen_plan(hmm_host, hc.ReadsBatch([lc]).ptr, hc.request_of([lc]))["chunks"][0]
        assert (c["device_loci"], c["host_loci"]) == (dev, 1 - dev), s
    assert hit == set(capi.HAPGEN_ROUTES)
    # the host twin does not care
    lc = hc.cap_locus(rng, cap + 1)
    hc.assert_result(capi.run_hapgen(hmm_host, hc.ReadsBatch([lc]).ptr, hc.request_of([lc]), host=True), hc.expectation([lc]), "cap + 1")


def test_plan_chunks_are_whole_loci_under_the_budget(hmm_host, golden):
    loci, _, b, rq, _ = golden["random"]
    one = capi.hapgen_plan(hmm_host, b.ptr, rq)
    assert len(one["chunks"]) == 1 and one["chunks"][0]["l1"] == 40
    p = capi.hapgen_plan(hmm_host, b.ptr, rq, ws_mib=0.125)
    ch = p["chunks"]
    assert len(ch) >= 3 and ch[0]["l0"] == 0 and ch[-1]["l1"] == 40 and all(a["l1"] == c["l0"] for a, c in zip(ch, ch[1:]))
    assert all(c["bytes"] <= p["budget_bytes"] or c["l1"] - c["l0"] == 1 for c in ch)
    assert sum(c["reads"] for c in ch) == one["chunks"][0]["reads"] and sum(c["bytes"] for c in ch) == one["chunks"][0]["bytes"]


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_symbols_structs_and_headers_agree(hmm_host):
    pub = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read(); dbg = open(os.path.join(ROOT, "include", "hipstr_hmm_debug.h")).read()
    for n in ("hipstr_hapgen", "hipstr_hapgen_host", "hipstr_hapgen_status_message", "hipstr_hapgen_batch", "hipstr_hapgen_batch_batch", "hipstr_hapgen_batch_locus",
              "hipstr_hapgen_batch_status", "hipstr_hapgen_batch_free"):
        assert hasattr(hmm_host, n) and re.search(r"\b%s\(" % n, pub), n
    for n in ("hipstr_debug_hapgen_plan", "hipstr_debug_hapgen_last", "hipstr_debug_hapgen_last_timing"):
        assert hasattr(hmm_host, n) and re.search(r"\b%s\(" % n, dbg) and n not in pub, n
    assert re.search(r"#define HIPSTR_HAPGEN_ON_HOST (\d+)u", pub).group(1) == str(capi.HAPGEN_ON_HOST)
    for struct, cls in (("hipstr_hapgen_out", capi.HipstrHapgenOut), ("hipstr_hapgen_request", capi.HipstrHapgenRequest)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), pub, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
        assert names == [f for f, _ in cls._fields_], struct
    assert [hmm_host.hipstr_hapgen_status_message(i) for i in (0, 1, 2)] == [m.encode() for m in capi.HAPGEN_STATUS] and hmm_host.hipstr_hapgen_status_message(3) is None
    from hipstr_amd import build
    assert {"hapgen.hip", "hapgen_host.cpp"} <= set(build.HIP_SOURCES) and {"hapgen_layout.h", "hapgen_host.h"} <= set(build.HIP_HEADERS)


def test_refusals(hmm_host):
    rng = np.random.default_rng(3)
    good = [hc.cap_locus(rng, 6, n_samples=2)]
    def attempt(fn, loci=good, mutate=None, **kw):
        """One call on a copy of the case with `mutate` applied to (reads batch, request): the message, after checking nothing was written."""
        b = hc.ReadsBatch(loci); rq = hc.request_of(loci, **kw)
        a = capi.hapgen_arrays(b.ptr, rq)
        if mutate:
            mutate(b, rq)
        rc = fn(b.ptr, rq.ptr, C.byref(capi.hapgen_out_struct(a)))
        assert rc != 0
        assert all(np.all(v == (0x5A if k == "seq" else capi.HAPGEN_FILL)) for k, v in a.items()), "written"
        return hmm_host.hipstr_last_error().decode()
    def set_(what, k, i, v):
        def f(b, rq):
            (b.a if what == "b" else rq.a)[k][i] = v
        return f
    def cigar_op(b, rq):
        b.a["cigar_op"] = b.a["cigar_op"].replace(b"=", b"S", 1); b.struct.cigar_op = b.a["cigar_op"]
    def short_window(b, rq):
        rq.a["win_off"][1] -= 1
    def null_field(name, what="rq"):
        def f(b, rq):
            setattr(rq.struct if what == "rq" else b.struct, name, None)
        return f
    for fn in (hmm_host.hipstr_hapgen_host, hmm_host.hipstr_hapgen):
        b = hc.ReadsBatch(good); rq = hc.request_of(good)
        o = capi.hapgen_out_struct(capi.hapgen_arrays(b.ptr, rq))
        for args in ((None, None, None), (b.ptr, rq.ptr, None), (None, rq.ptr, C.byref(o)), (b.ptr, None, C.byref(o))):
            assert fn(*args) != 0 and b"null argument" in hmm_host.hipstr_last_error()
        for k in capi.HAPGEN_FIELDS:
            if k not in capi.HAPGEN_OPTIONAL:
                a = capi.hapgen_arrays(b.ptr, rq)
                assert fn(b.ptr, rq.ptr, C.byref(capi.hapgen_out_struct(a, skip=(k,)))) != 0 and b"null output array" in hmm_host.hipstr_last_error(), k
        for k in ("region_start", "region_stop", "period", "chrom_len", "win_off", "window", "n_samples", "sample_label"):
            assert "null array in the request" in attempt(fn, mutate=null_field(k)), k
        for k in ("read_off", "base_off", "bases", "read_start", "cigar_off", "cigar_op", "cigar_len"):
            assert "null table in a batch with loci" in attempt(fn, mutate=null_field(k, "b")), k
        assert "base_off must not decrease" in attempt(fn, mutate=set_("b", "base_off", 1, 700))
        assert "cigar_off must not decrease" in attempt(fn, mutate=set_("b", "cigar_off", 1, 70))
        assert "read_off must not decrease" in attempt(fn, loci=good + [hc.cap_locus(rng, 0)], mutate=set_("b", "read_off", 2, 0))
        assert "negative offset" in attempt(fn, mutate=set_("b", "read_off", 0, -1))
        assert "CIGAR run of non-positive length" in attempt(fn, mutate=set_("b", "cigar_len", 0, 0))
        assert "win_off must not decrease" in attempt(fn, loci=good + good, mutate=set_("rq", "win_off", 1, 500))
        assert "CIGAR op other than = X I D" in attempt(fn, mutate=cigar_op)
        assert "sample_label outside [0, n_samples)" in attempt(fn, mutate=set_("rq", "sample_label", 2, 2))
        assert "sample_label outside [0, n_samples)" in attempt(fn, mutate=set_("rq", "sample_label", 2, -1))
        assert "window shorter than" in attempt(fn, mutate=short_window)
        assert "read_stop beyond start" in attempt(fn, mutate=lambda b, rq: rq.a["read_stop"].__setitem__(1, int(rq.a["read_stop"][1]) + 1))
        assert "CIGAR covers more bases than the read has" in attempt(fn, mutate=lambda b, rq: b.a["cigar_len"].__setitem__(0, int(b.a["cigar_len"][0]) + 40))
        assert "period below 1" in attempt(fn, mutate=set_("rq", "period", 0, 0))
        assert "region_stop before region_start" in attempt(fn, mutate=set_("rq", "region_stop", 0, 10))
        assert "negative n_samples" in attempt(fn, mutate=set_("rq", "n_samples", 0, -1))
        # a window is not asked of a locus that fails the chromosome-end check; a read_stop under the CIGAR's end is the caller's convention
        b = hc.ReadsBatch(good); rq = hc.request_of(good)
        rq.a["read_stop"][:] -= 1
        assert capi.run_hapgen(hmm_host, b.ptr, rq, host=True)["status"].tolist() == [0]
    b = hc.ReadsBatch(good); rq = hc.request_of(good)
    assert hmm_host.hipstr_hapgen_batch(None, rq.ptr, 0) is None and b"null argument" in hmm_host.hipstr_last_error()
    assert hmm_host.hipstr_hapgen_batch(b.ptr, rq.ptr, 6) is None and b"unknown flag" in hmm_host.hipstr_last_error()
    rq2 = hc.request_of(good, stutter=False)
    assert hmm_host.hipstr_hapgen_batch(b.ptr, rq2.ptr, capi.HAPGEN_ON_HOST) is None and b"null array in the request" in hmm_host.hipstr_last_error()
    assert hmm_host.hipstr_debug_hapgen_plan(None, None, 0.0, None, 0) == -1
    assert not hmm_host.hipstr_hapgen_batch_batch(None) and not hmm_host.hipstr_hapgen_batch_locus(None) and not hmm_host.hipstr_hapgen_batch_status(None)
    hmm_host.hipstr_hapgen_batch_free(None)


def test_no_host_fallback_without_a_device(hmm_host):
    """tests/test_prep.py::test_no_cpu_fallback_without_device's rule for this stage: the device entry point fails, it does not quietly work on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    loci = hc.unit_trim()[:3]
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.run_hapgen(hmm_host, b.ptr, rq)
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.HapgenBatch(hmm_host, b.ptr, rq, 0)
    capi.run_hapgen(hmm_host, b.ptr, rq, host=True)


# ------------------------------------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_host_twin_under_sanitizers(tmp_path):
    """hapgen_host.cpp next to a program with a main of its own, both built with AddressSanitizer and UBSan, the runtimes linked statically:
    nothing is preloaded and nothing of it is loaded into python."""
    exe = str(tmp_path / "hapgen_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "hapgen_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "hapgen_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ok, loci, reads, built, options = r.stdout.decode().split()
    assert ok == "ok" and int(loci) == 80 and int(reads) > 3000 and int(built) > 40 and int(options) > 3 * int(built)
