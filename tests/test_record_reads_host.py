"""CPU: the host forms of the record's per-read sizes and per-sample histograms — hipstr_cigar_bp_diffs_host, hipstr_sample_histograms_host
and hipstr_em_batch_from_bp_diffs (include/hipstr_hmm.h; hipstr_amd/csrc/record_reads_host.cpp).  ExtractCigar and condense_read_counts
against what the compiled reference returned on the same cases (tests/golden/record_reads_*.npz, written by
tests/golden/make_golden_record_reads.py), byte for byte; the EM's read loop against its Python restatement (tests/record_reads_cases.py,
with the reference's line numbers); the refusals; the names in the header, the export map and capi.py; and the stand-alone program
tests/cpp/record_reads_host_test.cpp built with -fsanitize=address,undefined (run as a program: nothing is preloaded)."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import record_reads_cases as rc

ROOT = rc.ROOT


@pytest.fixture(scope="module")
def lib(hmm_host):
    return hmm_host


# ------------------------------------------------------------------------------------------------------------------ CIGARs
def test_cigar_cases_hold_what_they_name():
    loci = rc.cigar_loci()
    got, bp = rc.cigar_golden()
    reads = [(l, r) for l in loci for r in l[3]]
    assert len(got) == len(bp) == len(reads) and got.dtype == np.uint8 and bp.dtype == np.int32
    assert os.path.getsize(rc.GOLDEN_CIGARS) < 64 * 1024 and os.path.getsize(rc.GOLDEN_HISTOGRAMS) < 64 * 1024
    runs = [len(r[1]) for _, r in reads]
    assert 1 in runs and max(runs) > rc.CIGAR_DEVICE_RUNS and rc.CIGAR_DEVICE_RUNS in runs and rc.CIGAR_DEVICE_RUNS + 1 in runs
    assert {o for _, r in reads for o, _ in r[1]} == set(rc.OPS)
    assert 0 < got.sum() < len(got) and np.any(bp > 0) and np.any(bp < 0) and np.all(bp[got == 0] == 0)
    # the named reads, by the reference's own verdict: the two boundary tests from either side by one base
    g = iter(got.tolist())
    first = [next(g) for _ in range(3)]; second = [next(g) for _ in range(4)]
    assert first == [1, 0, 1] and second == [1, 0, 0, 1]
    [next(g) for _ in range(2)]
    assert [next(g) for _ in range(4)] == [0, 0, 1, 1]              # a leading I / S with the region at the read's start; a trailing I; one base earlier
    assert [next(g) for _ in range(5)] == [0, 0, 1, 1, 1]           # a trailing I / S behind the deletion that holds the region's end
    assert [next(g) for _ in range(5)] == [1, 0, 0, 1, 1]           # last_match_index stays 0 without a match before the region: run 0 decides


def test_cigars_equal_the_reference(lib):
    rq = capi.cigar_request(rc.cigar_loci())
    got, bp = capi.run_cigar_bp_diffs(lib, rq, host=True)
    want_got, want_bp = rc.cigar_golden()
    assert np.array_equal(got, want_got) and np.array_equal(bp, want_bp)
    # one locus at a time gives the same
    at = 0
    for l in rc.cigar_unit_loci():
        g, b = capi.run_cigar_bp_diffs(lib, capi.cigar_request([l]), host=True)
        assert np.array_equal(g, want_got[at:at + len(g)]) and np.array_equal(b, want_bp[at:at + len(b)])
        at += len(g)


def test_cigar_refusals(lib):
    base = [(102, 147, 2, [(100, [("M", 50)]), (100, [("S", 3), ("M", 50)])])]
    def refused(msg, edit=None, null=(), loci=base):
        rq = capi.cigar_request(loci)
        if edit:
            edit(rq)
        with pytest.raises(RuntimeError, match=msg) as e:
            capi.run_cigar_bp_diffs(lib, rq, host=True, null=null)
        g, b = e.value.raw
        assert np.all(g == 0xEE) and np.all(b == capi.UNTOUCHED), "a refused call wrote"
    def put(name, i, v):
        def edit(rq):
            rq[name][i] = v
        return edit
    for nm in ("read_off", "read_start", "cigar_off", "cigar_op", "cigar_len", "region_start", "region_stop", "pad", "got", "bp_diff"):
        refused("null argument", null=(nm,))
    refused("negative read_start", put("read_start", 1, -1))
    refused("without CIGAR runs", put("cigar_off", 1, 0))
    refused("non-positive length", put("cigar_len", 1, 0))
    refused("non-positive length", put("cigar_len", 2, -4))
    refused("no SAM letter", put("cigar_op", 0, ord("m")))
    refused("no SAM letter", put("cigar_op", 0, 0))
    refused("below its region_start", put("pad", 0, -30))
    refused("below its region_start", put("region_stop", 0, 90))
    refused("outside int32", put("region_stop", 0, 2 ** 31 - 2))
    refused("outside int32", put("pad", 0, 2 ** 31 - 1))
    refused("leave int32", put("cigar_len", 2, 2 ** 31 - 1 - 102))
    refused("begin at 0", put("read_off", 0, 1))
    refused("begin at 0", put("cigar_off", 0, 1))
    refused("ascend", loci=base + [(5, 6, 0, [])], edit=put("read_off", 1, 3))
    # the largest positions that are allowed
    rq = capi.cigar_request([(5500, 2 ** 31 - 1 - 12, 2, [(5000, [("M", 1000), ("I", 7), ("M", 2 ** 31 - 1 - 1000 - 7 - 5000)])])])
    g, b = capi.run_cigar_bp_diffs(lib, rq, host=True)
    assert list(g) == [1] and list(b) == [7]
    # an empty request and a request of loci without reads
    g, b = capi.run_cigar_bp_diffs(lib, capi.cigar_request([]), host=True)
    assert len(g) == len(b) == 0
    g, b = capi.run_cigar_bp_diffs(lib, capi.cigar_request([(5, 6, 0, []), (7, 8, 1, [])]), host=True)
    assert len(g) == 0


# ------------------------------------------------------------------------------------------------------------------ histograms
def want_histograms(loci, strings):
    pair_off = [0]; value = []; count = []
    for s in strings:
        for v, c in rc.pairs_of_string(s):
            value.append(v); count.append(c)
        pair_off.append(len(value))
    assert len(pair_off) == 1 + sum(len(l) for l in loci)
    return np.asarray(pair_off, np.int32), np.asarray(value, np.int32), np.asarray(count, np.int32)


def test_histogram_cases_hold_what_they_name():
    loci = rc.histogram_loci()
    strings = rc.histogram_golden()
    samples = [s for l in loci for s in l]
    assert len(strings) == len(samples)
    kept = [sum(1 for x in s if x != rc.SKIP) for s in samples]
    assert {0, 1, 64, 65, rc.HISTOGRAM_DEVICE_READS, rc.HISTOGRAM_DEVICE_READS + 1} <= set(kept) and max(kept) >= 3000
    assert any(len(s) > 0 and k == 0 for s, k in zip(samples, kept)) and any(len(s) > rc.HISTOGRAM_DEVICE_READS and k == 0 for s, k in zip(samples, kept))
    assert "5|40" in strings and "." in strings and any(s.startswith("-") and ";0|" in s for s in strings)
    assert any(len(l) == 0 for l in loci)
    for s, text in zip(samples, strings):                           # the reference's strings are what their rule says
        vals = sorted(x for x in s if x != rc.SKIP)
        assert rc.pairs_of_string(text) == [(v, vals.count(v)) for v in sorted(set(vals))]


def test_histograms_equal_the_reference(lib):
    loci = rc.histogram_loci()
    a = rc.histogram_arrays(loci)
    pb = rc.post_batch(capi, a)
    po, hv, hc = capi.run_sample_histograms(lib, pb, a["value"], rc.SKIP, host=True)
    wo, wv, wc = want_histograms(loci, rc.histogram_golden())
    assert np.array_equal(po, wo) and np.array_equal(hv, wv) and np.array_equal(hc, wc)
    # another skip value: the sentinel is the call's argument, and INT32_MIN is then a value like any other
    po2, hv2, hc2 = capi.run_sample_histograms(lib, pb, a["value"], 2, host=True)
    for s, v in enumerate(x for l in loci for x in l):
        vals = sorted(x for x in v if x != 2)
        want = [(x, vals.count(x)) for x in sorted(set(vals))]
        assert list(zip(hv2[po2[s]:po2[s + 1]].tolist(), hc2[po2[s]:po2[s + 1]].tolist())) == want, s


def test_histogram_refusals(lib):
    a = rc.histogram_arrays([[[1, 2], [], [3]], [[4]]])
    def refused(msg, **edit):
        b = {k: v.copy() for k, v in a.items()}
        value = b["value"]
        for k, (i, v) in edit.items():
            b[k][i] = v
        pb = rc.post_batch(capi, b)
        with pytest.raises(RuntimeError, match=msg) as e:
            capi.run_sample_histograms(lib, pb, value, rc.SKIP, host=True)
        assert all(np.all(x == capi.UNTOUCHED) for x in e.value.raw), "a refused call wrote"
    refused("grouped by ascending", sample_label=(0, 1))
    refused("out of range", sample_label=(3, 1))
    refused("out of range", sample_label=(0, -1))
    refused("negative sample count", n_samples=(1, -1))
    refused("begin at 0", read_off=(0, 1))
    refused("ascend", read_off=(1, 5))
    pb = rc.post_batch(capi, a)
    with pytest.raises(RuntimeError, match="null argument"):
        capi.run_sample_histograms(lib, pb, None, rc.SKIP, host=True)
    pb.struct.sample_label = None
    with pytest.raises(RuntimeError, match="null argument"):
        capi.run_sample_histograms(lib, pb, a["value"], rc.SKIP, host=True)
    # nothing to do
    e = rc.histogram_arrays([])
    po, hv, hc = capi.run_sample_histograms(lib, rc.post_batch(capi, e), e["value"], rc.SKIP, host=True)
    assert list(po) == [0] and len(hv) == 0


# ------------------------------------------------------------------------------------------------------------------ the EM's reads
def em_case(seed, sizes, got_rate=0.85):
    """sizes: per locus the reads of every sample."""
    r = np.random.default_rng(seed)
    loci = [[[0] * n for n in s] for s in sizes]
    a = rc.histogram_arrays(loci)
    n = len(a["sample_label"])
    got = (r.random(n) < got_rate).astype(np.uint8)
    bp = r.integers(-40, 25, size=n).astype(np.int32)
    rs = r.integers(100, 200, size=len(sizes)).astype(np.int32)
    re_ = (rs + r.integers(0, 30, size=len(sizes))).astype(np.int32)
    log_p = (-r.random(n), -r.random(n))
    return a, got, bp, rs, re_, log_p


def same_batch(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("seed", [1, 2])
def test_em_batch_equals_the_restated_loop(lib, seed):
    a, got, bp, rs, re_, log_p = em_case(seed, [[5, 0, 9, 3], [0, 0], [], [40], [2, 2, 2, 2, 2, 2]])
    assert np.any(bp[got == 1] < -(re_.max() + 1 - rs.min())) or np.any(bp < -31)      # some reads fall below the floor
    for min_reads in (0, 6, 7, 100):
        for lp in (log_p, None):
            pb = rc.post_batch(capi, a, lp)
            if lp is None:
                pb.struct.log_p1 = None; pb.struct.log_p2 = None
            same_batch(capi.em_batch_from_bp_diffs(lib, pb, got, bp, rs, re_, min_reads), rc.em_batch_restated(a, got, bp, rs, re_, min_reads, lp))


def test_em_batch_floor_is_the_region_length(lib):
    """bp_diff == -(region_stop - region_start + 1) stays, one less goes (:119)."""
    a = rc.histogram_arrays([[[0, 0, 0]]])
    pb = rc.post_batch(capi, a)
    out = capi.em_batch_from_bp_diffs(lib, pb, [1, 1, 1], [-11, -12, 5], [100], [110], 2)
    assert list(out["num_bps"]) == [-11, 5] and list(out["too_few"]) == [0]
    assert list(capi.em_batch_from_bp_diffs(lib, pb, [1, 1, 1], [-11, -12, 5], [100], [110], 3)["too_few"]) == [1]


def test_em_batch_stops_behind_the_sample_that_passes_10000(lib):
    """The cut falls inside a sample: that sample's reads all enter, the next sample's none (:131-132); 10000 itself does not stop the walk."""
    sizes = [[6000, 3999, 5, 7, 11], [6000, 4000, 5, 7], [3]]
    a = rc.histogram_arrays([[[0] * n for n in s] for s in sizes])
    n = len(a["sample_label"])
    got = np.ones(n, np.uint8); bp = (np.arange(n) % 9 - 4).astype(np.int32)
    out = capi.em_batch_from_bp_diffs(lib, rc.post_batch(capi, a), got, bp, [10, 10, 10], [40, 40, 40], 10)
    assert list(out["read_off"]) == [0, 10004, 20009, 20012] and list(out["too_few"]) == [0, 0, 1]
    same_batch(out, rc.em_batch_restated(a, got, bp, [10, 10, 10], [40, 40, 40], 10))
    assert out["sample_label"][10003] == 2 and out["sample_label"][20008] == 2


def test_em_batch_refusals(lib):
    a = rc.histogram_arrays([[[0, 0], [0]]])
    pb = rc.post_batch(capi, a)
    for msg, args in (("region_stop < region_start", ([1, 1, 1], [0, 0, 0], [10], [9], 0)), ("must not be negative", ([1, 1, 1], [0, 0, 0], [10], [19], -1))):
        with pytest.raises(RuntimeError, match=msg):
            capi.em_batch_from_bp_diffs(lib, pb, *args)
    pb.struct.log_p2 = None
    with pytest.raises(RuntimeError, match="log_p1 without log_p2"):
        capi.em_batch_from_bp_diffs(lib, pb, [1, 1, 1], [0, 0, 0], [10], [19], 0)
    b = dict(a, sample_label=np.asarray([1, 0, 0], np.int32))
    with pytest.raises(RuntimeError, match="grouped by ascending"):
        capi.em_batch_from_bp_diffs(lib, rc.post_batch(capi, b), [1, 1, 1], [0, 0, 0], [10], [19], 0)


def test_em_batch_feeds_the_cigars_of_a_locus(lib):
    """The two calls in a row, as learn_stutter_model runs them: ExtractCigar with the period as pad, then the loop."""
    loci = rc.cigar_fuzz_loci(5, n_loci=6, max_reads=30)
    rq = capi.cigar_request(loci)
    got, bp = capi.run_cigar_bp_diffs(lib, rq, host=True)
    samples = [[[0] * (len(l[3]) // 3), [0] * (len(l[3]) - len(l[3]) // 3)] for l in loci]
    a = rc.histogram_arrays(samples)
    assert np.array_equal(a["read_off"], rq["read_off"])
    out = capi.em_batch_from_bp_diffs(lib, rc.post_batch(capi, a), got, bp, rq["region_start"], rq["region_stop"], 4)
    same_batch(out, rc.em_batch_restated(a, got, bp, rq["region_start"], rq["region_stop"], 4))
    assert 0 < out["read_off"][-1] < len(got)


# ------------------------------------------------------------------------------------------------------------------ names, the program
def test_names_agree(lib):
    """The header declares the entry points, the export map lets them through, the library has them and capi.py binds them; capi.py's
    struct has the header's fields in the header's order; the caps are one number in the header, the layout and capi.py."""
    raw = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", lambda m: " ", raw, flags=re.S)
    declared = set(re.findall(r"\b(hipstr_[a-z0-9_]+)\s*\(", hdr))
    patterns = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "hipstr_amd", "csrc", "exports.map")).read(), flags=re.S))
    patterns = [p.strip() for p in ",".join(patterns).split(",")]
    capi._record_reads_sigs(lib)
    for n in capi.RECORD_READS_NAMES:
        assert n in declared and any(fnmatch.fnmatchcase(n, p) for p in patterns) and hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    body = re.search(r"typedef struct hipstr_cigar_request \{(.*?)\} hipstr_cigar_request_t;", raw, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        fields += [f.strip(" *\n") for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if f.strip(" *\n")]
    assert fields == [f for f, _ in capi.HipstrCigarRequest._fields_]
    layout = open(os.path.join(ROOT, "hipstr_amd", "csrc", "record_reads_layout.h")).read()
    for name, lname, val in (("HIPSTR_CIGAR_DEVICE_RUNS", "HS_RR_CIGAR_RUNS", capi.CIGAR_DEVICE_RUNS), ("HIPSTR_HISTOGRAM_DEVICE_READS", "HS_RR_HIST_READS", capi.HISTOGRAM_DEVICE_READS)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, raw).group(1)) == int(re.search(r"#define %s\s+(\d+)" % lname, layout).group(1)) == val
    assert (rc.CIGAR_DEVICE_RUNS, rc.HISTOGRAM_DEVICE_READS, rc.SKIP) == (capi.CIGAR_DEVICE_RUNS, capi.HISTOGRAM_DEVICE_READS, capi.NO_ML_BP)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/cpp/record_reads_host_test.cpp with the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
    exe = str(tmp_path_factory.mktemp("record_reads") / "record_reads_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "record_reads_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "record_reads_host.cpp")], check=True)
    return exe


def test_sanitized_program_self_test(program):
    r = subprocess.run([program, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_sanitized_program_on_the_golden(program, tmp_path):
    """The lane body, the wavefront's steps and the host twin inside the sanitized program, on every case of the goldens: the reference's
    verdicts and strings."""
    src, dst = str(tmp_path / "cases.txt"), str(tmp_path / "results.txt")
    with open(src, "w") as f:
        f.write(rc.cigar_text(rc.cigar_loci()) + rc.histogram_text(rc.histogram_loci()))
    r = subprocess.run([program, "cases", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = open(dst).read().splitlines()
    got, bp = rc.cigar_golden()
    assert lines[:len(got)] == ["%d %d" % x for x in zip(got.tolist(), bp.tolist())]
    assert lines[len(got):] == rc.histogram_golden()
