"""CPU: hipstr_record_alleles_host (include/hipstr_hmm.h; hipstr_amd/csrc/record_alleles_host.cpp) against what the compiled reference's
get_alleles and reorder_alleles returned on the same cases (tests/golden/record_alleles_*.npz, written by
tests/golden/make_golden_record_alleles.py through `genotype_flow --record-cases`), byte for byte; the two refusal statuses; the flank
option strings against the Python restatement of seq_stutter_genotyper.cpp:1013-1040 (tests/record_alleles_cases.py); the call's
refusals; the names; and the stand-alone program tests/cpp/record_alleles_host_test.cpp built with -fsanitize=address,undefined (run as a
program: nothing is preloaded)."""
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import record_alleles_cases as ac

ROOT = ac.ROOT
REFUSED = {"duplicate_strings": ac.DUPLICATE, "pad_before_window": ac.OUTSIDE}


@pytest.fixture(scope="module")
def lib(hmm_host):
    return hmm_host


def check_against(got, cases, gold, what):
    """A call's per-locus results against the golden's records and the restated flanks."""
    assert len(got) == len(cases)
    for g, c in zip(got, cases):
        nm = "%s %s" % (what, c["name"])
        V = len(c["blocks"][1][2])
        if c["name"] in REFUSED or c["name"] not in gold:
            st = REFUSED.get(c["name"], ac.OUTSIDE)
            assert g["status"] == st and g["pos"] == g["left_trim"] == g["right_trim"] == 0, nm
            assert g["alleles"] == [b""] * V and g["bp_diff"] == [0] * V and g["old_to_new"] == g["new_to_old"] == [-1] * V, nm
            assert all(s == b"" for s in g.get("lflanks", []) + g.get("rflanks", [])), nm
            continue
        w = gold[c["name"]]
        assert (g["pos"], g["left_trim"], g["right_trim"]) == (w["pos"], w["left_trim"], w["right_trim"]), nm
        assert g["alleles"] == w["alleles"] and g["old_to_new"] == w["old_to_new"] and g["new_to_old"] == w["new_to_old"], nm
        assert g["bp_diff"] == [len(a) - len(w["alleles"][0]) for a in w["alleles"]], nm
        if "lflanks" in g:
            fl = ac.flanks_restated(c, w["left_trim"], w["right_trim"])
            assert g["status"] == (0 if fl else ac.FLANK_ASSERT), nm
            assert (g["lflanks"], g["rflanks"]) == (fl if fl else ([b""] * len(c["blocks"][0][2]), [b""] * len(c["blocks"][2][2]))), nm
        else:
            assert g["status"] == 0, nm


def test_cases_hold_what_they_name():
    g = ac.golden("unit")
    names = [c["name"] for c in ac.unit_cases()]
    assert sorted(g) == sorted(names) and all(os.path.getsize(p) < 64 * 1024 for p in ac.GOLDEN.values())
    V = {c["name"]: len(c["blocks"][1][2]) for c in ac.unit_cases()}
    assert (V["v1"], V["v2"], V["v65"]) == (1, 2, 65)
    assert g["trim_to_region_edge"]["left_trim"] == 10                                   # stopped by the region (the options share 15)
    assert g["trim_stopped_by_short_option"]["left_trim"] == 3 and min(len(a) for a in g["trim_stopped_by_short_option"]["alleles"]) == 1
    assert g["right_trim_to_region_edge"]["right_trim"] == 10 and g["right_trim_stopped_by_short_option"]["right_trim"] == 3
    assert g["left_flank_from_window"]["left_trim"] == -6 and g["left_flank_from_window"]["alleles"][0][:6] == ac.REF[150:156] != ac.CHROM[150:156]
    assert g["right_flank_before_region_stop"]["right_trim"] == -7 and g["right_flank_before_region_stop"]["alleles"][0][-7:] == ac.REF[163:170]
    for nm in ("empty_option", "first_bases_differ", "pad_after_trim_before_region"):
        assert all(a[:1] == ac.REF[g[nm]["pos"] - 1:g[nm]["pos"]] for a in g[nm]["alleles"]), nm
    assert g["empty_option"]["pos"] == 150 and g["empty_option"]["left_trim"] == -1 and g["empty_option"]["alleles"][1] == ac.REF[149:150]
    assert g["late_byte_compare"]["new_to_old"] == [0, 3, 2, 1, 4]
    assert g["unsigned_bytes"]["new_to_old"] == [0, 4, 2, 3, 1]                          # 0x80 and 0xC8 behind the letters
    assert -1 in g["duplicate_strings"]["old_to_new"]                                    # the reference's map lost an index
    r = ac.golden("random")
    assert len(r) == 60 and any(len(x["alleles"]) > 64 for x in r.values()) and any(x["new_to_old"] != sorted(x["new_to_old"]) for x in r.values())
    assert {c["name"] for c in ac.unit_cases() if ac.flanks_restated(c, g[c["name"]]["left_trim"], g[c["name"]]["right_trim"]) is None} >= {"right_flank_before_region_stop", "region_far_wider_than_block"}


@pytest.mark.parametrize("batch", sorted(ac.BATCHES))
def test_equals_the_reference(lib, batch):
    cases = ac.BATCHES[batch]()
    gold = ac.golden(batch)
    check_against(capi.run_record_alleles(lib, [ac.locus_of(c) for c in cases], host=True), cases, gold, batch)
    check_against(capi.run_record_alleles(lib, [ac.locus_of(c) for c in cases], host=True, flanks=False), cases, gold, batch + " without flanks")
    for c in cases[:12]:                                                                 # one locus at a time gives the same
        check_against(capi.run_record_alleles(lib, [ac.locus_of(c)], host=True), [c], gold, batch + " alone")


def test_statuses_the_reference_cannot_show(lib):
    cases = ac.no_reference_cases() + [ac.beyond_cap_case()]
    got = capi.run_record_alleles(lib, [ac.locus_of(c) for c in cases], host=True)
    assert got[0]["status"] == ac.OUTSIDE and got[0]["alleles"] == [b"", b""]
    big = got[1]
    opts = cases[1]["blocks"][1][2]
    assert big["status"] == 0 and len(big["alleles"]) == 300 and big["left_trim"] == 4 and big["right_trim"] == 4
    assert big["alleles"] == [o[4:-4] for o in opts]
    order = sorted(range(1, 300), key=lambda i: (len(opts[i]), opts[i]))
    assert big["new_to_old"] == [0] + order and [big["old_to_new"][i] for i in big["new_to_old"]] == list(range(300))
    # a window cut short at the chromosome's end: the right flank is not there
    c = ac.case("cut_window", 150, 170, 150, 163, [ac.REF[150:163], ac.REF[150:161]])
    L = ac.locus_of(c); L["window"] = L["window"][:40 + 18]
    assert capi.run_record_alleles(lib, [L], host=True)[0]["status"] == ac.OUTSIDE


def test_refusals(lib):
    c = ac.unit_cases()[3]
    def refused(msg, edit=None, **kw):
        L = ac.locus_of(c)
        if edit:
            edit(L)
        with pytest.raises(RuntimeError, match=msg) as e:
            capi.run_record_alleles(lib, [L], host=True, **kw)
        for k, v in e.value.raw.items():
            assert np.all(v == (0xEE if v.dtype == np.uint8 else capi.UNTOUCHED)), k
    refused("region_stop < region_start", lambda L: L.update(region_stop=L["region_start"] - 1))
    refused("a block 1 without options", lambda L: L.update(blocks=[L["blocks"][0], (140, 172, []), L["blocks"][2]]), caps=(10, 100, 100))
    refused("cap_alleles is too small", caps=(10, 1000, 1000))
    refused("cap_lflanks is too small", caps=(1000, 3, 1000))
    refused("cap_rflanks is too small", caps=(1000, 1000, 3))
    for nm in ("status", "pos", "left_trim", "right_trim", "allele_off", "alleles", "allele_bp_diff", "old_to_new", "new_to_old", "lflanks", "rflanks"):
        refused("null argument", null=(nm,))
    assert capi.run_record_alleles(lib, [], host=True) == []


def test_names_agree(lib):
    raw = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", lambda m: " ", raw, flags=re.S)
    declared = set(re.findall(r"\b(hipstr_[a-z0-9_]+)\s*\(", hdr))
    patterns = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "hipstr_amd", "csrc", "exports.map")).read(), flags=re.S))
    patterns = [p.strip() for p in ",".join(patterns).split(",")]
    capi._record_alleles_sigs(lib)
    for n in capi.RECORD_ALLELES_NAMES:
        assert n in declared and any(fnmatch.fnmatchcase(n, p) for p in patterns) and hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    for struct, cls in (("hipstr_record_alleles_request", capi.HipstrRecordAllelesRequest), ("hipstr_record_alleles_out", capi.HipstrRecordAllelesOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), raw, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip(" *\n") for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if f.strip(" *\n")]
        assert fields == [f for f, _ in cls._fields_], struct
    layout = open(os.path.join(ROOT, "hipstr_amd", "csrc", "record_alleles_layout.h")).read()
    assert int(re.search(r"#define HIPSTR_ALLELES_DEVICE_OPTIONS\s+(\d+)", raw).group(1)) == int(re.search(r"#define HS_RA_MAX_OPTIONS\s+(\d+)", layout).group(1)) \
        == capi.ALLELES_DEVICE_OPTIONS == ac.DEVICE_OPTIONS
    for name, val in (("DUPLICATE", ac.DUPLICATE), ("OUTSIDE_WINDOW", ac.OUTSIDE), ("FLANK_ASSERT", ac.FLANK_ASSERT)):
        assert int(re.search(r"#define HIPSTR_ALLELES_%s\s+(\d+)" % name, raw).group(1)) == val


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("record_alleles") / "record_alleles_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "record_alleles_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "record_alleles_host.cpp")], check=True)
    return exe


def test_sanitized_program_self_test(program):
    r = subprocess.run([program, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


@pytest.mark.parametrize("batch", sorted(ac.BATCHES))
def test_sanitized_program_on_the_golden(program, tmp_path, batch):
    """The replayed wavefront and the host twin inside the sanitized program on the golden's cases: the reference's records."""
    src, dst = str(tmp_path / "cases.txt"), str(tmp_path / "results.txt")
    with open(src, "w", encoding="latin-1") as f:
        f.write(ac.cases_text(ac.BATCHES[batch]()))
    r = subprocess.run([program, "cases", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    text = open(dst, encoding="latin-1").read()
    got = ac.parse_results(text)
    gold = ac.golden(batch)
    for nm, w in gold.items():
        if nm in REFUSED:
            assert got[nm] == {} and ("case %s\nstatus %d\n" % (nm, REFUSED[nm])) in text, nm
        else:
            assert got[nm] == w, nm
