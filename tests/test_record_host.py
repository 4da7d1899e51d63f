"""CPU: the host forms of the record's numeric fields — hipstr_bias_pvalues_host and hipstr_record_fields_host (include/hipstr_hmm.h;
hipstr_amd/csrc/record_host.cpp).  The p-values against the compiled reference routines (cephes' bdtr, htslib's kt_fisher_exact:
tests/golden/record_pvalues.npz, written by tests/golden/make_record_golden.py) bit for bit; the record's three sample loops against their
numpy restatement (tests/record_cases.py, with the reference's line numbers); the refusals; the names in the header, the export map and
capi.py; and the stand-alone program tests/cpp/record_host_test.cpp built with -fsanitize=address,undefined (run as a program: nothing is
preloaded)."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import record_cases as rc

ROOT = rc.ROOT


@pytest.fixture(scope="module")
def lib(hmm_host):
    return hmm_host


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_golden_is_the_golden_of_these_cases():
    z = np.load(rc.GOLDEN)
    assert sorted(z.files) == ["ab_large", "ab_small", "fs_large", "fs_small"]
    assert all(z[k].dtype == np.uint64 for k in z.files)
    assert len(z["ab_small"]) == 625 and len(z["fs_small"]) == 13 ** 4 and len(z["ab_large"]) == len(z["fs_large"]) == len(rc.large()[0])
    assert os.path.getsize(rc.GOLDEN) <= 300 * 1024
    # what the cases are there for
    u1, u2, r1, r2 = (x.astype(np.int64) for x in rc.large())
    n, k = u1 + u2, np.minimum(u1, u2)
    assert {0, 1, 2} <= set(k.tolist()) and np.any(n == 2 * k + 1) and np.any((n >= 165) & (n <= 176)) and n[n <= rc.TABLE_READS].max() == 5000
    assert np.any(n > rc.TABLE_READS) and max(r1.max(), r2.max(), (u1 - r1).max(), (u2 - r2).max()) >= 2500
    f = [x.astype(np.int64) for x in rc.fs_small()]
    n11 = f[0] - f[2]
    lower_end = n11 + (f[0] + f[1]) - f[0] - (n11 + f[1] - f[3])          # n11 + n - n1_ - n_1
    assert np.any(n11 % 11 == 0) and np.any(n11 == 11) and np.any(lower_end == 0)


def test_pvalues_equal_the_reference_bit_for_bit(lib):
    g = rc.golden()
    a1, a2 = rc.ab_small()
    z = np.zeros_like(a1)
    ab, fs = capi.bias_pvalues(lib, a1, a2, z, z, host=True)
    assert np.array_equal(bits(ab), bits(g["ab_small"]))
    # the three exact values of compute_allele_bias (:972-977)
    assert ab[0] == 1.0 and np.all(ab[(a1 == a2) & (a1 > 0)] == 0.0) and not np.signbit(ab[26])
    ab, fs = capi.bias_pvalues(lib, *rc.fs_small(), host=True)
    assert np.array_equal(bits(fs), bits(g["fs_small"]))
    ab, fs = capi.bias_pvalues(lib, *rc.large(), host=True)
    assert np.array_equal(bits(ab), bits(g["ab_large"])) and np.array_equal(bits(fs), bits(g["fs_large"]))
    # bdtr(4, 9, .5) is 0x1.0000000000001p-1: twice that exceeds 1 and only the clamp gives log10(1) = 0
    ab, _ = capi.bias_pvalues(lib, [4], [5], [0], [0], host=True)
    assert ab[0] == 0.0 and not np.signbit(ab[0])


def test_pvalues_refusals(lib):
    one = np.array([3], np.int32)
    for kw, word in ((dict(uniq_one=[-1]), "negative"), (dict(rv_uniq_two=[-2]), "negative"), (dict(rv_uniq_one=[4]), "rv_uniq exceeds uniq"),
                     (dict(rv_uniq_two=[9]), "rv_uniq exceeds uniq"), (dict(uniq_two=None), "null argument"), (dict(n=-1), "must not be negative")):
        a = dict(uniq_one=one, uniq_two=one, rv_uniq_one=[1], rv_uniq_two=[1]); a.update(kw)
        with pytest.raises(RuntimeError, match=word):
            capi.bias_pvalues(lib, host=True, **a)
    ab, fs = capi.bias_pvalues(lib, [], [], [], [], host=True)
    assert len(ab) == 0 and len(fs) == 0


def host_pvalues(lib):
    def f(u1, u2, r1, r2):
        ab, fs = capi.bias_pvalues(lib, [u1], [u2], [r1], [r2], host=True)
        return ab[0], fs[0]
    return f


def post_batch(b):
    """The posterior batch of a fields batch: only n_loci, n_alleles, n_samples and haploid are read by the host form."""
    z = np.zeros(0)
    return capi.PostBatch(b.n_alleles, b.n_samples, np.zeros(b.n_loci + 1, np.int32), np.zeros(0, np.int32), z, z, np.zeros(0, np.int32), z, haploid=b.haploid)


def counts_of(b):
    return {nm: getattr(b, nm) for nm in capi.RECORD_COUNTS}


def run_host(lib, b, **kw):
    a = dict(n_variants=b.n_variants, hap_to_allele=b.hap_to_allele, counts=counts_of(b), map_gt=b.map_gt, sample_reported=b.reported,
             sample_masked=b.masked, max_flank_indel_frac=b.frac)
    a.update(kw)
    return capi.run_record_fields(lib, post_batch(b), **a)


def assert_fields(got, want, exact_doubles=True, what=""):
    for k in rc.INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in ("ab", "fs"):
        if exact_doubles:
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)
        else:
            same = (got[k] == want[k])
            assert np.all(same[(want[k] == rc.NOT_APPLICABLE) | (want[k] == 1.0) | np.isinf(want[k])]), (what, k)
            assert np.all(np.abs(got[k][~same] - want[k][~same]) <= 1e-9), (what, k)


@pytest.mark.parametrize("seed", rc.FIELD_SEEDS)
def test_fields_equal_the_restated_loops(lib, seed):
    b = rc.fields_batch(seed)
    want = rc.expect_fields(b, host_pvalues(lib))
    assert_fields(run_host(lib, b), want, what=seed)
    # without the optional arrays: every sample reported, none masked
    b.reported[:] = 1; b.masked[:] = 0
    want = rc.expect_fields(b, host_pvalues(lib))
    assert_fields(run_host(lib, b, sample_reported=None, sample_masked=None), want, what=seed)


def test_cases_reach_what_they_name(lib):
    combos, seen = set(), dict(status=set(), float_edge=0, masked_and_over=0, hom_hap_het_gt=0, het=0, hom=0, ab_one=0, ab_zero=0)
    for seed in rc.FIELD_SEEDS:
        b = rc.fields_batch(seed)
        got = run_host(lib, b)
        over = (b.n_aligned > 0) & (b.n_flank_indel.astype(np.float32) > np.float32(0.15) * b.n_aligned.astype(np.float32))
        combos |= set(zip(b.reported.tolist(), (b.n_aligned == 0).tolist(), b.masked.tolist(), (b.n_flank_indel > 3 * b.n_aligned // 20).tolist()))
        seen["status"] |= set(got["status"].tolist())
        # the float comparison: with n_flank_indel == 3 n / 20 exactly, 0.15f * n (0.15f > 0.15) rounds to the float 3 n / 20 and the
        # sample is NOT over the fraction; one read more is
        edge = (b.n_aligned > 0) & (b.n_flank_indel * 20 == 3 * b.n_aligned)
        assert not np.any(edge & over) and np.all(over[(b.n_aligned > 0) & (b.n_flank_indel == 3 * b.n_aligned // 20 + 1)])
        seen["float_edge"] += int(np.sum(edge))
        seen["masked_and_over"] += int(np.sum(b.reported.astype(bool) & b.masked.astype(bool) & over))
        computed = got["ab"] != rc.NOT_APPLICABLE
        seen["het"] += int(np.sum(computed)); seen["hom"] += int(np.sum((got["status"] == rc.PASS) & ~computed))
        seen["hom_hap_het_gt"] += int(np.sum(computed & (got["gt"][:, 0] == got["gt"][:, 1])))       # haplotypes differ, genotypes do not
        seen["ab_one"] += int(np.sum(got["ab"] == 1.0)); seen["ab_zero"] += int(np.sum(got["ab"] == 0.0))
        assert b.haploid.sum() == 1 and (b.n_variants == 1).sum() == 1
    assert len(combos) == 16
    assert seen["status"] == {rc.PASS, rc.NO_READS, rc.MASKED, rc.FLANK_INDEL_FRAC, rc.NOT_REPORTED}
    for k in ("float_edge", "masked_and_over", "hom_hap_het_gt", "het", "hom", "ab_one", "ab_zero"):
        assert seen[k] > 0, k


def test_fraction_is_the_requests(lib):
    b = rc.fields_batch(0)
    b.reported[:] = 1; b.masked[:] = 0
    b.frac = 0.5
    want = rc.expect_fields(b, host_pvalues(lib))
    got = run_host(lib, b)
    assert_fields(got, want)
    assert not np.array_equal(got["status"], run_host(lib, b, max_flank_indel_frac=0.0)["status"])


def refused(run, b, word, **kw):
    with pytest.raises(RuntimeError, match=word) as e:
        run(b, **kw)
    for k, v in e.value.raw.items():
        assert np.all(np.isnan(v)) if v.dtype == np.float64 else np.all(v == capi.UNTOUCHED), k


def common_refusals(run):
    """The refusals both forms share; run(b, **changes)."""
    b = rc.fields_batch(0)
    b.reported[:] = 1; b.masked[:] = 0
    for nm in ("n_variants", "hap_to_allele"):
        refused(run, b, "null argument", **{nm: None})
    for nm in capi.RECORD_COUNTS:
        c = counts_of(b); c[nm] = None
        refused(run, b, "null argument", counts=c)
        c = counts_of(b); c[nm] = c[nm].copy(); c[nm][4] = -1
        refused(run, b, "negative", counts=c)
    for nm in ("status", "ab", "allele_count", "dflankindel"):
        refused(run, b, "null argument", null_out=nm)
    for one, rv in (("uniq_one", "rv_uniq_one"), ("uniq_two", "rv_uniq_two")):
        c = counts_of(b); c[rv] = c[rv].copy(); c[rv][2] = c[one][2] + 1
        refused(run, b, "rv_uniq exceeds uniq", counts=c)
    h = b.hap_to_allele.copy(); h[1] = int(b.n_variants[0])
    refused(run, b, r"hap_to_allele outside \[0, n_variants\)", hap_to_allele=h)
    v = b.n_variants.copy(); v[2] = 0
    refused(run, b, "n_variants below 1", n_variants=v)
    refused(run, b, "must not be negative", max_flank_indel_frac=-0.5)


def haploid_het(b):
    """A batch whose haploid locus has a counted sample with a heterozygous genotype."""
    b.reported[:] = 1; b.masked[:] = 0
    l = int(np.argmax(b.haploid)); s = 7 * l + 1
    b.n_aligned[s] = 20; b.n_flank_indel[s] = 0
    ho = int(b.n_alleles[:l].sum())
    b.map_gt[s] = (0, 1)
    assert b.hap_to_allele[ho] != b.hap_to_allele[ho + 1]
    return b, s


def test_refusals(lib):
    common_refusals(lambda b, **kw: run_host(lib, b, **kw))
    b, s = haploid_het(rc.fields_batch(1, haploid_locus=0, one_variant_locus=2))
    refused(lambda b, **kw: run_host(lib, b, **kw), b, "heterozygous genotype at a haploid locus")
    b.masked[s] = 1                      # not counted: the reference's assertion is never reached
    run_host(lib, b)
    b.masked[s] = 0
    m = b.map_gt.copy(); m[s] = (-1, -1)
    refused(lambda b, **kw: run_host(lib, b, **kw), b, "without a MAP pair", map_gt=m)
    m[s] = (0, int(b.n_alleles[0]))
    refused(lambda b, **kw: run_host(lib, b, **kw), b, "map_gt outside", map_gt=m)
    with pytest.raises(RuntimeError, match="null argument"):
        capi._record_sigs(lib)
        if lib.hipstr_record_fields_host(None, None, None, None) != 0:
            raise RuntimeError(lib.hipstr_last_error().decode())


def test_empty_batch(lib):
    pb = capi.PostBatch([], [], [0], [], [], [], [], [])
    got = capi.run_record_fields(lib, pb, [], [], {nm: [] for nm in capi.RECORD_COUNTS}, map_gt=np.zeros(0, np.int32))
    assert all(len(v) == 0 for v in got.values())
    # loci without samples
    pb = capi.PostBatch([2, 3], [0, 0], [0, 0, 0], [], [], [], [], [])
    got = capi.run_record_fields(lib, pb, [2, 1], [0, 1, 0, 0, 0], {nm: [] for nm in capi.RECORD_COUNTS}, map_gt=np.zeros(0, np.int32))
    assert list(got["allele_count"]) == [0, 0, 0] and list(got["an"]) == [0, 0] and list(got["dp"]) == [0, 0]


def test_names_agree(lib):
    """The header declares the new entry points, the export map lets them through, the library has them and capi.py binds them; the
    structs of capi.py have the header's fields in the header's order."""
    hdr = re.sub(r"/\*.*?\*/", lambda m: " ", open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hipstr_[a-z0-9_]+)\s*\(", hdr))
    patterns = re.findall(r"global:\s*([^;]+);", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "hipstr_amd", "csrc", "exports.map")).read(), flags=re.S))
    patterns = [p.strip() for p in ",".join(patterns).split(",")]
    capi._record_sigs(lib)
    for n in capi.RECORD_NAMES:
        assert n in declared and any(fnmatch.fnmatchcase(n, p) for p in patterns) and hasattr(lib, n) and getattr(lib, n).argtypes is not None, n
    raw = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read()
    for struct, cls in (("hipstr_record_request", capi.HipstrRecordRequest), ("hipstr_record_out", capi.HipstrRecordOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), raw, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            fields += [f.strip(" *\n") for f in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip()).split(",") if f.strip(" *\n")]
        assert fields == [f for f, _ in cls._fields_], struct
    for name, val in (("HIPSTR_RECORD_PASS", capi.RECORD_PASS), ("HIPSTR_RECORD_NO_READS", capi.RECORD_NO_READS), ("HIPSTR_RECORD_MASKED", capi.RECORD_MASKED),
                      ("HIPSTR_RECORD_FLANK_INDEL_FRAC", capi.RECORD_FLANK_INDEL_FRAC), ("HIPSTR_RECORD_TABLE_READS", capi.RECORD_TABLE_READS)):
        assert int(re.search(r"#define %s\s+\(?(-?\d+)" % name, raw).group(1)) == val, name
    layout = open(os.path.join(ROOT, "hipstr_amd", "csrc", "record_layout.h")).read()
    assert int(re.search(r"#define HS_REC_TABLE_READS (\d+)", layout).group(1)) == capi.RECORD_TABLE_READS == rc.TABLE_READS


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/cpp/record_host_test.cpp with the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
    exe = str(tmp_path_factory.mktemp("record") / "record_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "record_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "record_host.cpp")], check=True)
    return exe


def test_sanitized_program_self_test(program):
    r = subprocess.run([program, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


def test_sanitized_program_on_the_golden(program, tmp_path):
    """The host twin inside the sanitized program, on every quadruple of the golden: the reference's bits."""
    u1, u2, r1, r2, ab, fs = rc.all_quadruples()
    src, dst = str(tmp_path / "quadruples.txt"), str(tmp_path / "values.txt")
    with open(src, "w") as f:
        f.write("".join("%d %d %d %d\n" % q for q in zip(u1.tolist(), u2.tolist(), r1.tolist(), r2.tolist())))
    r = subprocess.run([program, "pvalues", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    v = np.array([[int(x, 16) for x in line.split()] for line in open(dst)], np.uint64)
    assert v.shape == (len(u1), 2)
    has_ab, has_fs = ~np.isnan(ab), ~np.isnan(fs)
    assert np.array_equal(v[has_ab, 0], bits(ab)[has_ab]) and np.array_equal(v[has_fs, 1], bits(fs)[has_fs])
