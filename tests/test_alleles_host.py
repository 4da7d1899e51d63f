"""CPU: hipstr_alleles_apply_host and hipstr_alleles_step(HIPSTR_ALLELES_ON_HOST) (hipstr_amd/csrc/alleles_host.cpp) against the records of
the reference's own HapBlock / RepeatBlock / Haplotype (tests/golden/alleles_*.npz): the new blocks, the haplotypes in visit order,
allele_mapping and realign_to_haplotype by the rule of seq_stutter_genotyper.cpp:331-336 / :358-367 — and, with the haplotype hash cut to 4
bits, the same bytes from many more byte comparisons: the hash only filters."""
import numpy as np
import pytest

from hipstr_amd import capi
import alleles_cases as ac
import alleles_checks as chk


@pytest.fixture
def lib(hmm_host):
    capi._alleles_sigs(hmm_host)
    assert hmm_host.hipstr_debug_alleles_hash_bits(0) == 0
    yield hmm_host
    hmm_host.hipstr_debug_alleles_hash_bits(0)


def test_limits_are_the_ones_the_cases_are_built_around(lib):
    assert capi.alleles_limits(lib) == dict(threads=ac.THREADS, max_haps=ac.MAX_HAPS, max_opts=ac.MAX_OPTS, slots=2 * ac.MAX_HAPS)


@pytest.mark.parametrize("batch", sorted(ac.BATCHES))
def test_golden_batches(lib, batch):
    a, cases = chk.run_golden(lib, batch, host=True)
    last = capi.alleles_last(lib)
    assert last["device_loci"] == 0 and last["host_loci"] == sum(c["on"] for c in cases)


def test_off_locus_ignores_its_keep_and_locus_on_null_does_not(lib):
    cases, _ = chk.golden("unit")
    off = [c["name"] for c in cases].index("off_between")
    a = chk.apply_cases(lib, cases, host=True)
    b = chk.apply_cases(lib, cases, host=True, all_on=True)
    assert int(a.new_n_alleles[off]) == 6 and int(b.new_n_alleles[off]) == 2          # [2,3,1] as it was; with the keep applied [1,2,1]


@pytest.mark.parametrize("batch", ["unit", "random"])
def test_bytes_decide_when_hashes_collide(lib, batch):
    full, cases = chk.run_golden(lib, batch, host=True)
    n64 = capi.alleles_last(lib)["compares"]
    assert lib.hipstr_debug_alleles_hash_bits(4) == 0
    cut, _ = chk.run_golden(lib, batch, host=True)
    n4 = capi.alleles_last(lib)["compares"]
    chk.same(cut, full, "4-bit hash against 64-bit hash")
    assert n4 > n64, (n4, n64)


def test_refusals(lib):
    chk.refusals(lib, host=True)


def test_policy_against_flow_chain_state(lib, oracle):
    chk.policy(lib, oracle, host=True)


def test_host_form_under_sanitizers(tmp_path):
    """alleles_host.cpp next to a program with a main of its own (tests/cpp/alleles_host_main.cpp), both built with AddressSanitizer and UBSan,
    the runtimes linked statically: nothing is preloaded and nothing of it is loaded into python.  It runs the `unit` cases."""
    import os
    import subprocess
    root = os.path.dirname(ac.HERE)
    cases, recs = chk.golden("unit")
    src = tmp_path / "cases.txt"; src.write_text(ac.case_text(cases))
    exe = str(tmp_path / "alleles_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall",
                           os.path.join(root, "tests", "cpp", "alleles_host_main.cpp"), os.path.join(root, "hipstr_amd", "csrc", "alleles_host.cpp"), "-o", exe])
    r = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        w = line.split(" "); i, j = w.index("map"), w.index("realign")
        mapping, realign = ac.expected_of(recs[c["name"]])
        assert w[1] == c["name"] and [int(x) for x in w[3:6]] == [len(o) for _, _, o in recs[c["name"]]["blocks"]]
        assert [int(x) for x in w[i + 1:j]] == list(mapping) and [int(x) for x in w[j + 1:]] == list(realign), c["name"]
