"""CPU: the host entry points of the flank reassembly — hipstr_flank_kmer_lengths and hipstr_flank_assemble (include/hipstr_hmm.h;
hipstr_amd/csrc/flank_host.cpp) — against the records of the reference's own DebruijnGraph (tests/golden/flank_*.npz, written by
tests/golden/make_golden_flank.py through `genotype_flow --debruijn-cases`): per task k, the paths in pop order and their weights, and, on
those records, the aggregation of seq_stutter_genotyper.cpp:99-201 restated in tests/flank_cases.py: statuses, options, masks.  Also the
refusals, the return-3 convention, and the stand-alone program tests/cpp/flank_host_test.cpp built with -fsanitize=address,undefined: the
host twin and the device's task body (run as plain C++) on the same case text and on random tasks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import flank_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return capi.load_hmm()


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name, make in fc.BATCHES.items():
        c = fc.build(make())
        text, records = fc.golden(name)
        assert fc.case_text(c) == text, "tests/golden/flank_%s.npz is not the golden of this batch: run tests/golden/make_golden_flank.py" % name
        out[name] = (c, records)
    return out


@pytest.mark.parametrize("name", sorted(fc.BATCHES))
def test_host_entry_point_equals_the_reference(lib, batches, name):
    c, records = batches[name]
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c))
    fc.assert_matches(c, got, fc.expect(c, records), name)
    km = capi.flank_kmer_lengths(lib, C.pointer(c.pooled))
    for l, L in enumerate(c.loci):
        assert [int(km[l, f]) for f in range(2)] == [records["%s.%d" % (L["name"], f)]["kmer"] for f in range(2)], L["name"]


def test_unit_cases_reach_what_they_name(lib, batches):
    c, records = batches["unit"]
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c))
    loc = {L["name"]: l for l, L in enumerate(c.loci)}
    ss = lambda nm: list(got["sample_status"][int(c.samp_off[loc[nm]]):int(c.samp_off[loc[nm] + 1])])
    rs = lambda nm: list(got["realign_sample"][int(c.samp_off[loc[nm]]):int(c.samp_off[loc[nm] + 1])])
    tk = lambda nm, f: list(got["task_k"][2 * int(c.samp_off[loc[nm]]) + f * c.n_samples[loc[nm]]:][:c.n_samples[loc[nm]]])
    npaths = lambda nm, f, s: len(got["paths"][2 * int(c.samp_off[loc[nm]]) + f * c.n_samples[loc[nm]] + s])
    st = lambda nm: int(got["status"][loc[nm]])
    assert [npaths("no_reads_and_short_strings", 0, s) for s in range(3)] == [1, 1, 1]
    assert rs("snp_two_reads") == [1] and len(got["opts"][loc["snp_two_reads"]][1]) == 1
    assert rs("snp_one_read_pruned") == [0] and npaths("snp_one_read_pruned", 0, 0) == 1
    assert [npaths("threshold_three", 1, s) for s in range(3)] == [1, 2, 2]              # weight 2 under a threshold of 3; weight 3; weight 2 under 2
    assert npaths("alt_source", 0, 0) == 2 and npaths("alt_sink", 1, 0) == 2 and npaths("alt_source_with_incident_edge", 0, 0) == 1
    assert tk("source_with_incident_edge", 1) == [12] and tk("cycle_at_10_not_at_12", 0) == [12]
    assert ss("cycle_at_10_not_at_12") == [fc.INDEL]
    assert tk("cycle_at_every_k", 1) == [fc.T_CYCLIC, 10] and ss("cycle_at_every_k") == [fc.CYCLIC, fc.OK]
    assert ss("indels") == [fc.INDEL, fc.INDEL, fc.OK] and rs("indels") == [0, 0, 0]
    # the order quirk of :105-130: an equal-length alternative popped after the indel sets realign_sample again
    assert ss("indel_then_equal_length") == [fc.INDEL, fc.INDEL, fc.OK] and rs("indel_then_equal_length") == [0, 1, 0]
    assert npaths("sixteen_paths", 0, 0) == 10 and {w for w, _ in got["paths"][2 * int(c.samp_off[loc["sixteen_paths"]])]} == {2}
    assert any(b"N" in p for _, p in got["paths"][2 * int(c.samp_off[loc["strings_with_n"]]) + 2])
    assert st("ref_len_10") == 1 and st("ref_len_0") == 1 and st("ref_len_11") == 0 and tk("ref_len_11", 1) == [10, 10]
    assert tk("masked_sample", 1) == [fc.T_SKIPPED, 10] and ss("masked_sample") == [fc.OK, fc.OK] and rs("masked_sample") == [0, 1]
    low = ss("low_frequency_then_skipped")
    assert low[3] == fc.LOW_FREQ and low.count(fc.OK) == 9 and tk("low_frequency_then_skipped", 1)[3] == fc.T_SKIPPED
    assert rs("low_frequency_then_skipped") == [0, 0, 0, 0, 0, 1, 1, 0, 0, 0] and [n for _, n in got["opts"][loc["low_frequency_then_skipped"]][1]] == [2]
    assert st("five_alternatives") == 2 and st("four_alternatives") == 0 and len(got["opts"][loc["four_alternatives"]][1]) == 4
    assert got["opts"][loc["four_alternatives"]][1] == sorted(got["opts"][loc["four_alternatives"]][1])       # std::map order
    assert st("too_many_haplotypes") == 3 and int(got["new_n_haps"][loc["two_left_options"]]) == 3
    l = loc["shared_pool"]
    r0, p0 = int(c.read_off[l]), int(c.pooled_off[l])
    assert list(got["copy_read"][r0:int(c.read_off[l + 1])]) == [1] * 5 + [0] * 4
    pools = got["realign_pool"][p0:int(c.pooled_off[l + 1])]
    assert pools[int(c.pool_index[r0 + 4])] == 1 and c.pool_index[r0 + 4] == c.pool_index[r0 + 5] and list(pools) == [1] * 5 + [0] * 3


def test_parameters_reach_the_graph(lib, batches):
    """max_paths, min_path_weight and the k range are the request's: 16 paths come back when asked for, a weight bound of 3 drops the
    weight-2 alternatives, and max_kmer 11 leaves the flank that needs k = 12 without an acyclic k."""
    c, _ = batches["unit"]
    loc = {L["name"]: l for l, L in enumerate(c.loci)}
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c, max_paths=16))
    assert len(got["paths"][2 * int(c.samp_off[loc["sixteen_paths"]])]) == 16
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c, min_path_weight=3))
    assert len(got["paths"][2 * int(c.samp_off[loc["snp_two_reads"]]) + 1]) == 1
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c, max_kmer=11))
    assert got["task_k"][2 * int(c.samp_off[loc["cycle_at_10_not_at_12"]])] == fc.T_CYCLIC


def test_return_3_convention(lib, batches):
    c, _ = batches["unit"]
    full = capi.run_flank(lib, trace=c.trace, **fc.args(c))
    need = full["need"]
    n_opts = sum(len(o) for L in full["opts"] for o in L)
    assert full["rc"] == 0 and n_opts > 5
    for short in ("opts", "opt_chars", "paths", "path_chars"):
        caps = dict(opts=n_opts, opt_chars=sum(len(s) for L in full["opts"] for o in L for s, _ in o), paths=sum(len(p) for p in full["paths"]),
                    path_chars=sum(len(s) for p in full["paths"] for _, s in p))
        exact = capi.run_flank(lib, trace=c.trace, caps=caps, **fc.args(c))
        assert exact["rc"] == 0, short
        want = dict(caps)
        caps[short] -= 1
        got = capi.run_flank(lib, trace=c.trace, caps=caps, **fc.args(c))
        assert got["rc"] == 3 and got["need"] == want, short
        assert np.array_equal(got["opt_off"], full["opt_off"]) and got["opt_off"][-1] == n_opts
    # without the path arrays their capacities do not matter
    got = capi.run_flank(lib, trace=c.trace, caps=dict(opts=n_opts, opt_chars=need["opt_chars"] if need["opt_chars"] else 10000, paths=0, path_chars=0),
                         want_paths=False, **fc.args(c))
    assert got["rc"] == 0 and got["opts"] == full["opts"] and np.array_equal(got["sample_status"], full["sample_status"])


def _untouched(e):
    for k, v in e.value.raw.items():
        if isinstance(v, bytes):
            assert not any(v), k
        else:
            assert np.all(v == (capi.FLANK_FILL if v.dtype == np.uint8 else capi.UNTOUCHED)), k


def refusals(run, c):
    """The refusals both entry points share: `run(**changes)` calls one of them on the unit batch."""
    def refused(word, **kw):
        with pytest.raises(RuntimeError, match=word) as e:
            run(**kw)
        _untouched(e)
    for bad in (c.n_req, -2):
        rr = c.read_req.copy(); rr[1] = bad
        refused(r"read_req outside \[-1, n_req\)", read_req=rr)
    rr = c.read_req.copy(); rr[0] = c.n_req - 1
    refused("request belongs to another locus", read_req=rr)
    q = c.req_read.copy(); q[0], q[-1] = q[-1], q[0]
    refused("grouped by locus", req_read=q)
    q = c.req_read.copy(); q[-1] = int(c.pooled_off[-1])
    refused("req_read outside the pooled reads", req_read=q)
    pi = c.pool_index.copy(); pi[2] = 1000
    refused("pool_index outside", pool_index=pi)
    other = fc.build(fc.unit_loci()[:3])
    refused("pooled->n_loci differs", bptr=C.pointer(other.pooled))
    for kw in (dict(seed=None), dict(read_req=None), dict(bptr=None), dict(pool_index=None), dict(null_out="status"), dict(null_out="copy_read"),
               dict(null_out="opt_seq")):
        refused("null argument", **kw)


def test_refusals(lib, batches):
    c, _ = batches["unit"]
    def run(**kw):
        a = fc.args(c, **kw)
        return capi.run_flank(lib, trace=a.pop("trace", c.trace), **a)
    refusals(run, c)
    with pytest.raises(RuntimeError, match="without flank_seq_off / flank_seq"):
        run(trace=dict(flank_seq_off=c.trace["flank_seq_off"]))
    with pytest.raises(RuntimeError, match="null argument"):
        run(trace=None)
    # labels that do not ascend within a locus
    lab = c.sample_label.copy(); l = [i for i, L in enumerate(c.loci) if L["name"] == "indels"][0]
    lab[c.read_off[l]] = 1
    n = c.n_reads
    pb = capi.PostBatch(np.diff(c.hap_off).astype(np.int32), c.n_samples, c.read_off, lab, np.zeros(n), np.zeros(n), np.ones(n, np.int32),
                        np.zeros(int((np.diff(c.read_off) * np.diff(c.hap_off)).sum())))
    with pytest.raises(RuntimeError, match="grouped by ascending sample label"):
        run(pb=pb)


def test_empty_inputs(lib):
    c = fc.build([])
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c))
    assert got["rc"] == 0 and len(got["status"]) == 0 and list(got["opt_off"]) == [0]
    # loci without reads and without requests
    c = fc.build([dict(name="a", ref=("ACGTTGCATGCCATGACTGACTTGA", "TTGACCATGGTACCGATTACAGGAC"), samples=[dict(reads=[]), dict(reads=[])])])
    got = capi.run_flank(lib, trace=c.trace, **fc.args(c))
    assert got["rc"] == 0 and list(got["status"]) == [0] and list(got["task_k"]) == [10] * 4 and [len(p) for p in got["paths"]] == [1] * 4
    assert all(p[0] == (2, ref.encode()) for p, ref in zip(got["paths"], [c.loci[0]["ref"][0]] * 2 + [c.loci[0]["ref"][1]] * 2))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/cpp/flank_host_test.cpp with the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
    exe = str(tmp_path_factory.mktemp("flank") / "flank_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "flank_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "flank_host.cpp")], check=True)
    return exe


def test_sanitized_program_self_test(program):
    r = subprocess.run([program, "self"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout


@pytest.mark.parametrize("name", sorted(fc.BATCHES))
def test_sanitized_program_on_the_goldens(program, name, tmp_path):
    """Host twin == reference records, and (inside the program) the device's task body == host twin, on the golden's own case text."""
    text, records = fc.golden(name)
    src, dst = str(tmp_path / "cases.txt"), str(tmp_path / "records.txt")
    with open(src, "w") as f:
        f.write(text)
    r = subprocess.run([program, "cases", src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    with open(dst) as f:
        assert fc.parse_records(f.read()) == records
