"""CPU: the chain of INTEGRATION.md §2a — pool, read x haplotype matrix, posteriors, read assignment, tracebacks, allele census, remap, partial
realignment, EM retraining — run END TO END by tests/flow_chain.py on the HOST backend (hipstr_pool_reads_host, the oracle's process_reads /
posteriors / trace / em_train, and the numpy restatements of the stage tests), all twelve loci as one ragged batch, against the reference's
own final state: tests/golden/flow_<case>.txt.gz, written by the compiled reference's genotype() from the inputs in
tests/golden/flowin_<case>.txt.gz (the same run's --dump-inputs).  Bars: test_genotype_flow._compare's, unchanged — counts, blocks, pools,
pool qualities, mates, seeds, MAP haplotypes, every field of every cached traceback and the bit patterns of log_aln_probs identical,
posteriors and sample totals to 1e-9; after --recompute the stutter model and log_aln_probs to 1e-9.

This proves the driver's own bookkeeping (new blocks, allele_mapping, realign_to_haplotype, the trace cache, the phases of genotype()) before
a device is involved: tests/test_flow_chain_gpu.py runs the same driver on the device backend.

Every case runs with --no-flanks: assemble_flanks (seq_stutter_genotyper.cpp:40-217) is De Bruijn assembly on the host and out of scope."""
import os

import numpy as np
import pytest

import flow_chain as fc

NAMES = list(fc.CASES)
LARGEST_FLOW_FIXTURE = 61051           # tests/golden/flow_s1p3_recompute.txt.gz, the largest before these


def test_fixtures_cover_the_rounds():
    """From the fixtures, not from the code under test: what the reference's rounds did to the twelve loci."""
    w = {n: fc.what_the_rounds_do(n) for n in NAMES}
    assert len(w) == 12
    assert sum(x["added"] > 0 for x in w.values()) >= 4
    assert sum(x["uncalled"] > 0 for x in w.values()) >= 3
    assert sum(x["unspanned"] > 0 for x in w.values()) >= 1
    assert sum(x["added"] > 0 and x["uncalled"] + x["unspanned"] > 0 for x in w.values()) >= 2
    assert {x["period"] for x in w.values()} == {1, 2, 3, 4, 5, 6}
    assert w["s4p3_noflank"]["added"] == w["s4p3_noflank"]["uncalled"] == w["s4p3_noflank"]["unspanned"] == 0           # the control
    assert sum("--recompute" in a for a in fc.CASES.values()) == 1 and all("--no-flanks" in a for a in fc.CASES.values())
    pools = [(len([l for l in fc.gold(n).splitlines() if l.startswith("pool_qual ")]), fc.Inputs(n).n_reads) for n in NAMES]
    assert any(p < r for p, r in pools) and any(p == r for p, r in pools)          # pooled loci, and one in which every read is its own pool
    assert any(sum(fc.Inputs(n).second_mate) > 0 for n in NAMES)


def test_fixtures_are_small_and_hold_data_only():
    for n in NAMES:
        for kind in ("flow", "flowin"):
            assert os.path.getsize(os.path.join(fc.GOLD, "%s_%s.txt.gz" % (kind, n))) <= LARGEST_FLOW_FIXTURE, (kind, n)
        keys = {l.split(" ")[0] for l in fc._read_gz("flowin", n).splitlines()}
        assert keys == {"region", "initialized", "num_samples", "num_reads", "block", "repeat_block", "stutter_model", "read"}


@pytest.fixture(scope="module")
def host_chain(hmm_host, oracle):
    recs = []
    out = fc.run(NAMES, fc.HostBackend(hmm_host, oracle), oracle, recs)
    return out, recs


def actions(rec):
    """Per locus what a round did to it: "add", "remove" or "idle" (identity mapping)."""
    out = []; o = 0
    for a, na in zip(rec["n_alleles"], rec["new_n_alleles"]):
        m = rec["mapping"][o:o + a]; o += a
        out.append("add" if na > a else "remove" if np.any(m == -1) else "idle")
        assert out[-1] != "idle" or (na == a and np.array_equal(m, np.arange(a)))
    return out


def test_the_batch_is_ragged(host_chain):
    """Loci leave the add loop at different rounds: in one round some add alleles, some remove alleles and some idle with the identity
    mapping; loci that added in round 1 remove in round 2 while the others idle; the second pass of the --recompute locus is a batch of one."""
    _, recs = host_chain
    rounds = [actions(r) for r in recs if "mapping" in r]
    first = [a for a in rounds if len(a) == 12]; second = [a for a in rounds if len(a) == 1]
    assert len(first) >= 3 and len(second) >= 2 and len(first) + len(second) == len(rounds)
    assert {"add", "remove", "idle"} == set(first[0])
    assert any(first[0][l] == "add" and first[1][l] == "remove" for l in range(12)) and first[1].count("idle") >= 6
    assert any(first[0][l] == "remove" and first[1][l] == "idle" for l in range(12))
    assert set(first[-1]) == {"idle"}                                  # the round in which the last locus finds nothing more to do
    assert [a[0] for a in second][:2] == ["add", "remove"]
    assert sum("em_stutter" in r for r in recs) == 1


def test_new_columns_hold_the_fill_until_they_are_aligned(host_chain):
    """seq_stutter_genotyper.cpp:374: after a remap every new column holds -100000 in every row and no kept column does; after the scatter
    that follows, none is left — every read is copied in a --no-flanks round, so the final state alone cannot show the fill."""
    _, recs = host_chain
    rounds = [r for r in recs if "mapping" in r]
    assert all(fc.fill_after_remap(r)[1] for r in rounds) and sum(fc.fill_after_remap(r)[0] for r in rounds) >= 10
    assert not any(np.any(r["matrix_after_scatter"] == fc.UNALIGNED) for r in recs if "matrix_after_scatter" in r)


@pytest.mark.parametrize("name", NAMES)
def test_host_chain_reproduces_the_reference(host_chain, name):
    fc.against_gold(host_chain[0][name], name)


def test_one_locus_per_batch_gives_the_same(host_chain, hmm_host, oracle):
    for n in NAMES:
        one = fc.run([n], fc.HostBackend(hmm_host, oracle), oracle)
        assert one[n] == host_chain[0][n], n


def test_new_alleles_are_ordered_by_length_then_sequence(oracle):
    """id_and_align_to_stutter_alleles sorts a block's candidates with orderByLengthAndSequence (:582, stringops.cpp:35-39) before
    add_alternate appends them (:345-350).  The simulated loci are pure repeats — a shorter candidate is a prefix of a longer one, so both
    orders agree in every fixture — hence this hand-made step: candidates in std::set order (by string), as :872 hands them over."""
    s = fc.State(fc.Inputs("s4p3_noflank"), oracle)
    old = s.hap_seqs(); n1 = s.nopts[1]; A = s.A
    cand = [b"AAAAAA", b"CC", b"CG", b"T"]
    assert cand == sorted(cand)
    m, r, added = s.step(cand, None, None, A // n1 * (n1 + 4))
    assert added and s.phase == fc.ADD
    assert s.blocks[1][2][n1:] == ["T", "CC", "CG", "AAAAAA"] and s.blocks[1][2][:n1] == fc.Inputs("s4p3_noflank").blocks[1][2]
    new = s.hap_seqs()
    assert len(new) == A // n1 * (n1 + 4) and [new[j] for j in m] == old           # allele_mapping: every old haplotype, by its string (:358-367)
    assert [new[j] not in old for j in range(len(new))] == r and sum(r) == 4 * A // n1
