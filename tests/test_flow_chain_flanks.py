"""CPU: genotype() WITH its last statement — assemble_flanks (seq_stutter_genotyper.cpp:40-217) on hipstr_flank_assemble — run end to end by
tests/flow_chain_flanks.py on the host backend, the six flank cases of tests/test_genotype_flow.py as one batch, against the reference's own
final state: their existing goldens tests/golden/flow_<case>.txt.gz (runs of the compiled reference with flanks on), from the same runs'
inputs tests/golden/flowin_<case>.txt.gz.  Bars: flow_chain.against_gold's, unchanged.  The final state holds the new flank options (the
blocks), the matrix with its -100000 where copy_read was false, the seeds, the posteriors and the traces get_unused_alleles cached after the
realignment: wrong masks, options or option order show there."""
import os
import re

import pytest

import flow_chain as fch
import flow_chain_flanks as ff

NAMES = list(ff.CASES)


def test_fixtures_cover_the_stage():
    """From the fixtures alone: every case gained a flank haplotype, and the fill survives somewhere: a subset of the reads was copied."""
    some_partial = 0
    for n in NAMES:
        g = fch.gold(n); inp = ff.Inputs(n)
        logs = "\n".join(l for l in g.splitlines() if l.startswith("log "))
        assert re.search(r"Identified \d+ new (left|right) flank haplotype", logs), n
        some_partial += "c0f86a0000000000" in [l for l in g.splitlines() if l.startswith("log_aln_probs")][0]      # -100000 survives where copy_read was false
        final = [l.split(" ") for l in g.splitlines() if l.startswith("block ")]
        assert sum(int(w[4]) for w in final if w[1] in ("0", "2")) > 2 and [len(b[2]) for b in inp.blocks][::2] == [1, 1], n
        assert os.path.getsize(os.path.join(fch.GOLD, "flowin_%s.txt.gz" % n)) <= 61051
        keys = {l.split(" ")[0] for l in fch._read_gz("flowin", n).splitlines()}
        assert keys == {"region", "initialized", "num_samples", "num_reads", "block", "repeat_block", "stutter_model", "read"}
    assert some_partial >= 1


@pytest.fixture(scope="module")
def host_chain(hmm_host, oracle):
    recs = []
    out = ff.run(NAMES, ff.HostBackend(hmm_host, oracle), oracle, recs)
    return out, recs


@pytest.mark.parametrize("name", NAMES)
def test_host_chain_with_flanks_reproduces_the_reference(host_chain, name):
    ff.against_gold(host_chain[0][name], name)


def test_what_the_stage_did(host_chain):
    rec = [r for r in host_chain[1] if "flank_status" in r]
    assert len(rec) == 1
    r = rec[0]
    assert not r["flank_status"].any() and all(len(L[0]) + len(L[1]) >= 1 for L in r["flank_opts"])
    assert 0 < r["flank_realign_sample"].sum() < len(r["flank_realign_sample"])            # some samples realign, some keep their rows
    assert 0 < r["flank_copy_read"].sum() < len(r["flank_copy_read"]) and 0 < r["flank_realign_pool"].sum() < len(r["flank_realign_pool"])
    assert (r["flank_task_k"] >= 10).all() and max(len(p) for p in r["flank_paths"]) >= 2
    assert "flank_called" in r and len(r["flank_mapping"]) > 0
