"""CPU: genotype() for the twelve --no-flanks loci as one batch and for the six flank loci as one batch (tests/golden/flow_*.txt.gz) with the
bookkeeping between the rounds done by hipstr_alleles_step / hipstr_alleles_apply (tests/flow_chain_step.py) on the host backends — under
against_gold's bars, and bit for bit against the unmodified drivers' per-round records (tests/flow_chain.py, tests/flow_chain_flanks.py)."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
import flow_chain_flanks as ff
import flow_chain_step as fs
from test_flow_chain_gpu import ROUND_KEYS, same_rounds
from test_flow_chain_flanks_gpu import FLANK_KEYS

NAMES, FLANK_NAMES = list(fc.CASES), list(ff.CASES)


def rounds_do(recs, names):
    """n_added / n_removed summed over the rounds, per locus of the first pass and of the --recompute pass"""
    n = {x: dict(added=0, removed=0) for x in names}; live = list(names)
    for r in recs:
        if "em_stutter" in r:
            live = [x for x in names if "--recompute" in fc.CASES.get(x, [])]
        if "n_added" in r:
            for l, x in enumerate(live):
                n[x]["added"] += int(r["n_added"][l]); n[x]["removed"] += int(r["n_removed"][l])
    return n


def same_flank_rounds(got, want, what):
    same_rounds(got, want, ROUND_KEYS, what)
    g = [r for r in got if "flank_status" in r]; w = [r for r in want if "flank_status" in r]
    assert len(g) == len(w) == 1
    for k in FLANK_KEYS:
        assert repr(g[0][k]) == repr(w[0][k]) if isinstance(g[0][k], list) else np.array_equal(np.asarray(g[0][k]), np.asarray(w[0][k])), (what, k)


@pytest.fixture(scope="module")
def plain(hmm_host, oracle):
    recs = []
    return fc.run(NAMES, fc.HostBackend(hmm_host, oracle), oracle, recs), recs


@pytest.fixture(scope="module")
def stepped(hmm_host, oracle):
    recs = []
    return fs.run(NAMES, fc.HostBackend(hmm_host, oracle), oracle, hmm_host, True, recs), recs


@pytest.mark.parametrize("name", NAMES)
def test_stepped_chain_reproduces_the_reference(stepped, name):
    fc.against_gold(stepped[0][name], name)


def test_stepped_chain_equals_the_caller_side_bookkeeping(stepped, plain):
    for n in NAMES:
        assert stepped[0][n] == plain[0][n], n
    same_rounds(stepped[1], plain[1], ROUND_KEYS, "hipstr_alleles_step against State.step")


def test_counts_are_the_reference_log_lines(stepped):
    got = rounds_do(stepped[1], NAMES)
    for n in NAMES:
        w = fc.what_the_rounds_do(n)
        assert got[n]["added"] == w["added"] and got[n]["removed"] == w["uncalled"] + w["unspanned"], (n, got[n], w)


@pytest.fixture(scope="module")
def flank_plain(hmm_host, oracle):
    recs = []
    return ff.run(FLANK_NAMES, ff.HostBackend(hmm_host, oracle), oracle, recs), recs


@pytest.fixture(scope="module")
def flank_stepped(hmm_host, oracle):
    recs = []
    return fs.run_flanks(FLANK_NAMES, ff.HostBackend(hmm_host, oracle), oracle, hmm_host, True, recs), recs


@pytest.mark.parametrize("name", FLANK_NAMES)
def test_stepped_chain_with_flanks_reproduces_the_reference(flank_stepped, name):
    ff.against_gold(flank_stepped[0][name], name)


def test_stepped_flank_chain_equals_the_caller_side_bookkeeping(flank_stepped, flank_plain):
    for n in FLANK_NAMES:
        assert flank_stepped[0][n] == flank_plain[0][n], n
    same_flank_rounds(flank_stepped[1], flank_plain[1], "hipstr_alleles_apply against State.apply")
