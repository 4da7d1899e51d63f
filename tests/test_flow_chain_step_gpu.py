"""GPU: the resident genotype() chain of INTEGRATION.md §2a with hipstr_alleles_step / hipstr_alleles_apply on the device between the rounds
(tests/flow_chain_step.py on flow_chain's and flow_chain_flanks' DeviceBackend): the twelve --no-flanks loci as one batch and the six flank
loci as one batch against tests/golden/flow_*.txt.gz under against_gold's bars, and bit for bit — the final state and every round's
records — against the unmodified drivers on the same backend."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
import flow_chain_flanks as ff
import flow_chain_step as fs
from test_flow_chain_gpu import ROUND_KEYS, same_rounds
from test_flow_chain_step import FLANK_NAMES, NAMES, rounds_do, same_flank_rounds

pytestmark = pytest.mark.gpu


def on_device(make, run, *args):
    be = make(); recs = []
    try:
        return run(*((args[0], be) + args[1:] + (recs,))), recs
    finally:
        be.close()


@pytest.fixture(scope="module")
def plain(hmm, oracle):
    return on_device(lambda: fc.DeviceBackend(hmm), fc.run, NAMES, oracle)


@pytest.fixture(scope="module")
def stepped(hmm, oracle):
    capi._alleles_sigs(hmm)
    out = on_device(lambda: fc.DeviceBackend(hmm), fs.run, NAMES, oracle, hmm, False)
    return out + (capi.alleles_last(hmm),)


@pytest.mark.parametrize("name", NAMES)
def test_stepped_resident_chain_reproduces_the_reference(stepped, name):
    fc.against_gold(stepped[0][name], name)


def test_stepped_chain_equals_the_caller_side_bookkeeping(stepped, plain):
    for n in NAMES:
        assert stepped[0][n] == plain[0][n], n
    same_rounds(stepped[1], plain[1], ROUND_KEYS, "hipstr_alleles_step against State.step")
    assert stepped[2]["host_loci"] == 0                               # no locus of the flow cases is beyond a limit of the kernel


def test_counts_are_the_reference_log_lines(stepped):
    got = rounds_do(stepped[1], NAMES)
    for n in NAMES:
        w = fc.what_the_rounds_do(n)
        assert got[n]["added"] == w["added"] and got[n]["removed"] == w["uncalled"] + w["unspanned"], (n, got[n], w)


@pytest.fixture(scope="module")
def flank_plain(hmm, oracle):
    return on_device(lambda: ff.DeviceBackend(hmm), ff.run, FLANK_NAMES, oracle)


@pytest.fixture(scope="module")
def flank_stepped(hmm, oracle):
    return on_device(lambda: ff.DeviceBackend(hmm), fs.run_flanks, FLANK_NAMES, oracle, hmm, False)


@pytest.mark.parametrize("name", FLANK_NAMES)
def test_stepped_chain_with_flanks_reproduces_the_reference(flank_stepped, name):
    ff.against_gold(flank_stepped[0][name], name)


def test_stepped_flank_chain_equals_the_caller_side_bookkeeping(flank_stepped, flank_plain):
    for n in FLANK_NAMES:
        assert flank_stepped[0][n] == flank_plain[0][n], n
    same_flank_rounds(flank_stepped[1], flank_plain[1], "hipstr_alleles_apply against State.apply")
