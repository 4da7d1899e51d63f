"""GPU: the resident chain of INTEGRATION.md §2a with the trace cache in it (tests/flow_chain_cache.py: hipstr_trace_cache_round for
hipstr_hmm_trace_resident, hipstr_trace_cache_remap beside hipstr_rm_remap, a fresh cache for the second pass), all twelve loci of
tests/flow_chain.py as ONE batch.

Yardsticks: (1) the reference's own final state, tests/golden/flow_<case>.txt.gz, under test_genotype_flow._compare's bars — including
every field of every cached traceback; (2) the cache's own final state: the dump's `trace` lines taken from hipstr_trace_cache_entries /
_view instead of the driver's dictionary must be the same lines; (3) the plain DeviceBackend run of the same commit: every per-round
intermediate bit for bit — a cached record is the record of the round that first asked for it, which the uncached chain retraces; on these
fixtures the two agree in every field; (4) the misses per trace call: the dictionary restatement of the reference's cache
(flow_chain.State.cache) counted by the HOST backend on the CPU (flow_chain_cache.CountingHostBackend); where every locus takes its
records that restatement gives the reference's own 1826 / 32 / 0 / 0 of 4 x 1826 requests in the first pass.

No GPU test reads the reference tree or oracle/_ref: inputs and expectations are the committed fixtures."""
import pytest

from hipstr_amd import capi
import flow_chain as fc
import flow_chain_cache as fcc
from test_flow_chain_gpu import NAMES, ROUND_KEYS, same_rounds

pytestmark = pytest.mark.gpu
FIRST_PASS = [1826, 32, 0, 0]          # the reference's misses in the first pass' trace calls (three rounds and the EM's retrace), of 1826 requests each


@pytest.fixture(scope="module")
def cached(hmm, oracle):
    be = fcc.CachedDeviceBackend(hmm); recs = []
    try:
        out = fc.run(NAMES, be, oracle, recs)
        return out, recs, be.calls, be.finals
    finally:
        be.close()


@pytest.fixture(scope="module")
def plain(hmm, oracle):
    be = fc.DeviceBackend(hmm); recs = []
    try:
        return fc.run(NAMES, be, oracle, recs), recs
    finally:
        be.close()


@pytest.fixture(scope="module")
def restated(hmm_host, oracle):
    """The host backend with the dictionary restatement counting: no device.  (requests, misses, misses if every locus took) per trace call."""
    be = fcc.CountingHostBackend(hmm_host, oracle)
    with capi.oracle_cr_math(oracle):
        fc.run(NAMES, be, oracle, None)
    return be.calls


@pytest.mark.parametrize("name", NAMES)
def test_cached_chain_reproduces_the_reference(cached, name):
    fc.against_gold(cached[0][name], name)


def test_the_caches_own_state_gives_the_same_trace_lines(cached):
    out, _, _, finals = cached
    assert len(finals) == 2
    again = [n for n in NAMES if "--recompute" in fc.CASES[n]]
    first = [n for n in NAMES if n not in again]
    n_lines = 0
    for names, fin, where in ((first, finals[0], NAMES), (again, finals[1], again)):
        for n in names:
            want = [x for x in out[n].splitlines() if x.startswith("trace ")]
            got = fcc.trace_lines(fin, where.index(n))
            assert got == want, n
            n_lines += len(got)
    assert n_lines > 1000


def test_cached_equals_uncached_bit_for_bit(cached, plain):
    for n in NAMES:
        assert cached[0][n] == plain[0][n], n
    same_rounds(cached[1], plain[1], ROUND_KEYS, "cached against uncached")
    assert sum("em_stutter" in r for r in cached[1]) == 1


def test_the_misses_are_the_restatements(cached, restated):
    """Equality with the restatement, call by call.  The first pass: a cache in which every locus takes its records misses the reference's
    1826 / 32 / 0 / 0; with locus_takes from the phases a DONE locus takes nothing and misses its few new keys again in the later calls
    (the restatement's second column says how many); the total stays strictly below half of the 7304 requests."""
    calls = cached[2]
    assert [(n, m) for n, m, _ in calls] == [(n, m) for n, m, _ in restated]       # the same request counts, the same expected misses
    for n, want, st in calls:
        assert st["n_misses"] == want and st["n_hits"] == n - want, (n, want, st)
    first = restated[:len(FIRST_PASS)]
    assert [n for n, _, _ in first] == [1826] * 4 and [e for _, _, e in first] == FIRST_PASS
    assert 2 * sum(st["n_misses"] for _, _, st in calls[:4]) < 7304
    assert 2 * sum(st["n_misses"] for _, _, st in calls) < sum(n for n, _, _ in calls)
    assert calls[3][2]["n_inserted"] == 0                               # the EM's retrace: every locus is done, nothing is taken
