"""GPU: the resident chain of INTEGRATION.md §2a executed as a whole —

  hipstr_pool_batch -> hipstr_rm_create -> upload / align -> hipstr_rm_scatter -> hipstr_post_upload / launch -> hipstr_post_assign(RETRACE)
  -> hipstr_hmm_trace_resident -> hipstr_post_census_dev -> hipstr_rm_remap -> align only the new haplotypes -> hipstr_rm_scatter(copy_read)
  -> ... -> hipstr_em_train_dev

— by tests/flow_chain.py's driver of genotype() on its device backend: exactly those calls in that order, nothing synchronised between them,
the matrix, the posteriors and the trace records never fetched between the rounds (only the seeds once, the assign request list, the census
outputs and the EM result cross to the host), everything else fetched once at the end.  All twelve loci of the table run as ONE ragged
batch: loci leave the add loop at different rounds and idle with the identity mapping.

Yardsticks: (1) the reference's own final state, tests/golden/flow_<case>.txt.gz, under test_genotype_flow._compare's bars (counts, blocks,
pools, pool qualities, mates, seeds, MAP haplotypes, every field of every cached traceback and log_aln_probs' bit patterns identical;
posteriors and totals 1e-9; the --recompute case: stutter model and log_aln_probs 1e-9); (2) the same driver on the host backend
(tests/test_flow_chain.py proves that one against the goldens without a device) with the oracle under capi.oracle_cr_math: every one of
those and every per-round intermediate bit for bit.

Every case runs with --no-flanks: assemble_flanks (seq_stutter_genotyper.cpp:40-217) is De Bruijn assembly on the host and out of scope.
No GPU test reads the reference tree or oracle/_ref: inputs and expectations are the committed fixtures."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain as fc
from test_poison_gpu import same_bits

pytestmark = pytest.mark.gpu
NAMES = list(fc.CASES)
ROUND_KEYS = ("n_alleles", "cand", "called", "spanned", "new_n_haps", "n_req", "req_read", "req_allele", "read_req", "mapping", "new_n_alleles",
              "em_trained", "em_stutter")
MATRIX_KEYS = ("matrix_after_remap", "matrix_after_scatter")


def device_run(hmm, oracle, names=NAMES, **kw):
    be = fc.DeviceBackend(hmm, **kw); recs = []
    try:
        return fc.run(names, be, oracle, recs), recs
    finally:
        be.close()


@pytest.fixture(scope="module")
def host(hmm_host, oracle):
    """The host backend with the oracle's exp / log those of the device (cr_math.h): computed once, never changed."""
    recs = []
    with capi.oracle_cr_math(oracle):
        out = fc.run(NAMES, fc.HostBackend(hmm_host, oracle), oracle, recs)
    return out, recs


@pytest.fixture(scope="module")
def device(hmm, oracle):
    """The first pass: no fetch between the rounds."""
    return device_run(hmm, oracle)


@pytest.mark.parametrize("name", NAMES)
def test_resident_chain_reproduces_the_reference(device, name):
    fc.against_gold(device[0][name], name)


def same_rounds(got, want, keys, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        ks = [k for k in keys if k in w]
        assert ks == [k for k in keys if k in g], "%s round %d" % (what, i)
        for k in ks:
            same_bits(list(g[k]) if k == "cand" else (g[k] if isinstance(g[k], int) else np.asarray(g[k])),
                      list(w[k]) if k == "cand" else (w[k] if isinstance(w[k], int) else np.asarray(w[k])), "%s round %d %s" % (what, i, k))


def test_device_equals_host_bit_for_bit(device, host):
    """The final state (the dump prints posteriors with 17 digits: equal text = equal bits) and, round by round, the candidates, the called /
    spanned marks, new_n_haps, the request lists, the mappings and the EM's model."""
    for n in NAMES:
        assert device[0][n] == host[0][n], n
    same_rounds(device[1], host[1], ROUND_KEYS, "device against host")
    assert sum("em_stutter" in r for r in device[1]) == 1 and sum("cand" in r for r in device[1]) >= 5


def test_the_matrix_after_every_remap_and_scatter(hmm, oracle, device, host):
    """A second, diagnostic pass that fetches the matrix after each remap and each scatter: the bits of the host backend's, and the fetches
    change nothing downstream."""
    out, recs = device_run(hmm, oracle, diag=True)
    assert out == device[0]
    same_rounds(recs, host[1], MATRIX_KEYS, "matrix")
    assert sum(k in r for r in recs for k in MATRIX_KEYS) >= 2 * sum("mapping" in r for r in recs)
    rounds = [r for r in recs if "mapping" in r]
    assert all(fc.fill_after_remap(r)[1] for r in rounds) and sum(fc.fill_after_remap(r)[0] for r in rounds) >= 10      # :374
    assert not any(np.any(r["matrix_after_scatter"] == fc.UNALIGNED) for r in recs if "matrix_after_scatter" in r)


def test_pooling_on_the_host_changes_nothing(hmm, oracle, device):
    out, recs = device_run(hmm, oracle, pool_flags=capi.POOL_ON_HOST)
    assert out == device[0]
    same_rounds(recs, device[1], ROUND_KEYS, "HIPSTR_POOL_ON_HOST")


def test_a_second_run_takes_nothing_from_the_driver(hmm, oracle, device):
    out, _ = device_run(hmm, oracle)
    allocs = hmm.hipstr_debug_driver_allocs()
    again, recs = device_run(hmm, oracle)
    assert hmm.hipstr_debug_driver_allocs() == allocs
    assert out == device[0] and again == device[0]
    same_rounds(recs, device[1], ROUND_KEYS, "second run")


def test_on_poisoned_cache_blocks(hmm, oracle, device):
    """tests/test_poison_gpu.py's protocol for the chain as a whole: every free block of the caches filled with 0xFF (the runs before were the
    warm-up), the same result, and no block fresh from the driver."""
    device_run(hmm, oracle)
    allocs = hmm.hipstr_debug_driver_allocs()
    assert hmm.hipstr_debug_cache_poison(0xFF) > 0, hmm.hipstr_last_error().decode()
    out, recs = device_run(hmm, oracle)
    assert hmm.hipstr_debug_driver_allocs() == allocs
    assert out == device[0]
    same_rounds(recs, device[1], ROUND_KEYS, "poisoned")


def test_one_locus_per_batch_gives_the_same(hmm, oracle, device):
    for n in NAMES:
        out, _ = device_run(hmm, oracle, names=[n])
        assert out[n] == device[0][n], n
