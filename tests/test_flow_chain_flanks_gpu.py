"""GPU: the resident chain of INTEGRATION.md §2a with the flank step — ... -> hipstr_post_assign(RETRACE) -> hipstr_hmm_trace_resident ->
hipstr_flank_assemble_dev -> hipstr_rm_remap -> align only the marked pools against the new haplotypes -> hipstr_rm_scatter(copy_read) ->
posteriors -> the census's `called` marks with sample_uncallable -> removal -> posteriors — by tests/flow_chain_flanks.py on its device
backend, the six flank cases as one batch.  Yardsticks: the reference's own final state (tests/golden/flow_<case>.txt.gz, flanks on) under
flow_chain.against_gold's bars, and the same driver on the host backend with the oracle under capi.oracle_cr_math: the final state and every
intermediate of the flank step bit for bit."""
import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain_flanks as ff
from test_flow_chain_gpu import ROUND_KEYS, same_rounds

pytestmark = pytest.mark.gpu
NAMES = list(ff.CASES)
FLANK_KEYS = ("flank_status", "flank_new_n_haps", "flank_opts", "flank_sample_status", "flank_realign_sample", "flank_realign_pool", "flank_copy_read",
              "flank_task_k", "flank_paths", "flank_called", "flank_mapping", "flank_n_req", "flank_req_read", "flank_req_allele")


@pytest.fixture(scope="module")
def host(hmm_host, oracle):
    recs = []
    with capi.oracle_cr_math(oracle):
        out = ff.run(NAMES, ff.HostBackend(hmm_host, oracle), oracle, recs)
    return out, recs


@pytest.fixture(scope="module")
def device(hmm, oracle):
    be = ff.DeviceBackend(hmm); recs = []
    try:
        out = ff.run(NAMES, be, oracle, recs)
        last = capi.flank_last(hmm)
    finally:
        be.close()
    return out, recs, last


@pytest.mark.parametrize("name", NAMES)
def test_resident_chain_with_flanks_reproduces_the_reference(device, name):
    ff.against_gold(device[0][name], name)


def test_device_equals_host_bit_for_bit(device, host):
    for n in NAMES:
        assert device[0][n] == host[0][n], n
    same_rounds(device[1], host[1], ROUND_KEYS, "device against host")
    d = [r for r in device[1] if "flank_status" in r]; h = [r for r in host[1] if "flank_status" in r]
    assert len(d) == len(h) == 1
    for k in FLANK_KEYS:
        assert repr(d[0][k]) == repr(h[0][k]) if isinstance(d[0][k], list) else np.array_equal(np.asarray(d[0][k]), np.asarray(h[0][k])), k


def test_no_task_of_the_flow_cases_leaves_the_device(device):
    last = device[2]
    assert last["tasks"] == 2 * (5 * 10 + 24) and last["host_tasks"] == 0 and not last["fetched_strings"]
