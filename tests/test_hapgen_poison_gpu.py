"""GPU: hipstr_hapgen on poisoned cache blocks (hipstr_debug_cache_poison), tests/test_poison_gpu.py's protocol: warm once, then under every
poison byte no new driver allocation and identical results — the stage reads no word of a recycled device or pinned block that the same
call did not write."""
import numpy as np
import pytest

from hipstr_amd import capi
import hapgen_cases as hc

pytestmark = pytest.mark.gpu
PATTERNS = (0xFF, 0x7F, 0x80, 0x00)


def test_poisoned_caches(hmm):
    loci = []
    for name in sorted(hc.BATCHES):
        loci += hc.load_golden(name)[0]
    loci += hc.no_flagged_loci()
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    want = hc.expectation(loci)
    hmm.hipstr_hmm_trim()
    def run():
        got = capi.run_hapgen(hmm, b.ptr, rq)
        last = capi.hapgen_last(hmm)
        assert last["collision_loci"] == 0 and last["host_loci"] == 0 and last["device_loci"] == len(loci), last
        return got
    run()
    allocs = hmm.hipstr_debug_driver_allocs()
    out = []
    for pat in PATTERNS:
        assert hmm.hipstr_debug_cache_poison(pat) > 0, hmm.hipstr_last_error().decode()
        out.append(run())
    assert hmm.hipstr_debug_driver_allocs() == allocs
    for pat, r in zip(PATTERNS, out):
        hc.assert_same(r, out[0], "poison 0x%02X" % pat)
    hc.assert_result(out[0], want, "poisoned")
    hc.assert_same(out[0], capi.run_hapgen(hmm, b.ptr, rq, host=True), "poisoned, device against host twin")
