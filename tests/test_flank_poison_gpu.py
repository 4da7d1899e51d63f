"""GPU: the flank stage (hipstr_flank_assemble_dev) on poisoned cache blocks — the protocol and the hook of tests/test_poison_gpu.py
(hipstr_debug_cache_poison): the caches never clear a block, so a kernel that reads a word of its workspace it did not write gets whatever
the block held before; results that change with the poison byte show the read.  Both routes: every task on the device, and part of them
through the host twin (shrunk caps).  In steady state the call takes no block from the driver."""
import numpy as np
import pytest

from hipstr_amd import capi
import flank_cases as fc
import test_flank_gpu as tfg
import test_poison_gpu as tp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("caps", [None, dict(edges=24, recs=40)], ids=["device", "host_twin_for_some"])
def test_flank_stage_on_poisoned_cache_blocks(hmm, caps):
    hmm.hipstr_hmm_trim()
    c = fc.build(fc.unit_loci())
    what = "hipstr_flank_assemble_dev, caps %s" % caps
    with tfg.Resident(hmm, c) as R, tfg.caps_env(caps):
        def run():
            raw = R.run()["raw"]
            return {k: (np.frombuffer(v, np.uint8) if isinstance(v, bytes) else v) for k, v in raw.items()}
        out = tp.poisoned(hmm, run, what)
        tp.same_bits(run(), out[0], what + ", unpoisoned against poisoned")
        assert (capi.flank_last(hmm)["host_tasks"] > 0) == (caps is not None)
        allocs = hmm.hipstr_debug_driver_allocs()
        run(); run()
        assert hmm.hipstr_debug_driver_allocs() == allocs, what
