"""GPU: hipstr_hapgen / hipstr_hapgen_batch on the device (hipstr_amd/csrc/hapgen.hip) against the records of the reference's own
HaplotypeGenerator (tests/golden/hapgen_*.npz), the python restatement (tests/hapgen_cases.py) and the host twin — bit for bit in every
output, dist_frac included, and untouched behind what the call writes.  Sizes are the smallest at which a decision of
hipstr_amd/csrc/hapgen_layout.h flips, read from the plan.  In every case that does not force a collision the count of loci redone after one
must be 0: a broken hash must not hide behind the fallback."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hipstr_amd import capi
import flow_chain_hapgen as fh
import hapgen_cases as hc
from test_flow_chain_hapgen import check_blocks, check_batch, restated
from test_readmat_gpu import upload_and_align, same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = sorted(hc.BATCHES)


@pytest.fixture(scope="module")
def T(hmm):
    return capi.hapgen_plan(hmm, hc.ReadsBatch([]).ptr, hc.request_of([]))["thresholds"]


def on_device(hmm, b, rq, collisions=0, **kw):
    got = capi.run_hapgen(hmm, b.ptr, rq, **kw)
    last = capi.hapgen_last(hmm)
    assert (last["collision_loci"] > 0) == bool(collisions), last
    return got, last


@pytest.mark.parametrize("name", BATCHES)
def test_golden_batches(hmm, name):
    loci, recs = hc.load_golden(name)
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    got, last = on_device(hmm, b, rq)
    for l, lc in enumerate(loci):
        r = recs[lc["name"]]
        assert int(got["status"][l]) == r["status"] and hc.blocks_of(got, l) == (r["blocks"] or [(0, 0, [])] * 3), lc["name"]
    hc.assert_same(got, capi.run_hapgen(hmm, b.ptr, rq, host=True), "device against host twin")
    hc.assert_result(got, hc.expectation(loci), name)
    assert last["device_loci"] == len(loci) and last["host_loci"] == 0 and last["chunks"] == 1
    assert last["reads_uploaded"] == sum(len(lc["reads"]) for lc in loci)
    # without the optional outputs
    bare, _ = on_device(hmm, b, rq, skip=capi.HAPGEN_OPTIONAL)
    hc.assert_result(bare, hc.expectation(loci), name + " without the optional outputs")


def test_the_caps_edges(hmm, T):
    """One locus of cap - 1, cap and cap + 1 short reads; cap and cap + 1 distinct strings (found on the device, redone by the host)."""
    cap, dcap = T["HS_HAPGEN_LDS_READS"], T["HS_HAPGEN_MAX_DISTINCT"]
    rng = np.random.default_rng(5)
    for n in (cap - 1, cap, cap + 1):
        lc = hc.cap_locus(rng, n, n_samples=3, n_alleles=6)
        b = hc.ReadsBatch([lc]); rq = hc.request_of([lc])
        got, last = on_device(hmm, b, rq)
        hc.assert_same(got, capi.run_hapgen(hmm, b.ptr, rq, host=True), "%d reads" % n)
        assert (last["device_loci"], last["host_loci"], last["reads_uploaded"]) == ((1, 0, n) if n <= cap else (0, 1, 0)), (n, last)
        assert int(got["n_spanning"][0]) == n and int(got["n_distinct"][0]) == 6
    for nd in (dcap, dcap + 1):
        lc = hc.many_distinct_locus(rng, nd)
        b = hc.ReadsBatch([lc]); rq = hc.request_of([lc])
        got, last = on_device(hmm, b, rq)
        hc.assert_same(got, capi.run_hapgen(hmm, b.ptr, rq, host=True), "%d distinct strings" % nd)
        assert int(got["n_distinct"][0]) == nd and int(got["blk_nopts"][1]) == nd + 1
        assert (last["device_loci"], last["host_loci"], last["reads_uploaded"]) == ((1, 0, 2 * nd) if nd <= dcap else (0, 1, 2 * nd)), (nd, last)


def test_truncated_hash_collides_and_changes_nothing():
    """In a fresh child process with HIPSTR_DEBUG_HAPGEN_HASH_BITS = 3: loci are redone by the host twin, every output stays identical;
    without the variable no locus is redone."""
    out = {}
    for bits in ("3", ""):
        env = dict(os.environ)
        env.pop("HIPSTR_DEBUG_HAPGEN_HASH_BITS", None)
        if bits:
            env["HIPSTR_DEBUG_HAPGEN_HASH_BITS"] = bits
        r = subprocess.run([sys.executable, os.path.join(HERE, "hapgen_child.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out[bits] = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert out["3"]["same"] and out[""]["same"], out
    assert out[""]["collision_loci"] == 0 and out[""]["device_loci"] == out[""]["loci"]
    assert out["3"]["collision_loci"] >= 1 and out["3"]["collision_loci"] + out["3"]["device_loci"] == out["3"]["loci"] and out["3"]["host_loci"] == 0


def test_chunks_twice_and_empty_loci(hmm):
    """The five golden batches as one call, loci without reads between them and three reads in front of the first locus; a budget that cuts
    the call into three or more chunks and a second call change no byte."""
    loci = []
    for name in BATCHES:
        loci += hc.load_golden(name)[0] + hc.no_flagged_loci()[:1]
    loci = hc.no_flagged_loci() + loci
    b = hc.ReadsBatch(loci, lead_reads=3); rq = hc.request_of(loci, lead_reads=3)
    host = capi.run_hapgen(hmm, b.ptr, rq, host=True)
    got, last = on_device(hmm, b, rq)
    hc.assert_same(got, host, "device against host twin")
    hc.assert_result(got, hc.expectation(loci, base_read=3), "all batches")
    assert last["chunks"] == 1 and last["device_loci"] == len(loci) and last["host_loci"] == 0
    raw = capi.run_hapgen(hmm, b.ptr, rq, raw=True)
    assert np.all(raw["ext_off"][:3] == capi.HAPGEN_FILL) and np.all(raw["ext_len"][:3] == capi.HAPGEN_FILL)
    again, _ = on_device(hmm, b, rq)
    hc.assert_same(again, got, "second call")
    os.environ["HIPSTR_HAPGEN_WS_MIB"] = "0.125"
    try:
        assert len(capi.hapgen_plan(hmm, b.ptr, rq)["chunks"]) >= 3
        cut, last = on_device(hmm, b, rq)
    finally:
        del os.environ["HIPSTR_HAPGEN_WS_MIB"]
    assert last["chunks"] >= 3 and last["device_loci"] == len(loci)
    hc.assert_same(cut, got, "three or more chunks")
    # nothing but loci without reads; no loci
    empty = hc.no_flagged_loci()[:1] * 3
    e, last = on_device(hmm, hc.ReadsBatch(empty), hc.request_of(empty))
    assert e["status"].tolist() == [2, 2, 2] and last["reads_uploaded"] == 0 and last["chunks"] == 0
    e, _ = on_device(hmm, hc.ReadsBatch([]), hc.request_of([]))
    assert e["opt_off"].tolist() == [0] and e["untouched"]


@pytest.fixture(scope="module")
def eighteen():
    inps = [fh.inputs(n) for n in fh.NAMES]
    loci = [fh.locus_of(i) for i in inps]
    return inps, loci, hc.ReadsBatch(loci), hc.request_of(loci, give_stop=False)


def test_the_eighteen_fixtures_on_the_device(hmm, eighteen):
    inps, loci, b, rq = eighteen
    got, last = on_device(hmm, b, rq)
    check_blocks(got, inps)
    hc.assert_result(got, restated(loci), "the eighteen")
    hc.assert_same(got, capi.run_hapgen(hmm, b.ptr, rq, host=True), "the eighteen, device against host twin")
    assert last["device_loci"] == 18


def test_reads_alone_to_the_alignment(hmm, eighteen):
    """hipstr_hapgen_batch(0) -> hipstr_pool_batch -> hipstr_hmm_upload / hipstr_hmm_align: the same log_aln_probs and seeds as the same
    calls on the batch built from the fixtures' own blocks."""
    inps, loci, b, rq = eighteen
    hb = capi.HapgenBatch(hmm, b.ptr, rq, 0)
    assert capi.hapgen_last(hmm)["collision_loci"] == 0 and capi.hapgen_last(hmm)["device_loci"] == 18
    check_batch(hb, inps)
    results = []
    for ptr in (hb.ptr, fh.fixture_batch(inps).ptr):
        pb = capi.PooledBatch(hmm, ptr, 0)
        dev = upload_and_align(hmm, pb)
        n_reads, n_out, _ = capi.batch_dims(pb.ptr)
        ll = np.zeros(n_out); seeds = np.zeros(n_reads, np.int32)
        try:
            assert hmm.hipstr_hmm_fetch(dev, ll.ctypes.data_as(capi._f64p), seeds.ctypes.data_as(capi._i32p)) == 0, hmm.hipstr_last_error().decode()
        finally:
            hmm.hipstr_hmm_free(dev)
        results.append((ll, seeds, pb.pool_index.copy()))
        pb.close()
    hb.close()
    assert np.array_equal(results[0][1], results[1][1]) and np.array_equal(results[0][2], results[1][2])
    same(results[0][0], results[1][0], "log_aln_probs from reads alone")
    assert results[0][0].size > 1000 and np.isfinite(results[0][0]).all()


def test_refusals_with_a_device(hmm):
    """The refusals of tests/test_hapgen_host.py on a library that has a device: decided before anything is launched or written."""
    from test_hapgen_host import test_refusals
    allocs = hmm.hipstr_debug_driver_allocs()
    test_refusals(hmm)
    assert hmm.hipstr_debug_driver_allocs() == allocs
