"""GPU: hipstr_pool_reads / hipstr_pool_batch on the device (hipstr_amd/csrc/pool.hip) against the compiled reference's pools (the six
fixtures), the numpy restatement (tests/pool_cases.py) and the host twin, bit for bit in every output and untouched behind what the call
writes.  Sizes are the smallest at which a decision of hipstr_amd/csrc/pool_layout.h flips, read from the plan.  In every case that does
not force a collision the count of loci redone after one must be 0: a broken hash must not hide behind the fallback."""
import os

import numpy as np
import pytest

from hipstr_amd import capi
import pool_cases as pc
import util
from test_pool_host import SCATTER, OWN, fixture_expectation, signed_cases_bite
from test_readmat_gpu import upload_and_align, same

pytestmark = pytest.mark.gpu
PATTERNS = (0xFF, 0x7F, 0x80, 0x00)


@pytest.fixture(scope="module")
def T(hmm):
    return capi.pool_plan(hmm, pc.batch_of([]).ptr)["thresholds"]


@pytest.fixture(scope="module")
def named(T):
    """name -> (loci, batch, restatement): built once, shared, never changed."""
    out = {}
    for name, loci in pc.named_loci(T["HS_POOL_NET"], T["HS_POOL_HASH_STEP"]).items():
        out[name] = (loci, pc.batch_of(loci), pc.restate(loci))
    return out


def pooled(hmm, b, collisions=0):
    got = capi.run_pool(hmm, b.ptr)
    last = capi.pool_last(hmm)
    assert (last["collision_loci"] > 0) == bool(collisions), last
    return got, last


@pytest.mark.parametrize("path", SCATTER + OWN, ids=lambda p: os.path.basename(p)[5:-4])
def test_fixtures_of_the_compiled_reference(hmm, path):
    d = np.load(path)
    got, last = pooled(hmm, util.batch_from_dict(d))
    pc.assert_pooled(got, fixture_expectation(d), os.path.basename(path))
    assert last["device_loci"] == 1 and last["host_loci"] == 0 and last["chunks"] == 1


@pytest.mark.parametrize("path", SCATTER, ids=lambda p: os.path.basename(p)[13:-4])
def test_the_references_matrix_from_unpooled_reads(hmm, path):
    """hipstr_pool_batch -> upload / align -> scatter with the returned pool_index: the matrix and seeds calc_hap_aln_probs left."""
    d = np.load(path)
    pb = capi.PooledBatch(hmm, util.batch_from_dict(d).ptr, 0)
    assert capi.pool_last(hmm)["collision_loci"] == 0
    assert np.array_equal(pb.pool_index, d["expect_pool_index"])
    # (every pool is realigned here; the fixture copies only from pools its realign_pool kept, so the copied rows are the same)
    R = int(d["read_off"][1]); A = int(d["hap_off"][1])
    dev = upload_and_align(hmm, pb)
    rm = capi.ReadMatrix(hmm, [A], [0, R], pb.pool_index, d["second_mate"], init_ll=d["prefill"], init_seeds=np.full(R, -9, np.int32))
    try:
        rm.scatter(dev, d["copy_read"])
        ll, seeds = rm.fetch()
    finally:
        rm.close(); hmm.hipstr_hmm_free(dev); pb.close()
    assert np.array_equal(seeds, d["expect_seeds"])
    same(ll, d["expect_log_aln_probs"], os.path.basename(path))


@pytest.mark.parametrize("name", ["sizes", "lengths", "counts", "many_small"])
def test_named_shapes(hmm, named, T, name):
    loci, b, want = named[name]
    got, last = pooled(hmm, b)
    pc.assert_pooled(got, want, name)
    assert last["device_loci"] == len(loci) and last["host_loci"] == 0 and last["chunks"] == 1
    net = T["HS_POOL_NET"]
    if name == "sizes":           # one pool each of 1, 2, 3, net, net + 1, 300 members and the three pools of 6, 5, 5
        assert sorted(want["pool_size"].tolist()) == sorted([1, 2, 3, net, net + 1, 300, 6, 5, 5])
        assert (last["pools_copy"], last["pools_net"], last["pools_radix"]) == (1, 6, 2)
        q = sorted((int(s), bytes(want["pool_quals"][o:o + 37])) for s, o in zip(want["pool_size"], want["pool_qual_off"]) if s in (5, 6))
        assert q == [(5, b"C" * 37), (5, b"F" * 37), (6, b"F" * 37)]
    if name == "lengths":         # every length, the read that differs in its last byte, the lower-case copy
        lens = np.diff(want["pool_qual_off"])
        assert set(pc.LENGTHS) <= set(lens.tolist()) and int(want["n_pools"][0]) == 2 * len(pc.LENGTHS)
    if name == "counts":
        assert want["n_pools"].tolist() == [0, 1, 1, 0, 50, 0]
    if name == "many_small":
        assert len(loci) == 300 and all(len(lc) == 7 for lc in loci)


def test_bytes_order_as_signed_chars(hmm, T):
    """Qualities over 0x00 .. 0xFF, the device against the host twin: pools of 1 .. HS_POOL_NET + 2, 33 and 300 members, so the copy, every
    size of the network and the radix select all meet bytes >= 0x80, and in each of them an unsigned order gives other medians."""
    net = T["HS_POOL_NET"]
    loci = pc.signed_loci(net)
    want = pc.restate(loci)
    signed_cases_bite(loci, want, net)
    b = pc.batch_of(loci)
    host = capi.run_pool(hmm, b.ptr, host=True)
    got, last = pooled(hmm, b)
    pc.assert_same(got, host, "device against host twin, signed bytes")
    pc.assert_pooled(got, want, "signed bytes")
    assert (last["device_loci"], last["host_loci"]) == (3, 0)
    assert (last["pools_copy"], last["pools_net"], last["pools_radix"]) == (2, 2 * (net - 1) + 2, 2 * 4)


def test_every_locus_alone_equals_the_locus_in_the_batch(hmm, named):
    for name in ("sizes", "lengths", "counts"):
        loci, b, want = named[name]
        for l, lc in enumerate(loci):
            got, _ = pooled(hmm, pc.batch_of([lc]))
            pc.assert_pooled(got, pc.restate([lc]), "%s locus %d alone" % (name, l))
            p0, p1 = want["pool_off"][l], want["pool_off"][l + 1]
            assert np.array_equal(got["pool_size"][:p1 - p0], want["pool_size"][p0:p1])


def test_the_lds_routes_edge(hmm, T):
    lds = T["HS_POOL_LDS_READS"]
    rng = np.random.default_rng(5)
    for n in (lds - 1, lds, lds + 1):
        lc = pc.short_read_locus(rng, n)
        got, last = pooled(hmm, pc.batch_of([lc]))
        pc.assert_pooled(got, pc.restate([lc]), "%d reads" % n)
        assert (last["device_loci"], last["host_loci"]) == ((1, 0) if n <= lds else (0, 1)), (n, last)
        assert last["reads_uploaded"] == (n if n <= lds else 0) and last["pools_copy"] + last["pools_net"] + last["pools_radix"] == (int(got["n_pools"][0]) if n <= lds else 0)
        assert n > lds or last["pools_radix"] > 100


def test_truncated_hash_collides_and_changes_nothing(hmm, named, monkeypatch):
    loci = pc.fuzz_loci(7, 12) + named["lengths"][0]
    b = pc.batch_of(loci)
    want = pc.restate(loci)
    plain, _ = pooled(hmm, b)
    monkeypatch.setenv("HIPSTR_DEBUG_POOL_HASH_BITS", "4")
    got, last = pooled(hmm, b, collisions=1)
    monkeypatch.delenv("HIPSTR_DEBUG_POOL_HASH_BITS")
    pc.assert_same(got, plain, "4-bit hash")
    pc.assert_pooled(got, want, "4-bit hash")
    assert last["collision_loci"] >= 1 and last["collision_loci"] + last["device_loci"] == len(loci)


def test_chunks_twice_and_the_host_twin(hmm):
    """200 fuzzed loci: the device equals the host twin and the restatement; a budget that cuts the batch into three or more chunks and a
    second call change no byte."""
    loci = pc.fuzz_loci(20261018, 200)
    b = pc.batch_of(loci)
    sizes = pc.restate(loci)["pool_size"]
    assert sizes.min() == 1 and sizes.max() >= 60 and len(set(range(1, 61)) & set(sizes.tolist())) >= 50        # pools of 1 to 60 members and more
    host = capi.run_pool(hmm, b.ptr, host=True)
    got, last = pooled(hmm, b)
    pc.assert_same(got, host, "device against host twin")
    pc.assert_pooled(got, pc.restate(loci), "fuzz")
    assert last["chunks"] == 1 and last["device_loci"] == 200
    again, _ = pooled(hmm, b)
    pc.assert_same(again, got, "second call")
    os.environ["HIPSTR_POOL_WS_MIB"] = "4"
    try:
        assert len(capi.pool_plan(hmm, b.ptr)["chunks"]) >= 3
        cut, last = pooled(hmm, b)
    finally:
        del os.environ["HIPSTR_POOL_WS_MIB"]
    assert last["chunks"] >= 3
    pc.assert_same(cut, got, "three or more chunks")


def test_poisoned_caches(hmm, named):
    """tests/test_poison_gpu.py's protocol: warm once, then under every poison byte no new driver allocation and four identical results."""
    loci = named["sizes"][0] + named["lengths"][0] + named["counts"][0] + pc.fuzz_loci(9, 10)
    b = pc.batch_of(loci)
    want = pc.restate(loci)
    hmm.hipstr_hmm_trim()
    run = lambda: pooled(hmm, b)[0]
    run()
    allocs = hmm.hipstr_debug_driver_allocs()
    out = []
    for pat in PATTERNS:
        assert hmm.hipstr_debug_cache_poison(pat) > 0, hmm.hipstr_last_error().decode()
        out.append(run())
    assert hmm.hipstr_debug_driver_allocs() == allocs
    for pat, r in zip(PATTERNS, out):
        pc.assert_same(r, out[0], "poison 0x%02X" % pat)
    pc.assert_pooled(out[0], want, "poisoned")


def test_refusals_with_a_device(hmm):
    """The refusals of tests/test_pool_host.py on a library that has a device: decided before anything is launched or written."""
    from test_pool_host import test_refusals
    allocs = hmm.hipstr_debug_driver_allocs()
    test_refusals(hmm)
    assert hmm.hipstr_debug_driver_allocs() == allocs
