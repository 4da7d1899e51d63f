"""CPU: the read pooler's host side (include/hipstr_hmm.h: hipstr_pool_reads_host, hipstr_pool_batch(HIPSTR_POOL_ON_HOST); the plan of
hipstr_pool_reads, hipstr_debug_pool_plan) — the host twin (hipstr_amd/csrc/pool_host.cpp) against the compiled reference's own pools (six
fixtures written by ReadPooler, and ref_pool itself on fresh batches where the reference is built), against the numpy restatement of the two
reference functions (tests/pool_cases.py) on batches of many loci; the pooled batch against tests/test_readmat_gpu.py's pooled_batch_of;
the plan's thresholds and routes on either side of every threshold; header, exports and ctypes structs; refusals; and the stand-alone
sanitizer build of the host twin (tests/cpp/pool_host_test.cpp)."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from hipstr_amd import capi
import pool_cases as pc
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SCATTER = sorted(glob.glob(os.path.join(GOLD, "pool_scatter_*.npz")))
OWN = [os.path.join(GOLD, "pool_%s.npz" % n) for n in ("many_members", "near_identical", "wide_quals")]


def fixture_expectation(d):
    """A fixture's expectation in restate()'s shape, as far as the reference wrote it (pool_rep and pool_size follow from pool_index)."""
    pi = d["expect_pool_index"]; P = int(d["expect_n_pools"][0])
    return dict(pool_index=pi, n_pools=d["expect_n_pools"], pool_off=np.array([0, P], np.int32),
                pool_rep=np.array([int(np.nonzero(pi == p)[0][0]) for p in range(P)], np.int32), pool_size=np.bincount(pi, minlength=P).astype(np.int32),
                pool_qual_off=d["expect_pool_qual_off"], pool_quals=d["expect_pool_quals"])


@pytest.mark.parametrize("path", SCATTER + OWN, ids=lambda p: os.path.basename(p)[5:-4])
def test_host_twin_equals_the_compiled_reference(hmm_host, path):
    assert len(SCATTER) == 3
    d = np.load(path)
    got = capi.run_pool(hmm_host, util.batch_from_dict(d).ptr, host=True)
    pc.assert_pooled(got, fixture_expectation(d), os.path.basename(path))


def test_own_fixtures_bite():
    """What the three fixtures of make_golden_pool.py are there for."""
    m, n, w = (np.load(p) for p in OWN)
    sizes = np.bincount(m["expect_pool_index"])
    assert len(sizes) == 12 and sizes.max() >= 30 and (sizes % 2 == 0).any() and (sizes % 2 == 1).any() and (sizes > 8).sum() >= 8
    lens = np.diff(n["expect_pool_qual_off"])
    assert int(n["expect_n_pools"][0]) == 7 and sorted(set(lens.tolist())) == [59, 60, 61]
    assert w["quals"][:-1].min() == ord("!") and w["quals"][:-1].max() == ord("~")


@pytest.mark.skipif(not capi.have_ref(), reason="the compiled reference is not built here")
def test_host_twin_equals_ref_pool_on_fresh_batches(hmm_host):
    ref = capi.load_ref()
    ref.ref_pool.restype = C.c_int; ref.ref_pool.argtypes = [capi._BP, capi._i32p, capi._i32p, C.c_char_p, capi._i32p, C.c_int32]
    for seed in (101, 102, 103, 104):
        loci = pc.fuzz_loci(seed, 1, max_reads=250, max_len=120)
        if seed == 104:
            loci = [pc.size_locus(np.random.default_rng(seed), 8)]
        b = pc.batch_of(loci); R = len(loci[0]); cap = 1 << 20
        pi = np.zeros(R, np.int32); npools = np.zeros(1, np.int32); pq = C.create_string_buffer(cap); pqo = np.zeros(R + 1, np.int32)
        assert ref.ref_pool(b.ptr, pi.ctypes.data_as(capi._i32p), npools.ctypes.data_as(capi._i32p), pq, pqo.ctypes.data_as(capi._i32p), cap) == 0
        P = int(npools[0])
        want = fixture_expectation(dict(expect_pool_index=pi, expect_n_pools=npools, expect_pool_qual_off=pqo[:P + 1],
                                        expect_pool_quals=np.frombuffer(pq.raw[:pqo[P]], np.uint8)))
        pc.assert_pooled(capi.run_pool(hmm_host, b.ptr, host=True), want, "seed %d" % seed)
        pc.assert_pooled(capi.run_pool(hmm_host, b.ptr, host=True), pc.restate(loci), "restatement, seed %d" % seed)


def test_host_twin_equals_the_restatement_on_many_loci(hmm_host):
    named = pc.named_loci()
    for name, loci in list(named.items()) + [("fuzz", pc.fuzz_loci(11, 40)), ("all", [lc for v in named.values() for lc in v]), ("none", [])]:
        pc.assert_pooled(capi.run_pool(hmm_host, pc.batch_of(loci).ptr, host=True), pc.restate(loci), name)
    # upper median of two, signed order: 0x80 (-128) sorts before '!' — against the host twin only (Phred+33 never has such a byte)
    loci = [[(b"ACGT", bytes([0x80, 0x21, 0xFF, 0x7E])), (b"ACGT", bytes([0x21, 0x80, 0x7E, 0xFF]))]]
    got = capi.run_pool(hmm_host, pc.batch_of(loci).ptr, host=True)
    assert bytes(got["pool_quals"][:4]) == bytes([0x21, 0x21, 0x7E, 0x7E])
    pc.assert_pooled(got, pc.restate(loci), "signed bytes")


def signed_cases_bite(loci, want, net):
    """pc.signed_loci() is worth its name: every byte value occurs, and in every pool of two or more members (every size of the network,
    four sizes of the radix select) an unsigned order would give other medians than the signed one."""
    assert len(set(b"".join(q for lc in loci for _, q in lc))) == 256
    wrong = pc.restate_unsigned(loci)
    differs = set()
    for s, o0, o1 in zip(want["pool_size"].tolist(), want["pool_qual_off"][:-1].tolist(), want["pool_qual_off"][1:].tolist()):
        assert s == 1 or not np.array_equal(want["pool_quals"][o0:o1], wrong[o0:o1]), s
        differs.add(s)
    assert differs >= set(range(1, net + 3)) | {33, 300}
    assert bytes(want["pool_quals"][-14:]) == bytes([0x21, 0x21, 0x00, 0x00, 0x7F, 0x7F, 0xFF]) * 2


def test_host_twin_orders_bytes_as_signed_chars(hmm_host):
    loci = pc.signed_loci()
    want = pc.restate(loci)
    signed_cases_bite(loci, want, 8)
    pc.assert_pooled(capi.run_pool(hmm_host, pc.batch_of(loci).ptr, host=True), want, "signed bytes, every size")


@pytest.mark.parametrize("path", SCATTER, ids=lambda p: os.path.basename(p)[13:-4])
def test_pooled_batch_equals_pooled_batch_of(hmm_host, path):
    from test_readmat_gpu import pooled_batch_of
    d = np.load(path)
    want = pooled_batch_of(d).arrays
    pb = capi.PooledBatch(hmm_host, util.batch_from_dict(d).ptr, capi.POOL_ON_HOST)
    got = pb.arrays()
    assert np.array_equal(pb.pool_index, d["expect_pool_index"])
    for k in util._ARRAY_KEYS:
        assert np.array_equal(got[k], want[k]), k
    for k in util._BYTES_KEYS:
        assert bytes(got[k]) == want[k][:-1], k                     # (pooled_batch_of's byte arrays end with a NUL)
    assert (got["realign_hap"].size == 0) == (want["realign_hap"] is None) and (want["realign_hap"] is None or np.array_equal(got["realign_hap"], want["realign_hap"]))
    assert got["realign_read"].size == 0                            # realign_read is NULL: every pool is realigned
    pb.close()


# ------------------------------------------------------------------------------------------------------------------ the plan
def layout_constants():
    txt = open(os.path.join(ROOT, "hipstr_amd", "csrc", "pool_layout.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (HS_POOL_[A-Z_]+) (\d+)\b", txt, flags=re.M)}


def test_plan_thresholds_are_the_headers(hmm_host):
    h = layout_constants()
    p = capi.pool_plan(hmm_host, pc.batch_of([]).ptr)
    t = p["thresholds"]
    assert t == {k: h[k] for k in t} and len(t) == 10
    for k in ("HS_POOL_LDS_READS", "HS_POOL_NET", "HS_POOL_HASH_STEP", "HS_POOL_WS_MIB", "HS_POOL_THREADS"):
        assert k in t
    assert p["routes"] == list(capi.POOL_ROUTES) and p["chunks"] == [] and p["routes_hit"] == []
    assert (h["HS_POOL_ROUTE_COPY"], h["HS_POOL_ROUTE_NET"], h["HS_POOL_ROUTE_RADIX"]) == (0, 1, 2)
    assert p["budget_bytes"] == t["HS_POOL_WS_MIB"] << 20
    # the grouping workgroup's LDS at the largest locus it takes fits a CU's 160 KiB
    rng = np.random.default_rng(1)
    big = capi.pool_plan(hmm_host, pc.batch_of([pc.short_read_locus(rng, t["HS_POOL_LDS_READS"])]).ptr)
    assert 64 * 1024 < big["chunks"][0]["lds_bytes"] <= 160 * 1024


def test_plan_routes_on_either_side_of_every_threshold(hmm_host):
    rng = np.random.default_rng(2)
    t = capi.pool_plan(hmm_host, pc.batch_of([]).ptr)["thresholds"]
    lds, net, step = t["HS_POOL_LDS_READS"], t["HS_POOL_NET"], t["HS_POOL_HASH_STEP"]
    hit = set()
    # reads of a locus: the LDS route's edge
    for n, dev in ((lds - 1, 1), (lds, 1), (lds + 1, 0)):
        p = capi.pool_plan(hmm_host, pc.batch_of([pc.short_read_locus(rng, n)]).ptr)
        c = p["chunks"][0]
        assert (c["device_loci"], c["host_loci"], c["reads"]) == (dev, 1 - dev, n * dev), n
        assert ("device" in p["routes_hit"]) == bool(dev) and ("host" in p["routes_hit"]) == (not dev)
        hit |= set(p["routes_hit"])
    # members of a pool: copy | net | radix
    s = pc.rand_seq(rng, 20)
    for m, want in ((1, [1, 0, 0]), (2, [0, 1, 0]), (net, [0, 1, 0]), (net + 1, [0, 0, 1])):
        p = capi.pool_plan(hmm_host, pc.batch_of([[(s, pc.rand_qual(rng, 20))] * m]).ptr)
        assert p["chunks"][0]["pools"] == want, m
        hit |= set(p["routes_hit"])
    # steps of the hash wavefront: 64 lanes of `step` bytes
    for n, steps in ((0, 0), (1, 1), (64 * step, 1), (64 * step + 1, 2)):
        p = capi.pool_plan(hmm_host, pc.batch_of([[(pc.rand_seq(rng, n), pc.rand_qual(rng, n))]]).ptr)
        assert p["chunks"][0]["hash_steps"] == steps, n
    # the routes the GPU test's cases reach are all there are
    for name, b in pc.sanity_batches():
        hit |= set(capi.pool_plan(hmm_host, b.ptr)["routes_hit"])
    assert hit == set(capi.POOL_ROUTES)


def test_plan_chunks_are_whole_loci_under_the_budget(hmm_host):
    loci = pc.fuzz_loci(7, 40)
    b = pc.batch_of(loci)
    one = capi.pool_plan(hmm_host, b.ptr)
    assert len(one["chunks"]) == 1 and one["chunks"][0]["l1"] == 40
    p = capi.pool_plan(hmm_host, b.ptr, ws_mib=0.25)
    ch = p["chunks"]
    assert len(ch) >= 3 and ch[0]["l0"] == 0 and ch[-1]["l1"] == 40 and all(a["l1"] == c["l0"] for a, c in zip(ch, ch[1:]))
    assert all(c["bytes"] <= p["budget_bytes"] or c["l1"] - c["l0"] == 1 for c in ch)
    assert sum(c["reads"] for c in ch) == one["chunks"][0]["reads"] and sum(c["bytes"] for c in ch) == one["chunks"][0]["bytes"]
    # the next locus would not have fitted
    cost = [capi.pool_plan(hmm_host, pc.batch_of([lc]).ptr)["chunks"][0]["bytes"] for lc in loci]
    for c in ch[:-1]:
        assert c["bytes"] + cost[c["l1"]] > p["budget_bytes"]


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_symbols_structs_and_headers_agree(hmm_host):
    pub = open(os.path.join(ROOT, "include", "hipstr_hmm.h")).read(); dbg = open(os.path.join(ROOT, "include", "hipstr_hmm_debug.h")).read()
    for n in ("hipstr_pool_reads", "hipstr_pool_reads_host", "hipstr_pool_batch", "hipstr_pooled_batch_batch", "hipstr_pooled_batch_pool_index",
              "hipstr_pooled_batch_free"):
        assert hasattr(hmm_host, n) and re.search(r"\b%s\(" % n, pub), n
    for n in ("hipstr_debug_pool_plan", "hipstr_debug_pool_last", "hipstr_debug_pool_last_timing"):
        assert hasattr(hmm_host, n) and re.search(r"\b%s\(" % n, dbg) and n not in pub, n
    assert re.search(r"#define HIPSTR_POOL_ON_HOST (\d+)u", pub).group(1) == str(capi.POOL_ON_HOST)
    body = re.search(r"typedef struct hipstr_pool_out \{(.*?)\} hipstr_pool_out_t;", pub, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [f for f, _ in capi.HipstrPoolOut._fields_] == list(capi.POOL_FIELDS)
    from hipstr_amd import build
    assert "pool.hip" in build.HIP_SOURCES and "pool_host.cpp" in build.HIP_SOURCES and "pool_layout.h" in build.HIP_HEADERS


def test_refusals(hmm_host):
    b = pc.batch_of([[(b"ACGT", b"FFFF")]])
    a = {k: np.zeros(8, np.int32) for k in capi.POOL_FIELDS[:6]}; q = np.zeros(8, np.uint8)
    def out(skip=None):
        return capi.HipstrPoolOut(*[None if k == skip else a[k].ctypes.data_as(capi._i32p) for k in capi.POOL_FIELDS[:6]],
                                  None if skip == "pool_quals" else q.ctypes.data_as(C.POINTER(C.c_char)))
    for fn in (hmm_host.hipstr_pool_reads_host, hmm_host.hipstr_pool_reads):
        for args in ((None, None), (b.ptr, None), (None, C.byref(out()))):
            assert fn(*args) != 0 and b"null argument" in hmm_host.hipstr_last_error()
        for k in capi.POOL_FIELDS:
            assert fn(b.ptr, C.byref(out(k))) != 0 and b"null output array" in hmm_host.hipstr_last_error(), k
        # tables validate_tables rejects
        bad = pc.batch_of([[(b"ACGT", b"FFFF"), (b"AC", b"FF")]])
        bad.arrays["base_off"][1] = 7
        assert fn(bad.ptr, C.byref(out())) != 0 and b"base_off must not decrease" in hmm_host.hipstr_last_error()
        bad = pc.batch_of([[(b"ACGT", b"FFFF")], []])
        bad.arrays["read_off"][2] = 0
        assert fn(bad.ptr, C.byref(out())) != 0 and b"read_off must not decrease" in hmm_host.hipstr_last_error()
        assert all(np.all(v == 0) for v in a.values()) and np.all(q == 0)          # nothing written
    assert hmm_host.hipstr_pool_batch(None, 0) is None and b"null argument" in hmm_host.hipstr_last_error()
    assert hmm_host.hipstr_pool_batch(b.ptr, 6) is None and b"unknown flag" in hmm_host.hipstr_last_error()
    assert hmm_host.hipstr_debug_pool_plan(None, 0.0, None, 0) == -1
    assert hmm_host.hipstr_pooled_batch_batch(None) in (None, 0) or not hmm_host.hipstr_pooled_batch_batch(None)
    hmm_host.hipstr_pooled_batch_free(None)


def test_no_host_fallback_without_a_device(hmm_host):
    """tests/test_prep.py::test_no_cpu_fallback_without_device's rule for the pooler: the device entry point fails, it does not quietly pool on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    b = pc.batch_of(pc.fuzz_loci(3, 2, max_reads=20, max_len=30))
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.run_pool(hmm_host, b.ptr)
    with pytest.raises(RuntimeError, match="no HIP device"):
        capi.PooledBatch(hmm_host, b.ptr, 0)
    capi.run_pool(hmm_host, b.ptr, host=True)                      # the host entry point needs none


# ------------------------------------------------------------------------------------------------------------------ sanitizers, stand-alone
def test_host_twin_under_sanitizers(tmp_path):
    """pool_host.cpp next to a program with a main of its own, both built with AddressSanitizer and UBSan, the runtimes linked statically:
    nothing is preloaded and nothing of it is loaded into python."""
    exe = str(tmp_path / "pool_host_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "pool_host_test.cpp"), os.path.join(ROOT, "hipstr_amd", "csrc", "pool_host.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ok, loci, reads, pools = r.stdout.decode().split()
    assert ok == "ok" and int(loci) == 60 and int(reads) > 5000 and int(pools) > 500
