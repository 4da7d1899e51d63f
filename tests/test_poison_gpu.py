"""GPU: every device stage on poisoned cache blocks — no kernel reads a word of a workspace or a result block that it did not write.

Every device workspace and every pinned result block comes from the block caches (BlockCache, api.hip), which never clear a block.  A fresh
driver page is zero and a recycled block holds the previous call's results — usually the right answer to a nearly identical question — so the
rest of the suite cannot see a kernel that reads stale memory.  Here every case runs once (the cache then holds free blocks of every size
the case takes), then again after hipstr_debug_cache_poison has filled every free block and every chunk's uncarved tail with 0xFF (NaN, -1,
every choice bit of a traceback byte), 0x7F (what HS_ASSIGN_EMPTY is built from; huge, finite and positive as a float: wins a maximum), 0x80
(a large negative int, a tiny negative float: wins a minimum) and 0x00 (the fresh page).  hipstr_debug_driver_allocs must not grow over the
poisoned runs — every block they took was poisoned memory — the four results must be identical bit for bit, and the first must meet the
stage's contract against the oracle, judged by the stage's own helper.

Before the first device run — the device-side loops that wait on a word, and the statement that writes it (a kernel spinning on a word
nobody wrote would spin for ever under a poison byte):

  hs_trail_kernel_coop / hs_lead_kernel_coop, band_sweep_coop (hmm_kernels.hip)
    prog[w] (columns a band has finished: `while (prog_read(a_top) <= base + j)`, `... (prog + wlast) ... <= base - nmax + j`, and
    `base + j - prog_read(a_bot) >= HS_RING`) is s_prog[] in LDS, not global memory: zeroed by `if (threadIdx.x < W + 1) s_prog[..] = 0`
    + __syncthreads() at the top of the trailing kernel and by `if (threadIdx.x <= W) s_prog[..] = 0` between two barriers for every item of
    the leading kernel.  s_q[] (records published / read: `while (prog_read(a_q) <= k)`, `while (prog_read(a_q + 4 (2 + ww)) < k)`) is LDS
    too: `if (threadIdx.x < 2 + W) s_q[..] = 0` before the same barrier.  No block of the cache is waited on.
    The boundary rows in the HBM scratch (ws_band) are not waited on either: the last band stores, drains (s_waitcnt vmcnt(0)) and then
    publishes the column in its LDS counter.
  item counters of the coop kernels (`atomicAdd(ctr, 1)`, ctr = redo + n_active + chunk: global, from the cache) and the re-do flags
    not waited on, but they end the item loops and pick the items: cleared by the n_clear pass of hs_col_kernel (`d.redo[i] = 0` for
    i < n_active + 2 chunks + 2), the first kernel hs_launch_lead2 puts on the stream for every chunk of every pass, in front of the
    leading-flank kernel on the same stream.  hipstr_hmm_align returns before any launch when n_active == 0.
  hs_assign_requests_kernel, assign_slot_find (assign.hip): `while (tab[h] != key) h = (h + 1) & mask`
    ends at the slot hs_assign_kernel's atomicCAS gave the key, earlier on the same stream (only reads with best_hap >= 0 are looked
    up, exactly the ones inserted); the table was set to HS_ASSIGN_EMPTY by the hipMemsetAsync(0x7f) in front of hs_assign_kernel and
    has at least one empty slot more than keys.
  EM (em.hip): no kernel waits.  hs_em_units and em_locus() compare blockIdx with counts[0] / next_counts[0], written by hs_em_compact (one
    workgroup, `d.next_counts[0] = base_n`) in the launch before; the host sizes the grids from a pinned copy of the counts it waits for
    with an event (hipMemcpyAsync + hipEventRecord + hipEventQuery), and its loop is bounded by max_iter + 2 rounds.
  hs_alleles_kernel (alleles.hip): the claim loop of step 2 (`prev = atomicCAS(&s_lead[s], -1, i)`, on to the next slot while the slot is
    another key's) and the probe loop of step 3 (`L = s_lead[s]; if (L < 0) break;`, the mapping through `s_val[s]`)
    walk s_lead[] / s_val[], the haplotype table in LDS, not global memory: `for (i = t; i < HS_ALLELES_SLOTS; i += AL_NT){ s_lead[i] = -1;
    s_val[i] = -1; }` at the top of the kernel writes every slot first (s_map[] and s_cnt[] beside it), a __syncthreads() stands between
    that and step 2 and another between step 2 and step 3.  Neither loop spins on a word: both count `probe < HS_ALLELES_SLOTS`, and the
    table is at most half full (the static_assert under the kernel), so an empty slot ends them earlier.  What bounds the other loops —
    nopts, l_ohap / l_nhap, o_off / n_off, n_src — are uploaded pieces: ChunkBlocks::upload copies them in front of the kernel on the same
    stream.  No block of the cache is waited on (tests/test_alleles_gpu.py::test_alleles_on_poisoned_cache_blocks).
  trace.hip, nw.hip, post_kernels.hip: no loop waits on memory.  The walks over decision bytes (hs_trace_walk, trace_assemble_serial,
    hs_nw_walk's `while (row > 0 && type >= 0)`) move towards row / column 0 with every byte they read, whatever it holds.

Every one of them is covered by a write in the same launch set; nothing had to be fixed before the first run."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from hipstr_amd import capi
from em_cases import em_case
import route_cases as rc
import stage_route_cases as sc
import test_assign_gpu as ta
import test_em_gpu as te
import test_em_oracle as teo
import test_genotypes_gpu as tg
import test_stage_routes_gpu as tsr
import test_trace_assemble_gpu as tta
import util

pytestmark = pytest.mark.gpu
PATTERNS = (0xFF, 0x7F, 0x80, 0x00)
FILL = -3.25                                   # tests/test_routes_gpu.py, tests/test_stream_gpu.py


@pytest.fixture(scope="module", autouse=True)
def small_caches(hmm):
    """Whatever the tests before left in the caches goes back to the driver: a fill then costs milliseconds."""
    hmm.hipstr_hmm_trim()


def same_bits(a, b, what):
    """Nested tuples / lists / dicts of arrays, floats, ints and strings, identical bit for bit (floats as their bytes: NaN payloads and signed zeros count)."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            same_bits(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), "%s differs in %d of %d entries, first at %s" % (what, int((x != y).sum()), x.size, np.argwhere(x != y)[:1].tolist())
    elif isinstance(a, float):
        assert struct.pack("d", a) == struct.pack("d", b), "%s: %r != %r" % (what, a, b)
    else:
        assert a == b, "%s: %r != %r" % (what, a, b)


def poisoned(hmm, run, what, same=same_bits):
    """The protocol of the module docstring; returns the four poisoned results."""
    run()                                                       # warm-up: free blocks of every size the case takes
    allocs = hmm.hipstr_debug_driver_allocs()
    out = []
    for pat in PATTERNS:
        filled = hmm.hipstr_debug_cache_poison(pat)
        assert filled > 0, "%s: hipstr_debug_cache_poison(0x%02X) filled %d bytes: %s" % (what, pat, filled, hmm.hipstr_last_error().decode())
        out.append(run())
    grown = hmm.hipstr_debug_driver_allocs() - allocs
    assert grown == 0, "%s: %d blocks came fresh from the driver during the poisoned runs: the warm-up did not cover the case" % (what, grown)
    for pat, r in zip(PATTERNS[1:], out[1:]):
        same(r, out[0], "%s, 0x%02X against 0x%02X" % (what, pat, PATTERNS[0]))
    return out


# =================================================================================================== the hook itself
def test_the_hook_fills_free_blocks_and_tails_and_no_block_that_is_out(hmm):
    n = 4096
    held = hmm.hipstr_debug_cache_get(n * 8); assert held
    x = np.arange(n, dtype=np.float64); y = np.zeros(n)
    # (one block out; the cr_math probe takes two more blocks and gives them back: those are free)
    assert hmm.hipstr_debug_cr_math(0, x.ctypes.data_as(capi._f64p), y.ctypes.data_as(capi._f64p), n) == 0
    try:
        a = hmm.hipstr_debug_cache_poison(0x7F)
        b = hmm.hipstr_debug_cache_poison(0x80)
        assert a == b and a >= 2 * n * 8                        # the same free blocks and tails twice; at least the probe's two blocks
        y2 = np.zeros(n)
        assert hmm.hipstr_debug_cr_math(0, x.ctypes.data_as(capi._f64p), y2.ctypes.data_as(capi._f64p), n) == 0
        assert np.array_equal(y.view(np.uint64), y2.view(np.uint64))
    finally:
        hmm.hipstr_debug_cache_put(held)
    grown = hmm.hipstr_debug_cache_poison(0x00) - a             # the block that was out is free now, and only now filled:
    assert n * 8 <= grown <= 2 * n * 8                          # its own size (the cache hands out a free block of up to twice the request)


# =================================================================================================== forward pass
FORWARD = [(c, d) for c in rc.CASES for d in c.deltas]


@pytest.fixture(scope="module")
def flim(hmm):
    return rc.lim_of(hmm)


@pytest.mark.parametrize("case,d", FORWARD, ids=["%s%+d" % (c.name, d) for c, d in FORWARD])
def test_forward_pass(hmm, oracle, flim, case, d):
    b = rc.build(case, flim, d)
    what = "forward %s %+d" % (case.name, d)
    with rc.environ(rc.case_env(case, d)):
        want, ws = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
        got, gs = poisoned(hmm, lambda: capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL), what)[0]
    assert np.array_equal(gs, ws), what + ": seeds differ"
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == FILL, want == FILL), what + ": untouched entries differ"
    assert np.array_equal(got, want), "%s: max|diff| %g" % (what, np.nanmax(np.abs(got - want)))


def test_forward_matrix_with_unwritten_entries_read_on_the_device(hmm, oracle):
    """Masked reads and alleles (not realigned) leave entries of the device's likelihood matrix that no kernel writes.  hipstr_hmm_fetch never
    copies them, so the one-shot cases above cannot see what they hold; whoever takes hipstr_hmm_dev_aln_probs reads them, as 0 (the upload
    clears the matrix when not all of it will be written).  Here the posteriors are computed from the device's matrix and must equal the
    oracle's posteriors of the oracle's matrix with 0 in the untouched entries."""
    nl, R = 3, 24
    sb = capi.SynthBatch(n_loci=nl, reads_per_locus=R, n_str_alleles=5, seed=83, mask_rate=0.25)
    marked, _ = capi.run_align(oracle, "oracle_", sb.ptr, fill=FILL)
    assert 0 < int((marked == FILL).sum()) < marked.size                     # some entries are left alone, not all
    want_ll, _ = capi.run_align(oracle, "oracle_", sb.ptr, fill=0.0)
    A = np.diff(np.ctypeslib.as_array(sb.ptr.contents.hap_off, shape=(nl + 1,)))
    rng = np.random.default_rng(83); n = nl * R
    kw = dict(n_alleles=A, n_samples=np.full(nl, 2), read_off=np.arange(nl + 1) * R, sample_label=np.tile(np.repeat(np.arange(2), R // 2), nl),
              log_p1=-rng.random(n), log_p2=-rng.random(n), read_weight=np.ones(n, np.int32))
    on_dev = capi.PostBatch(log_aln_probs=None, **kw); pb = capi.PostBatch(log_aln_probs=want_ll, **kw)
    S = int(pb.samp_off[-1])
    def run():
        dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev, hmm.hipstr_last_error()
        try:
            assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error()
            post = np.zeros(int(pb.post_off[-1])); tot = np.zeros(S); gt = np.zeros(2 * S, np.int32); ltot = np.zeros(nl)
            assert hmm.hipstr_post_run(on_dev.ptr, hmm.hipstr_hmm_dev_aln_probs(dev), post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p),
                                       gt.ctypes.data_as(capi._i32p), ltot.ctypes.data_as(capi._f64p)) == 0, hmm.hipstr_last_error()
        finally:
            hmm.hipstr_hmm_free(dev)
        return post, tot, gt.reshape(-1, 2), ltot
    got = poisoned(hmm, run, "posteriors of the device's matrix, masked batch")[0]
    want = capi.run_posteriors(oracle, "oracle_", pb)
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_posteriors(oracle, "oracle_", pb)
    util.assert_arrays_exact(got, want, cr, "posteriors of the device's matrix, masked batch")


# =================================================================================================== traceback
@pytest.fixture(scope="module")
def slim(hmm):
    return sc.limits(hmm)


@pytest.fixture(scope="module")
def tcalls(hmm, slim):
    return {c.name: c for c in sc.trace_calls(hmm, slim["trace"])}


def _raw_same(n):
    return lambda a, b, what: tta.assert_raw_equal(a, b, n, what)


def _trace_case(hmm, oracle, bptr, rr, aa, h2r, seeds, flags, env, what, cap=1 << 21):
    with rc.environ(env):
        run = lambda: capi.run_trace(hmm, "hipstr_hmm_", bptr, rr, aa, h2r, cap=cap, unpack=False, req_seed=seeds, flags=flags)
        got = poisoned(hmm, run, what, same=_raw_same(len(rr)))[0]
    want = capi.run_trace(oracle, "oracle_", bptr, rr, aa, h2r, cap=cap, req_seed=seeds)
    util.assert_traces_equal(capi.unpack_trace(got, len(rr)), want, what)


@pytest.mark.parametrize("flags", [0, capi.TRACE_ASSEMBLE_DEVICE], ids=["host_replay", "device_assembly"])
@pytest.mark.parametrize("name", tsr.TRACE_NAMES)
def test_traceback(hmm, oracle, tcalls, name, flags):
    call = tcalls[name]
    env = {"HIPSTR_TRACE_WS_MIB": call.ws_mib} if call.ws_mib else {}
    _trace_case(hmm, oracle, call.batch.ptr, call.rr, call.aa, sc.h2r_of(oracle, call), call.seeds, flags, env, "trace %s flags %d" % (name, flags))


@pytest.mark.parametrize("flags", [0, capi.TRACE_ASSEMBLE_DEVICE], ids=["host_replay", "device_assembly"])
def test_traceback_of_the_smallest_request_staged_in_hbm(hmm, oracle, flags):
    """The shape tests/test_trace_assemble_gpu.py::test_a_request_beyond_the_lds_threshold_reads_hbm finds, found the same way."""
    def shape(n):
        sb = capi.SynthBatch(n_loci=1, reads_per_locus=4, n_str_alleles=2, read_len=n, flank_len=(6 * n) // 10, str_bp=30, seed=35)
        rr, aa = tta._requests(oracle, sb, 2, 35)
        h2r = util.synthetic_hap_to_ref(oracle, sb.ptr)
        return sb, rr, aa, h2r, capi.trace_assemble_plan(hmm, sb.ptr, rr, aa, None, h2r)
    n = 64
    while "assemble_hbm" not in shape(n)[4]["routes_hit"]:
        n += 64
        assert n <= 1024
    sb, rr, aa, h2r, plan = shape(n)
    _trace_case(hmm, oracle, sb.ptr, rr, aa, h2r, None, flags, {}, "trace HBM route flags %d" % flags, cap=1 << 22)


# =================================================================================================== Needleman-Wunsch
NW_NAMES = ["rungs", "ref_lengths", "over_budget_whole", "over_budget_1"]


@pytest.mark.parametrize("pen", [False, True], ids=["no_end_penalty", "end_penalty"])
@pytest.mark.parametrize("name", NW_NAMES)
def test_needleman_wunsch(hmm, oracle, slim, name, pen):
    calls = {c.name: c for c in sc.nw_calls(slim["nw"])}
    assert sorted(calls) == sorted(NW_NAMES)
    call = calls[name]
    what = "nw %s penalty %d" % (name, pen)
    with rc.environ({"HIPSTR_NW_WS_MIB": call.ws_mib} if call.ws_mib else {}):
        got = poisoned(hmm, lambda: capi.run_nw(hmm, "hipstr_", call.pairs, pen), what)[0]
    want = capi.run_nw(oracle, "oracle_", call.pairs, pen)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s pair %d (reference %d, read %d bases)" % (what, i, len(call.pairs[i][0]), len(call.pairs[i][1]))


# =================================================================================================== posteriors and genotypes
POST_CASES = 30                                 # stage_route_cases.post_calls: their names carry the library's limits, so they are taken by position


@pytest.fixture(scope="module")
def pcalls(slim):
    return sc.post_calls(slim["post"])


def test_posterior_case_list_is_complete(pcalls):
    assert len(pcalls) == POST_CASES and len({c.name for c in pcalls}) == POST_CASES
    for a, b in sc.POST_TWINS:                              # split and unsplit twins both
        assert {a, b} <= {c.name for c in pcalls}


@pytest.mark.parametrize("i", range(POST_CASES))
def test_posteriors(hmm, oracle, pcalls, i):
    name, pb = pcalls[i].name, pcalls[i].pb
    got = poisoned(hmm, lambda: tsr._post(hmm, pb), "posteriors " + name)[0]
    want = capi.run_posteriors(oracle, "oracle_", pb)
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_posteriors(oracle, "oracle_", pb)
    util.assert_arrays_exact(got, want, cr, "posteriors " + name)


def test_genotype_extraction(hmm, oracle):
    """hipstr_post_upload / _launch / _extract on the smallest golden fixture, GL, PL and PHASEDGL switched on."""
    path = min(tg.FIXTURES, key=os.path.getsize)
    pb, nv, h2a, exp = util.load_gt_fixture(path)
    run = lambda: capi.run_gt_extract(hmm, "hipstr_", pb, nv, h2a, calc_gls=True, calc_pls=True, calc_phased_gls=True)
    got = poisoned(hmm, run, "genotypes " + os.path.basename(path))[0]
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_gt_extract(oracle, "oracle_", pb, nv, h2a)
    util.assert_genotypes_exact(got, exp, cr, os.path.basename(path), verify=(oracle, pb, nv, h2a))


# =================================================================================================== assignment
@pytest.mark.parametrize("rule", [capi.ASSIGN_VCF, capi.ASSIGN_RETRACE], ids=["vcf", "retrace"])
def test_assignment_request_batch(hmm, oracle, rule):
    """A direct and a hashed first-occurrence table; at most 78 reads per unit: a wavefront per unit."""
    pb, LL, mg, seed, pool, pool_off = ta.request_inputs(oracle)
    what = "assignment, request batch, rule %d" % rule
    got = poisoned(hmm, lambda: capi.run_assign(hmm, pb, seed, pool_index=pool, pool_off=pool_off, rule=rule), what)[0]
    assert got["rc"] == 0
    ta.check(got, pb, LL, mg, seed, what, requests=True, pool_index=pool, pool_off=pool_off, rule=rule)


@pytest.mark.parametrize("rule", [capi.ASSIGN_VCF, capi.ASSIGN_RETRACE], ids=["vcf", "retrace"])
@pytest.mark.parametrize("mode", list(ta.EDGE_SIZES))
def test_assignment_edges(hmm, oracle, mode, rule):
    """Both launch modes (256 reads per unit at most / 257), with the request list on: seven pools shared by all samples."""
    sizes = ta.EDGE_SIZES[mode]
    pb, LL, seed, reverse = ta.edges_inputs(sizes)
    n = int(pb.a["read_off"][-1])
    plan = (C.c_int64 * 4)()
    capi._sig(hmm.hipstr_debug_assign_plan, C.c_int, [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)])
    assert hmm.hipstr_debug_assign_plan(max(sizes), len(sizes), 21, n, plan) == 0 and plan[0] == (4 if max(sizes) > 256 else 1)
    pool = ((np.arange(n) * 5) % 7).astype(np.int32); pool_off = np.array([0, 7], np.int32)
    mg = ta.oracle_map(oracle, pb)
    what = "assignment, edges %s, rule %d" % (mode, rule)
    run = lambda: capi.run_assign(hmm, pb, seed, reverse=reverse, pool_index=pool, pool_off=pool_off, rule=rule)
    got = poisoned(hmm, run, what)[0]
    assert got["rc"] == 0
    ta.check(got, pb, LL, mg, seed, what, requests=True, reverse=reverse, pool_index=pool, pool_off=pool_off, rule=rule)


# =================================================================================================== EM
def _em_case(hmm, oracle, kw, want, what):
    got = poisoned(hmm, lambda: capi.run_em(hmm, "hipstr_", **kw), what)[0]
    te._exact(got, want if want is not None else capi.run_em(oracle, "oracle_", **kw), oracle, kw, what)


def test_em_smallest_golden_fixture(hmm, oracle):
    path = min(teo.FIXTURES, key=os.path.getsize)
    kw, d = teo.load(path)
    _em_case(hmm, oracle, kw, (d["expect_trained"], d["expect_stutter"], d["expect_n_iter"], d["expect_final_ll"]), "EM " + os.path.basename(path))


def test_em_loci_that_converge_at_very_different_rounds(hmm, oracle):
    """The shape of tests/test_em_gpu.py's test of that name: the lists of loci and units still training are compacted on the device."""
    kw = em_case(123, n_loci=60, samples=(4, 120), reads_per_sample=(2, 9))
    _em_case(hmm, oracle, kw, None, "EM, 60 loci, 4-120 samples")


# =================================================================================================== stream
def test_stream_created_after_a_poison(hmm, oracle):
    """Two slots, six small batches, collected in order: the slots' workspaces and result blocks are poisoned blocks, each used three times."""
    pieces = [capi.SynthBatch(n_loci=1 + i % 2, reads_per_locus=12 + 5 * i, n_str_alleles=3 + i % 3, seed=40 + i) for i in range(6)]
    def run():
        st = capi.Stream(hmm, slots=2, batch_alignments=1)                 # every submission a batch of its own
        try:
            for p in pieces:
                st.submit(p.ptr)
            st.flush()
            got = [st.next(fill=FILL) for _ in pieces]
            assert st.next() is None
        finally:
            st.close()
        assert [g[0] for g in got] == list(range(len(pieces)))
        return [(g[1], g[2]) for g in got]
    got = poisoned(hmm, run, "stream")[0]
    for i, p in enumerate(pieces):
        one = capi.run_align(hmm, "hipstr_hmm_", p.ptr, fill=FILL)
        same_bits(got[i], one, "stream, batch %d against the one-shot call" % i)
        want = capi.run_align(oracle, "oracle_", p.ptr, fill=FILL)
        assert np.array_equal(got[i][1], want[1]) and np.array_equal(got[i][0], want[0]), "stream, batch %d against the oracle" % i


@pytest.mark.parametrize("name", ["no_reads_between_S3", "samples_without_reads", "alleles_M+1"])
def test_em_idle_scratch(hmm, oracle, name):
    """tests/em_route_cases.py: a locus without reads between two ordinary ones, samples without reads, and one allele more than a sweep of
    the allele-frequency scans holds (the second sweep uses one lane's worth of the LDS tiles; the rest idles) — where a stale read would show."""
    import em_route_cases as ec
    kw = ec.cases(ec.limits(hmm))[name].kw
    _em_case(hmm, oracle, kw, None, "EM route case " + name)

