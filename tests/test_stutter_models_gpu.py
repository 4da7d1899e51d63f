"""GPU: every stage that reads a stutter model, under per-locus, asymmetric models (tests/stutter_models.py) — the forward pass on every
kernel route, a locus next to neighbours with other models, the device's constants after a change of model, the traceback in its three
forms, the stream and multi-device front ends, and the device forms of the pooler's and the haplotype generator's output batches.
Every comparison is bit for bit, with the oracle (whose agreement with the compiled reference under these models is pinned on the CPU by
the stutter_models_* fixtures of tests/golden)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hipstr_amd import capi, shard
import stutter_models as sm
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = -3.25
ALL = sm.NON_DEFAULT + ["default"]      # ten models; a batch of n loci under rotate(ALL, k) has n different ones


def both(hmm, oracle, b):
    """(device result, oracle result) of a batch, each (aln_probs, seeds)."""
    want = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
    got = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL)
    return got, want


def same(got, want):
    return np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def where_it_differs(b, got, want):
    """The loci (with their models) whose rows differ: what a failure should name."""
    m = b.arrays["stutter"].reshape(-1, 6)
    bad = [l for l in range(len(m)) if not np.array_equal(sm.locus_rows(b, got[0], l), sm.locus_rows(b, want[0], l))]
    return "seeds equal: %s; loci that differ: %s" % (np.array_equal(got[1], want[1]), [(l, int(b.arrays["period"][l]), m[l].tolist()) for l in bad])


# ---------------------------------------------------------------------------------------------------------------- a. the kernel routes
ROUTES = {
    # name: (models' rotation, generator switches, generator shape, library switch, share of kind-3 alleles demanded)
    "periodic":       (0, {}, dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=401), None, None),
    "host_tables":    (1, {}, dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=401), ("HIPSTR_HOST_TABLES", "1"), None),
    "pw":             (2, dict(imperfect=1.0), dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=402), None, None),
    "pw_flank_masks": (3, dict(imperfect=1.0), dict(n_loci=7, reads_per_locus=16, n_str_alleles=8, n_flank_opts=3, mask_rate=0.3, seed=412), None, None),
    "rp_inherit2":    (4, dict(inherit=2, imperfect=0.0), dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=403), None, 0.3),
    "rp_inherit3":    (5, dict(inherit=3, imperfect=0.0), dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=404), None, 0.3),
    "long_sides":     (6, dict(imperfect=1.0), dict(n_loci=7, reads_per_locus=10, n_str_alleles=8, read_len=300, flank_len=140, str_bp=50, seed=405), None, None),
    "per_read":       (7, dict(imperfect=0.05), dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, seed=406), ("HIPSTR_STR_GROUP", "0"), None),
    "redo_all":       (8, dict(imperfect=0.1), dict(n_loci=7, reads_per_locus=20, n_str_alleles=32, seed=407), ("HIPSTR_DEBUG_REDO", "1"), None),
    "redo_third":     (9, dict(imperfect=0.1), dict(n_loci=7, reads_per_locus=20, n_str_alleles=32, seed=407), ("HIPSTR_DEBUG_REDO", "3"), None),
    "short_blocks":   (0, dict(imperfect=1.0), dict(n_loci=7, reads_per_locus=20, n_str_alleles=16, str_bp=14, seed=408), None, None),
    "period_1":       (1, dict(period=1), dict(n_loci=7, reads_per_locus=20, n_str_alleles=8, seed=409), None, None),
    "period_7":       (2, dict(period=7), dict(n_loci=7, reads_per_locus=20, n_str_alleles=8, seed=410), None, None),
    "period_9":       (3, dict(period=9), dict(n_loci=7, reads_per_locus=20, n_str_alleles=8, seed=411), None, None),
    "ws_chunks":      (4, {}, dict(n_loci=7, reads_per_locus=30, n_str_alleles=12, n_flank_opts=2, mask_rate=0.15, seed=44), ("HIPSTR_WS_GIB", "0.0005"), None),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_forward_pass_on_every_route(hmm, oracle, monkeypatch, route):
    """Seven loci, seven models, one kernel route (the shapes of tests/test_hmm_gpu.py's route tests, shrunk): device == oracle."""
    rot, switches, kw, env, kind3 = ROUTES[route]
    b = sm.synth(sm.rotate(ALL, rot), **switches, **kw)
    assert len({tuple(m) for m in b.arrays["stutter"].reshape(-1, 6).tolist()}) == 7
    want = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
    if env:
        monkeypatch.setenv(*env)
        if env[0] == "HIPSTR_WS_GIB":        # the budget cuts this batch into many chunks of reads
            assert len(capi.launch_plan(hmm, b.ptr, float(env[1]))["chunks"]) >= 4
    got = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL)
    assert (want[1] >= 0).sum() >= 50
    assert same(got, want), where_it_differs(b, got, want)
    if kind3 is not None:         # the case keeps exercising hs_str_group_kernel_rp
        dev = hmm.hipstr_hmm_upload(b.ptr)
        assert dev
        kinds = (C.c_int64 * 4)()
        hmm.hipstr_debug_allele_kinds(dev, kinds)
        hmm.hipstr_hmm_free(dev)
        assert kinds[3] > kind3 * sum(kinds), list(kinds)


@pytest.mark.parametrize("threads", [1, 4])
def test_forward_pass_with_one_and_with_many_prep_fragments(threads):
    """HIPSTR_HOST_THREADS is read once per process: a process each.  14 loci: with 4 host threads prepare_batch builds 12 fragments on 3
    threads and merges them (the pmf offsets of every STR option are rebased); with one thread there is no fragment."""
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from hipstr_amd import capi; import stutter_models as sm\n"
            "hmm = capi.load_hmm(); ora = capi.load_oracle(); assert hmm.hipstr_hmm_init(0) == 0\n"
            "for rot, sw in ((0, {}), (3, dict(imperfect=1.0)), (6, dict(inherit=2))):\n"
            "    b = sm.synth(sm.rotate(sm.NON_DEFAULT + ['default'], rot), n_loci=14, reads_per_locus=10, n_str_alleles=8, seed=420 + rot, **sw)\n"
            "    want, ws = capi.run_align(ora, 'oracle_', b.ptr, fill=-3.25)\n"
            "    got, gs = capi.run_align(hmm, 'hipstr_hmm_', b.ptr, fill=-3.25)\n"
            "    assert np.array_equal(gs, ws) and np.array_equal(got, want), (rot, sw)\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, HIPSTR_HOST_THREADS=str(threads))
    out = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


# ---------------------------------------------------------------------------------------------------------------- b. neighbours
@pytest.fixture(scope="module")
def fourteen(oracle):
    """14 loci (interrupted alleles among them), 10 models: (batch, model names, oracle's result)."""
    models = sm.rotate(ALL, 5)
    b = sm.synth(models, imperfect=0.3, n_loci=14, reads_per_locus=12, n_str_alleles=8, seed=430)
    return b, models, capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)


def test_a_locus_does_not_see_its_neighbours_models(hmm, oracle, fourteen):
    b, models, want = fourteen
    got = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL)
    assert same(got, want), where_it_differs(b, got, want)
    a = b.arrays
    for l in range(14):         # every locus alone: the rows it had in the batch
        one = shard.batch_from_arrays(shard.subset_arrays(a, l, l + 1))
        p, s = capi.run_align(hmm, "hipstr_hmm_", one.ptr, fill=FILL)
        assert np.array_equal(p, sm.locus_rows(b, got[0], l)) and np.array_equal(s, got[1][a["read_off"][l]:a["read_off"][l + 1]]), l
    # the same sequences with every model moved on by one locus
    r = sm.with_models(b, sm.rotate(models, 1))
    got_r, want_r = both(hmm, oracle, r)
    assert same(got_r, want_r), where_it_differs(r, got_r, want_r)
    assert not np.array_equal(want_r[0], want[0])


# ---------------------------------------------------------------------------------------------------------------- c. a changed model
def _resident(hmm, b):
    n_reads, n_out, _ = capi.batch_dims(b.ptr)
    dev = hmm.hipstr_hmm_upload(b.ptr)
    assert dev, hmm.hipstr_last_error()
    assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error()
    p = np.full(n_out, FILL); s = np.full(n_reads, -7, np.int32)
    assert hmm.hipstr_hmm_fetch(dev, p.ctypes.data_as(capi._f64p), s.ctypes.data_as(capi._i32p)) == 0, hmm.hipstr_last_error()
    hmm.hipstr_hmm_free(dev)
    return p, s


@pytest.mark.parametrize("switches", [dict(imperfect=0.0), dict(imperfect=1.0), dict(inherit=2)], ids=["periodic", "pw", "rp"])
def test_the_constants_follow_a_changed_model(hmm, oracle, switches):
    """The same sequences under M, rotate(M, 1), M again, from one process — through the one-shot call and through upload / align / fetch
    with a fresh upload per model: a cache that kept an earlier model's constants would show."""
    M = sm.rotate(ALL, 2)
    base = sm.synth(M, n_loci=7, reads_per_locus=12, n_str_alleles=8, seed=440, **switches)
    lists = [M, sm.rotate(M, 1), M]
    batches = [sm.with_models(base, m) for m in lists]
    wants = [capi.run_align(oracle, "oracle_", x.ptr, fill=FILL) for x in batches[:2]]
    wants.append(wants[0])
    assert not np.array_equal(wants[0][0], wants[1][0])
    for call in (lambda x: capi.run_align(hmm, "hipstr_hmm_", x.ptr, fill=FILL), lambda x: _resident(hmm, x)):
        gots = [call(x) for x in batches]
        for i in range(3):
            assert same(gots[i], wants[i]), (i, where_it_differs(batches[i], gots[i], wants[i]))
        assert same(gots[2], gots[0])
    # rows the aligner leaves alone keep the caller's values in the resident form too
    assert np.array_equal(gots[0][0] == FILL, wants[0][0] == FILL)


# ---------------------------------------------------------------------------------------------------------------- d. traceback
TRACE_KINDS = {"periodic": (0, dict(imperfect=0.0), 450), "pw": (3, dict(imperfect=1.0), 451), "rp": (6, dict(inherit=2, imperfect=0.0), 452)}


@pytest.fixture(scope="module")
def trace_cases(oracle):
    """kind -> (batch, req_read, req_allele, hap_to_ref of all loci, the oracle's records locus by locus), made on first use and shared:
    every allele of 6 seeded reads per locus of a 7-locus batch under 7 models, in one shuffled request list."""
    made = {}
    def get(kind):
        if kind not in made:
            rot, switches, seed = TRACE_KINDS[kind]
            b = sm.synth(sm.rotate(ALL, rot), n_loci=7, reads_per_locus=12, n_str_alleles=8, seed=seed, **switches)
            a = b.arrays
            _, seeds = capi.run_align(oracle, "oracle_", b.ptr)
            rr, aa, want, h2r_all = [], [], [], []
            for l in range(7):
                r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1]); A = int(a["hap_off"][l + 1] - a["hap_off"][l])
                one = shard.batch_from_arrays(shard.subset_arrays(a, l, l + 1))
                h2r = util.synthetic_hap_to_ref(oracle, one.ptr); h2r_all += h2r
                lr = [r for r in range(r0, r1) if seeds[r] >= 0][:6]
                assert len(lr) == 6
                q_r = [r for r in lr for _ in range(A)]; q_a = [k for _ in lr for k in range(A)]
                want += capi.run_trace(oracle, "oracle_", one.ptr, [r - r0 for r in q_r], q_a, h2r, cap=1 << 21)
                rr += q_r; aa += q_a
            order = np.random.default_rng(seed).permutation(len(rr))
            sizes = [w["stutter_size"] for w in want if w["stutter_size"] != -100000]
            assert sum(x > 0 for x in sizes) >= 20 and sum(x < 0 for x in sizes) >= 20
            made[kind] = (b, [rr[i] for i in order], [aa[i] for i in order], h2r_all, [want[i] for i in order])
        return made[kind]
    return get


@pytest.mark.parametrize("form", ["host_replay", "device_assembly", "resident"])
@pytest.mark.parametrize("kind", sorted(TRACE_KINDS))
def test_traceback_under_per_locus_models(hmm, trace_cases, kind, form):
    """hipstr_hmm_trace, hipstr_hmm_trace_ex(HIPSTR_TRACE_ASSEMBLE_DEVICE) and hipstr_hmm_trace_resident + hipstr_trace_dev_fetch: one call with
    the requests of all loci, against the oracle's records of every locus on its own cut."""
    b, rr, aa, h2r, want = trace_cases(kind)
    if form == "host_replay":
        got = capi.run_trace(hmm, "hipstr_hmm_", b.ptr, rr, aa, h2r, cap=1 << 22)
    elif form == "device_assembly":
        got = capi.run_trace(hmm, "hipstr_hmm_", b.ptr, rr, aa, h2r, cap=1 << 22, flags=capi.TRACE_ASSEMBLE_DEVICE)
    else:
        td = capi.run_trace_resident(hmm, b.ptr, rr, aa, h2r)
        got = capi.unpack_trace(capi.trace_dev_fetch(hmm, td), len(rr))
        td.close()
    util.assert_traces_equal(got, want, "%s %s" % (kind, form))


# ---------------------------------------------------------------------------------------------------------------- e. stream and multi
@pytest.fixture(scope="module")
def twenty(oracle):
    """20 loci with masks under 10 models, cut into tickets of 1 to 3 loci: (batch, pieces, the oracle's result per piece and whole)."""
    b = sm.synth(sm.rotate(ALL, 7), imperfect=0.3, n_loci=20, reads_per_locus=10, n_str_alleles=8, n_flank_opts=2, mask_rate=0.2, seed=460)
    rng = np.random.default_rng(460)
    cuts = [0]
    while cuts[-1] < 20:
        cuts.append(min(20, cuts[-1] + int(rng.integers(1, 4))))
    a = b.arrays
    pieces = [shard.batch_from_arrays(shard.subset_arrays(a, lo, hi)) for lo, hi in zip(cuts[:-1], cuts[1:])]
    whole = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
    off = capi.batch_dims(b.ptr)[2]
    want = [(whole[0][off[lo]:off[hi]], whole[1][a["read_off"][lo]:a["read_off"][hi]]) for lo, hi in zip(cuts[:-1], cuts[1:])]
    return b, pieces, want, whole


@pytest.mark.parametrize("threshold,slots", [(1, 2), (3000, 3), (1 << 40, 2)])
def test_stream_tickets_under_per_locus_models(hmm, twenty, threshold, slots):
    """tests/test_stream_gpu.py's scheme — every ticket its own batch, batches of a few tickets, one batch flushed by next() — against
    the oracle and against the one-shot call of each piece: whatever batch a locus lands in, it keeps its model."""
    b, pieces, want, _ = twenty
    st = capi.Stream(hmm, slots=slots, batch_alignments=threshold)
    got = []
    for i, p in enumerate(pieces):
        assert st.submit(p.ptr) == i
        if i % 4 == 3:
            got.append(st.next(fill=FILL))
    while True:
        r = st.next(fill=FILL)
        if r is None:
            break
        got.append(r)
    st.close()
    assert [g[0] for g in got] == list(range(len(pieces)))
    for (t, probs, seeds), (wp, ws), p in zip(got, want, pieces):
        assert np.array_equal(probs, wp) and np.array_equal(seeds, ws), "ticket %d" % t
        if threshold == 3000:
            assert same(capi.run_align(hmm, "hipstr_hmm_", p.ptr, fill=FILL), (wp, ws)), "one-shot call of ticket %d" % t


def test_submit_each_under_per_locus_models(hmm, twenty):
    b, _, _, whole = twenty
    n_reads, n_out, _ = capi.batch_dims(b.ptr)
    st = capi.Stream(hmm, batch_alignments=700)
    assert st.submit_each(b.ptr) == 0
    probs = np.full(n_out, FILL); seeds = np.full(n_reads, -7, np.int32)
    assert st.collect(20, probs, seeds) == (n_out, n_reads)
    assert st.next() is None
    st.close()
    assert same((probs, seeds), whole), where_it_differs(b, (probs, seeds), whole)


def test_multi_streams_under_per_locus_models(hmm, twenty):
    """hipstr_multi_*: two streams on device 0, as tests/test_stream_gpu.py::test_multi_retry_after_too_small_buffer_keeps_the_order has
    them; blocks of a ticket or two alternate between the streams."""
    from test_stream_gpu import _multi_sigs
    lib = hmm; _multi_sigs(lib)
    b, pieces, want, _ = twenty
    devs = np.zeros(2, np.int32)
    m = lib.hipstr_multi_open(2, devs.ctypes.data_as(capi._i32p), 300, None)
    assert m, lib.hipstr_last_error()
    for i, p in enumerate(pieces):
        assert lib.hipstr_multi_submit(m, p.ptr) == i
    for i, (wp, ws) in enumerate(want):
        t = C.c_int64(); no = C.c_int64(); nr = C.c_int64()
        assert lib.hipstr_multi_next_size(m, C.byref(t), C.byref(no), C.byref(nr)) == 0 and t.value == i and no.value == wp.size
        probs = np.full(max(no.value, 1), FILL); seeds = np.full(max(nr.value, 1), -7, np.int32)
        assert lib.hipstr_multi_next(m, C.byref(t), probs.ctypes.data_as(capi._f64p), probs.size, seeds.ctypes.data_as(capi._i32p), seeds.size) == 0, lib.hipstr_last_error()
        assert t.value == i and np.array_equal(probs[:no.value], wp) and np.array_equal(seeds[:nr.value], ws), "ticket %d" % i
    assert lib.hipstr_multi_next(m, None, None, 0, None, 0) == 2
    lib.hipstr_multi_close(m)


# ---------------------------------------------------------------------------------------------------------------- f. device plumbing
def test_pooled_batch_on_the_device_keeps_the_models(hmm):
    b = sm.synth(sm.NON_DEFAULT, n_loci=9, reads_per_locus=6, n_str_alleles=4, seed=311)          # tests/test_stutter_models.py's batch
    host = capi.PooledBatch(hmm, b.ptr, capi.POOL_ON_HOST); dev = capi.PooledBatch(hmm, b.ptr, 0)
    h, d = host.arrays(), dev.arrays()
    assert np.array_equal(d["stutter"], h["stutter"]) and np.array_equal(d["stutter"], b.arrays["stutter"]) and np.array_equal(d["period"], h["period"])
    host.close(); dev.close()


def test_hapgen_batch_on_the_device_copies_the_model_of_the_source_locus(hmm):
    from test_stutter_models import hapgen_inputs
    b, rq, models = hapgen_inputs()
    host = capi.HapgenBatch(hmm, b.ptr, rq, capi.HAPGEN_ON_HOST); dev = capi.HapgenBatch(hmm, b.ptr, rq, 0)
    assert dev.locus.tolist() == host.locus.tolist() and any(k != l for k, l in enumerate(dev.locus.tolist()))
    assert np.array_equal(dev.arrays()["stutter"], host.arrays()["stutter"])
    assert dev.arrays()["stutter"].reshape(-1, 6).tolist() == [models[l] for l in dev.locus.tolist()]
    host.close(); dev.close()
