"""GPU: hipstr_em_train_dev (include/hipstr_hmm.h) — the stutter model retrained from a resident traceback result: the reads
SeqStutterGenotyper::recompute_stutter_models (seq_stutter_genotyper.cpp:1542-1581) hands to EMStutterGenotyper::train are selected,
compacted and prepared on the device (hipstr_amd/csrc/em_input.hip) and hipstr_em_train's loop runs on them.

The yardstick is the host form on the same commit: hipstr_em_train on the batch hipstr_em_batch_from_traces builds from
hipstr_trace_dev_fetch(td, SCALARS | STR_SEQ) — outputs, return codes and messages equal bit for bit and byte for byte — and, for the
numbers, the oracle's EM on that batch under the two-level contract of tests/test_em_gpu.py (util.assert_arrays_exact).  The device-built
preparation (hipstr_debug_em_input_fetch) must be em_prepare's: the compact arrays are the host batch's, the alleles are the distinct
sizes other than ref_allele ascending behind ref_allele, and the initial log frequencies are init_log_gt_priors' bits
(em_stutter_genotyper.cpp:10-20; hipstr_debug_em_input_fetch on the host route returns em_prepare's own).  Handles come from
capi.trace_dev_from_host unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from hipstr_amd import capi
import em_trace_cases as etc
import test_poison_gpu as tp
import util

pytestmark = pytest.mark.gpu

TABLE = 10000          # entries of the table of integer logarithms (mathops.cpp:13-21)


class Resident:
    """A case on the device: the posterior run (uploaded, launched on request) and the trace handle."""

    def __init__(self, hmm, c, launch=False, trace=None):
        self.hmm, self.c = hmm, c
        self.pd = hmm.hipstr_post_upload(c.pb.ptr, None); assert self.pd, hmm.hipstr_last_error().decode()
        if launch:
            assert hmm.hipstr_post_launch(self.pd, None) == 0
        self.td = capi.trace_dev_from_host(hmm, c.trace if trace is None else trace, c.n_req)

    def train(self, **kw):
        c = self.c
        a = dict(seed=c.seed, read_req=c.read_req, req_read=c.req_read, td=self.td, bptr=C.pointer(c.pooled)); a.update(kw)
        return capi.em_train_dev(self.hmm, self.pd, c.n_loci, a.pop("bptr"), a.pop("seed"), a.pop("read_req"), a.pop("req_read"), a.pop("td"), **a)

    def fetch(self, **kw):
        c = self.c
        return capi.em_input_fetch(self.hmm, self.pd, c.n_loci, c.n_reads, C.pointer(c.pooled), c.seed, c.read_req, c.req_read, self.td, **kw)

    def close(self):
        self.td.close(); self.hmm.hipstr_post_free(self.pd)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False


def host_form(hmm, c, td, **kw):
    """The host chain: fetch the two groups, hipstr_em_batch_from_traces, (the caller runs hipstr_em_train)."""
    tr = capi.trace_dev_fetch(hmm, td, capi.TRACE_F_SCALARS | capi.TRACE_F_STR_SEQ, null_others=True)
    return etc.host_batch(hmm, c, trace=tr, **kw)


def check_equal(hmm, oracle, c, what, launch=False, **kw):
    """hipstr_em_train_dev == hipstr_em_train on the host-built batch (bits) == the oracle (two-level contract); returns the device's results."""
    with Resident(hmm, c, launch=launch) as R:
        got = R.train(**kw)
        batch = host_form(hmm, c, R.td, **kw)
    assert etc.same_batch(batch, etc.restate(c)), what
    ekw = etc.em_kw(c, batch, **kw)
    want = capi.run_em(hmm, "hipstr_", **ekw)
    for g, w, nm in zip(got[:4], want, ("trained", "stutter", "n_iter", "final_ll")):
        assert np.array_equal(g, w), "%s: %s differs from hipstr_em_train on the host-built batch" % (what, nm)
    ora = capi.run_em(oracle, "oracle_", **ekw)
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_em(oracle, "oracle_", **ekw)
    util.assert_arrays_exact(got[:4], ora, cr, what)
    assert np.array_equal(got[4], batch["read_off"]), what
    n_sizes = [1 + len(set(batch["num_bps"][batch["read_off"][l]:batch["read_off"][l + 1]].tolist()) - {kw.get("ref_allele", 0)}) for l in range(c.n_loci)]
    assert list(got[5]) == n_sizes, what
    return got, batch


def _run(rng, n, frac, sizes):
    """n reads of a sample: each enters with probability frac (size from `sizes`), else it is one of the reads that do not."""
    out = []
    for _ in range(n):
        if rng.random() < frac:
            out.append(("in", int(rng.choice(sizes))))
        else:
            k = ("start", "stop", "seed", "noreq")[int(rng.integers(0, 4))]
            out.append((k,) if k == "noreq" else (k, int(rng.choice(sizes))))
    return out


def main_case():
    """6 loci of 1 to 5 samples; per-sample runs of 0, 1, 3, 7, 63, 64 and 65 reads (1.0/3 and 1.0/7 are inexact: the order of the prior sums
    shows); entering fractions 0, partial and all; one haploid locus; periods 1, 2 and 6."""
    rng = np.random.default_rng(2024)
    sz = lambda p, base=24: [base + p * k for k in (-2, -1, 0, 0, 0, 1, 2)] + [base + 1]       # multiples of the period and one out of frame
    return etc.build([
        dict(period=2, runs=[_run(rng, 63, 1.0, sz(2)), _run(rng, 64, 0.6, sz(2)), _run(rng, 65, 1.0, sz(2)), [], _run(rng, 1, 1.0, sz(2))]),
        dict(period=6, runs=[_run(rng, 3, 1.0, sz(6)), _run(rng, 7, 1.0, sz(6)), _run(rng, 65, 0.5, sz(6))]),
        dict(period=1, haploid=True, runs=[_run(rng, 7, 1.0, sz(1)), _run(rng, 3, 1.0, sz(1)), _run(rng, 64, 1.0, sz(1)), _run(rng, 0, 1.0, sz(1))]),
        dict(period=2, runs=[_run(rng, 64, 0.0, sz(2)), _run(rng, 7, 0.0, sz(2))]),                # reads, none enters
        dict(period=6, runs=[_run(rng, 63, 0.7, sz(6))]),
        dict(period=2, runs=[_run(rng, 3, 1.0, sz(2, 0)), _run(rng, 7, 0.8, sz(2, 0)), _run(rng, 1, 1.0, sz(2, 0)), _run(rng, 65, 0.9, sz(2, 0))]),
    ], seed=3)


# ------------------------------------------------------------------ 1. equality with the host form and the oracle
def test_equals_host_form_and_oracle(hmm, oracle):
    c = main_case()
    got, batch = check_equal(hmm, oracle, c, "6 loci")
    R = np.diff(batch["read_off"])
    assert R[3] == 0 and R.sum() > 300
    # launched or not, and ref_allele = the most frequent size, make no difference to the contract
    check_equal(hmm, oracle, c, "6 loci, launched, ref_allele 24", launch=True, ref_allele=24)
    check_equal(hmm, oracle, c, "6 loci, max_iter 3", max_iter=3)


# ------------------------------------------------------------------ 2. the device-built preparation
def check_prepared(hmm, c, what, route, ref_allele=0):
    """hipstr_debug_em_input_fetch against the host batch and a restatement of em_prepare; then both entry points train the same."""
    with Resident(hmm, c) as R:
        f = R.fetch(ref_allele=ref_allele)
        batch = host_form(hmm, c, R.td, ref_allele=ref_allele)
        got = R.train(ref_allele=ref_allele)
    assert f["route"] == route, what
    assert np.array_equal(f["read_off"], batch["read_off"]), what
    for k in ("num_bps", "sample_label", "log_p1", "log_p2"):
        assert np.array_equal(f[k], batch[k]), "%s: %s" % (what, k)
    so = [0]; sizes = []; obs = []; freq = []
    for l in range(c.n_loci):
        r0, r1 = int(batch["read_off"][l]), int(batch["read_off"][l + 1])
        nb = batch["num_bps"][r0:r1]; lab = batch["sample_label"][r0:r1]
        al = [ref_allele] + sorted(set(nb.tolist()) - {ref_allele})
        idx = {v: i for i, v in enumerate(al)}
        ob = [idx[v] for v in nb.tolist()]
        per = np.bincount(lab, minlength=c.n_samples[l])
        g = [1.0] * len(al)
        for o, s in zip(ob, lab.tolist()):
            g[o] += 1.0 / float(per[s])                                  # in read order (em_stutter_genotyper.cpp:13-16)
        tot = 0.0
        for x in g:
            tot += x
        sizes += al; obs += ob; freq.append((np.asarray(g), tot)); so.append(len(sizes))
    assert list(f["size_off"]) == so and list(f["sizes"]) == sizes and list(f["obs"]) == obs, what
    # the logarithms are cr_math.h's on both sides: compared with what the host's em_prepare leaves (the debug entry on the host route returns
    # em_prepare's arrays; on the device route the same numbers must come from the kernel) through the correctly rounded log of the library
    gs = np.concatenate([g for g, _ in freq] + [np.asarray([t for _, t in freq])])
    lg = np.zeros(len(gs))
    assert hmm.hipstr_debug_cr_math(1, gs.ctypes.data_as(capi._f64p), lg.ctypes.data_as(capi._f64p), len(gs)) == 0
    want = np.concatenate([lg[so[l]:so[l + 1]] - lg[len(sizes) + l] for l in range(c.n_loci)]) if sizes else np.zeros(0)
    assert np.array_equal(f["log_freq"].view(np.uint64), want.view(np.uint64)), "%s: initial log allele frequencies" % what
    want_em = capi.run_em(hmm, "hipstr_", **etc.em_kw(c, batch, ref_allele=ref_allele))
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], want_em)), what
    assert list(got[5]) == list(np.diff(so)), what
    return f


def _one_locus(sizes_per_sample, period=2, **kw):
    return etc.build([dict(period=period, runs=[[("in", s) for s in run] for run in sizes_per_sample], **kw)], seed=9)


PREP = {
    "all_ref": (_one_locus([[12, 12, 12], [12]]), 12),
    "ref_observed": (_one_locus([[10, 12, 14, 12, 12, 10, 16], [12, 14, 12]]), 12),
    "ref_unobserved": (_one_locus([[10, 14, 14, 10, 10, 16, 14], [14, 14, 10]]), 0),
    "ref_between": (_one_locus([[8, 10, 14, 16, 14, 10, 10], [16, 8, 14]]), 12),
    "duplicates_across_samples": (_one_locus([[10, 12, 12], [12, 10, 14], [14, 14, 10], [], [10]]), 11),
    "negative_size": (_one_locus([[-6, 0, 2, -6, 0, 0, 2], [0, -6, 0]]), 0),
    "word_edges": (_one_locus([[-50, -50 + 31, -50 + 32, -50 + 33, -50 + 63, -50 + 64, -50 + 65], [-50, -50 + 64, -50 + 32, -50 + 31, -50 + 33, -50 + 63, -50 + 65, -50]]), -48),
    "span_table_minus_1": (_one_locus([[0, TABLE - 1, 0, 0, 0, TABLE - 1, 6], [0, 0, 6]], period=6), 0),
}


@pytest.mark.parametrize("name", sorted(PREP))
def test_device_built_preparation(hmm, name):
    c, ref = PREP[name]
    f = check_prepared(hmm, c, name, "device", ref_allele=ref)
    assert f["sizes"][0] == ref


def test_wide_span_takes_the_host_route_and_still_trains(hmm, oracle):
    """A span of exactly the table's length with period 6: every effective difference stays inside the table, the locus is legal — prepared
    by em_prepare on the fetched compact arrays — next to a locus the device would have prepared."""
    c = etc.build([dict(period=6, runs=[[("in", s) for s in (0, TABLE, 0, 0, 0, TABLE, 6)], [("in", 0), ("in", 0), ("in", 6)]]),
                   dict(period=2, runs=[[("in", s) for s in (10, 12, 12, 14, 12)]])], seed=4)
    f = check_prepared(hmm, c, "span == table", "host")
    assert list(f["sizes"]) == [0, 6, TABLE, 0, 10, 12, 14]
    check_equal(hmm, oracle, c, "span == table")


# ------------------------------------------------------------------ 3. refusals and messages
def _refused_like_host(hmm, c, what, **kw):
    """Both forms refuse, with the same return code and message, and the resident call writes nothing."""
    with Resident(hmm, c) as R:
        with pytest.raises(RuntimeError) as dev:
            R.train(**kw)
        with pytest.raises(RuntimeError) as host:
            batch = host_form(hmm, c, R.td, **kw)
            capi.run_em(hmm, "hipstr_", **etc.em_kw(c, batch, **kw))
    d = str(dev.value).split(": ", 1)[1]; h = str(host.value).split(" ", 3)[3] if "em_train failed" in str(host.value) else str(host.value).split(": ", 1)[1]
    assert d == h, "%s: %r != %r" % (what, d, h)
    assert str(dev.value).split(":")[0].endswith("rc=1")
    _untouched(dev)
    return d


def _untouched(e):
    o = e.value.outputs
    assert np.all(o["trained"] == 0xAA) and np.all(np.isnan(o["stutter"])) and np.all(o["n_iter"] == capi.UNTOUCHED) and np.all(np.isnan(o["final_ll"]))
    assert np.all(o["em_read_off"] == capi.UNTOUCHED) and np.all(o["n_sizes"] == capi.UNTOUCHED)


def test_refusals_of_the_em_are_the_hosts(hmm):
    # a period of 0 in the second locus while the first has sizes too far apart: the first locus' message wins
    c = etc.build([dict(period=2, runs=[[("in", 0), ("in", 2 * TABLE), ("in", 2)]]), dict(period=0, runs=[[("in", 4)]])])
    assert "too far apart" in _refused_like_host(hmm, c, "two bad loci")
    c = etc.build([dict(period=0, runs=[[("in", 0), ("in", 2)]]), dict(period=2, runs=[[("in", 0), ("in", 2 * TABLE)]])])
    assert "period" in _refused_like_host(hmm, c, "two bad loci, the other way round")
    c = etc.build([dict(period=12, runs=[[("in", 4)]])])
    assert "period" in _refused_like_host(hmm, c, "period 12")
    # 9 998 distinct sizes (and the reference size) in one locus of one sample
    c = etc.build([dict(period=1, runs=[[("in", s) for s in range(1, TABLE - 1)]])])
    assert "too many distinct allele sizes" in _refused_like_host(hmm, c, "9998 sizes")
    # one fewer is legal (9 997 sizes and the reference size): the device prepares it, frequencies included (the loop itself is not run here:
    # its arrays grow with the square of the allele count)
    c = etc.build([dict(period=1, runs=[[("in", s) for s in range(1, TABLE - 2)]])])
    with Resident(hmm, c) as R:
        f = R.fetch()
    assert f["route"] == "device" and list(f["sizes"]) == list(range(TABLE - 2)) and list(f["obs"]) == list(range(1, TABLE - 2))
    n = TABLE - 3                                                       # reads, one per size: g = 1 + 1/n each, 1 for the reference size
    lf = np.log((1.0 + 1.0 / n) / (n + 2.0))
    assert abs(f["log_freq"][1] - lf) < 1e-12 and np.all(f["log_freq"][1:] == f["log_freq"][1]) and f["log_freq"][0] < f["log_freq"][1]
    # a locus without samples
    c = etc.build([dict(period=2, runs=[[("in", 4)]]), dict(period=2, runs=[])])
    assert "without samples" in _refused_like_host(hmm, c, "no samples")


def test_refusals_of_the_arguments(hmm):
    c = etc.build([dict(period=2, runs=[[("in", 12), ("in", 10)], [("in", 14)]]), dict(period=2, runs=[[("in", 8), ("noreq",)]])])
    with Resident(hmm, c) as R:
        def refused(word, **kw):
            with pytest.raises(RuntimeError, match=word) as e:
                R.train(**kw)
            _untouched(e)
        # n_req mismatch
        other = capi.trace_dev_from_host(hmm, dict(c.trace, **{k: c.trace[k][:c.n_req - 1] for k in ("ll", "max_index", "stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop")},
                                                   str_seq_off=c.trace["str_seq_off"][:c.n_req]), c.n_req - 1)
        refused("rq->n_req differs from the trace handle's", td=other)
        other.close()
        # a handle without the scalar group / without the str_seq offsets
        for nm in ("aln_start", "aln_stop", "stutter_size", "str_seq_off"):
            short = capi.trace_dev_from_host(hmm, dict(c.trace, **{nm: None}), c.n_req)
            refused("trace output without aln_start / aln_stop / stutter_size / str_seq_off", td=short)
            short.close()
        # read_req out of range, another locus' request, other tables
        for bad in (c.n_req, -2):
            rr = c.read_req.copy(); rr[1] = bad
            refused(r"read_req outside \[-1, n_req\)", read_req=rr)
        rr = c.read_req.copy(); rr[0] = c.n_req - 1
        refused("request belongs to another locus", read_req=rr)
        refused("pooled->n_loci differs", bptr=C.pointer(etc.pooled(1, [etc.BLK_START], [etc.BLK_END], [2], [0, c.n_req])))
        q = c.req_read.copy(); q[0], q[-1] = q[-1], q[0]
        refused("grouped by locus", req_read=q)
        for kw in (dict(seed=None), dict(read_req=None), dict(bptr=None), dict(td=None)):
            refused("null argument", **kw)
        # the messages of the shared checks are the host form's
        rr = c.read_req.copy(); rr[1] = c.n_req
        with pytest.raises(RuntimeError) as h:
            capi.em_batch_from_traces(hmm, c.pb, C.pointer(c.pooled), c.seed, rr, c.req_read, c.trace)
        with pytest.raises(RuntimeError) as d:
            R.train(read_req=rr)
        assert str(h.value).split(": ", 1)[1] == str(d.value).split(": ", 1)[1]
        # the device is as usable as before
        got = R.train()
        assert list(got[4]) == [0, 3, 4]


def test_read_without_str_data_is_refused_on_the_device(hmm):
    """Decided by the select kernel: refused, the lowest read named as the host form names it, nothing written, no fault — and the next call works."""
    c = etc.build([dict(period=2, runs=[[("in", 12), ("in", 10)], [("in", 14)]]),
                   dict(period=2, runs=[[("in", 8)] * 70 + [("nostr",)] + [("in", 8)] * 3 + [("nostr",)], [("nostr",), ("in", 6)]])])
    first = 3 + 70
    with Resident(hmm, c) as R:
        with pytest.raises(RuntimeError, match=r"read %d enters the EM but its request has no STR data" % first) as d:
            R.train()
        _untouched(d)
        with pytest.raises(RuntimeError) as h:
            host_form(hmm, c, R.td)
        assert str(h.value).split(": ", 1)[1] == str(d.value).split(": ", 1)[1]
        # the same requests, not entered with: no error
        seed = c.seed.copy(); seed[c.trace["stutter_size"][np.maximum(c.read_req, 0)] == etc.NO_STR_DATA] = -1
        got = R.train(seed=seed)
        assert list(got[4]) == [0, 3, 3 + 73 + 1]


# ------------------------------------------------------------------ 4. the chain on real records
def test_chain_on_real_records(hmm, oracle):
    """3 seeded loci of 40 pooled reads and 4 alleles: forward -> hipstr_rm_scatter -> posteriors -> hipstr_post_assign(RETRACE) ->
    hipstr_hmm_trace_resident -> hipstr_em_train_dev, against the same calls with the traces brought home and the oracle's EM."""
    rng = np.random.default_rng(5)
    sb = capi.SynthBatch(n_loci=3, reads_per_locus=40, n_str_alleles=4, seed=77)
    b = sb.ptr.contents
    A = np.diff(np.ctypeslib.as_array(b.hap_off, shape=(4,))).astype(np.int32)
    pool_off = np.ctypeslib.as_array(b.read_off, shape=(4,)).astype(np.int32)
    period = np.ctypeslib.as_array(b.period, shape=(3,)).astype(np.int32)
    P = np.diff(pool_off); extra = 8
    pool = np.concatenate([np.concatenate([np.arange(p), rng.integers(0, p, extra)]) for p in P]).astype(np.int32)
    read_off = np.concatenate([[0], np.cumsum(P + extra)]).astype(np.int32)
    n = int(read_off[-1]); S = 3
    lab = np.concatenate([np.sort(rng.integers(0, S, p + extra)) for p in P]).astype(np.int32)
    kw = dict(n_alleles=A, n_samples=np.full(3, S), read_off=read_off, sample_label=lab, log_p1=-rng.random(n), log_p2=-rng.random(n), read_weight=np.ones(n, np.int32))
    dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev, hmm.hipstr_last_error().decode()
    rm = pd = td = None
    try:
        assert hmm.hipstr_hmm_align(dev, None) == 0
        rm = capi.ReadMatrix(hmm, A, read_off, pool)
        rm.scatter(dev)
        _, seeds = rm.fetch()
        pb = capi.PostBatch(log_aln_probs=None, **kw)
        pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error().decode()
        assert hmm.hipstr_post_launch(pd, None) == 0
        asg = capi.run_assign(hmm, pd, seeds, pool_index=pool, pool_off=pool_off, rule=capi.ASSIGN_RETRACE, n_reads=n, n_samp=3 * S)
        assert asg["rc"] == 0 and asg["n_req"] > 0
        h2r = capi.hap_aln_info(hmm, "hipstr_", sb.ptr)
        td = capi.run_trace_resident(hmm, sb.ptr, asg["req_read"], asg["req_allele"], h2r)
        got = capi.em_train_dev(hmm, pd, 3, sb.ptr, seeds, asg["read_req"], asg["req_read"], td)
        # the same calls where the traces came home
        tr = capi.run_trace(hmm, "hipstr_hmm_", sb.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, unpack=False, cap=1 << 17, flags=0)
        batch = capi.em_batch_from_traces(hmm, pb, sb.ptr, seeds, asg["read_req"], asg["req_read"], tr)
    finally:
        if td:
            td.close()
        if pd:
            hmm.hipstr_post_free(pd)
        if rm:
            rm.close()
        hmm.hipstr_hmm_free(dev)
    ekw = dict(period=period, n_samples=kw["n_samples"], read_off=batch["read_off"], sample_label=batch["sample_label"], num_bps=batch["num_bps"],
               log_p1=batch["log_p1"], log_p2=batch["log_p2"])
    want = capi.run_em(hmm, "hipstr_", **ekw)
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], want))
    def cr():
        with capi.oracle_cr_math(oracle):
            return capi.run_em(oracle, "oracle_", **ekw)
    util.assert_arrays_exact(got[:4], capi.run_em(oracle, "oracle_", **ekw), cr, "chain on real records")
    assert np.array_equal(got[4], batch["read_off"]) and batch["read_off"][-1] >= 30
    assert list(got[5]) == [1 + len(set(batch["num_bps"][batch["read_off"][l]:batch["read_off"][l + 1]].tolist()) - {0}) for l in range(3)]
    assert max(got[5]) >= 2


# ------------------------------------------------------------------ 5. stale memory and allocation
def test_poisoned_cache_blocks_and_no_driver_allocation(hmm):
    c = main_case()
    wide = etc.build([dict(period=6, runs=[[("in", s) for s in (0, TABLE, 0, 0, 6)], [("in", 0), ("in", 6)]])], seed=4)       # the host route
    for case, what in ((c, "device route"), (wide, "host route")):
        with Resident(hmm, case) as R:
            def run():
                return tuple(np.asarray(x) for x in R.train()) + tuple(np.asarray(v) for k, v in sorted(R.fetch().items()) if k != "route")
            out = tp.poisoned(hmm, run, "hipstr_em_train_dev, " + what)
            tp.same_bits(run(), out[0], what + ", unpoisoned against poisoned")
            allocs = hmm.hipstr_debug_driver_allocs()
            run(); run()
            assert hmm.hipstr_debug_driver_allocs() == allocs, what


# ------------------------------------------------------------------ 6. empty inputs
def test_empty_inputs(hmm, oracle):
    c = etc.build([])
    with Resident(hmm, c) as R:
        got = R.train()
        assert all(len(x) == 0 for x in got[:4]) and list(got[4]) == [0] and len(got[5]) == 0
    # no request at all, an empty handle: every locus trains on no reads, as the host form does
    c = etc.build([dict(period=2, runs=[[("noreq",), ("noreq",)], [("noreq",)]]), dict(period=3, haploid=True, runs=[[], [("noreq",)]])])
    assert c.n_req == 0
    got, batch = check_equal(hmm, oracle, c, "no requests")
    assert list(got[4]) == [0, 0, 0] and list(got[5]) == [1, 1]
