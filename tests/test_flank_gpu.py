"""GPU: hipstr_flank_assemble_dev (include/hipstr_hmm.h; hipstr_amd/csrc/flank.hip, flank_task.h) — the De Bruijn assembly of
SeqStutterGenotyper::assemble_flanks, one wavefront per (locus, flank, sample) task on a resident traceback result.

The yardsticks: the records of the reference's own DebruijnGraph (tests/golden/flank_*.npz) with the aggregation restated in
tests/flank_cases.py, and, byte for byte in every output array, the host entry point hipstr_flank_assemble on
hipstr_trace_dev_fetch(td, HIPSTR_TRACE_F_FLANKS).  With the compiled caps no task of the unit cases, of the 200 random tasks or of the
chain on real records may leave the device (asserted through hipstr_debug_flank_plan and hipstr_debug_flank_last); with
HIPSTR_DEBUG_FLANK_CAPS shrunk part of them takes the host twin inside the call — the tasks the plan names — with identical bytes.
Handles come from capi.trace_dev_from_host for the crafted strings and from hipstr_hmm_trace_resident for the chain."""
import ctypes as C
import os

import numpy as np
import pytest

from hipstr_amd import capi
import flank_cases as fc
import test_flank_host as tfh
import test_flank_plan as tfp

pytestmark = pytest.mark.gpu


class Resident:
    """A case on the device: the posterior run (uploaded; launching is not needed) and the trace handle holding the flank strings."""

    def __init__(self, hmm, c, trace=None):
        self.hmm, self.c = hmm, c
        self.pd = hmm.hipstr_post_upload(c.pb.ptr, None); assert self.pd, hmm.hipstr_last_error().decode()
        self.td = capi.trace_dev_from_host(hmm, c.trace if trace is None else trace, c.n_req)

    def run(self, **kw):
        a = fc.args(self.c, **kw)
        return capi.run_flank(self.hmm, td=a.pop("td", self.td), pd=self.pd, **a)

    def host_form(self, **kw):
        """The host chain: fetch the FLANKS group, hipstr_flank_assemble."""
        tr = capi.trace_dev_fetch(self.hmm, self.td, capi.TRACE_F_FLANKS, null_others=True)
        return capi.run_flank(self.hmm, trace=dict(flank_seq_off=tr["flank_seq_off"], flank_seq=tr["flank_seq"]), **fc.args(self.c, **kw))

    def close(self):
        self.td.close(); self.hmm.hipstr_post_free(self.pd)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False


class caps_env:
    def __init__(self, caps):
        self.value = None if caps is None else ",".join(str(int(caps.get(k, 0))) for k in tfp.ORDER)

    def __enter__(self):
        self.old = os.environ.pop("HIPSTR_DEBUG_FLANK_CAPS", None)
        if self.value is not None:
            os.environ["HIPSTR_DEBUG_FLANK_CAPS"] = self.value

    def __exit__(self, *a):
        os.environ.pop("HIPSTR_DEBUG_FLANK_CAPS", None)
        if self.old is not None:
            os.environ["HIPSTR_DEBUG_FLANK_CAPS"] = self.old
        return False


@pytest.fixture(scope="module")
def batches():
    out = {}
    for name, make in fc.BATCHES.items():
        c = fc.build(make())
        text, records = fc.golden(name)
        assert fc.case_text(c) == text
        out[name] = (c, fc.expect(c, records))
    return out


def check(hmm, c, want, what, caps=None, **kw):
    """Device == golden aggregation == host entry point (bytes); the route of every task is the plan's.  Returns (result, last)."""
    n_tasks = 2 * int(c.samp_off[-1])
    with Resident(hmm, c) as R, caps_env(caps):
        got = R.run(**kw)
        last = capi.flank_last(hmm, n_tasks)
        host = R.host_form(**kw)
        plan = tfp.rows(capi.flank_plan(hmm, trace=c.trace, **fc.args(c, **kw)))
    fc.same_bytes(got, host, what + ": device against hipstr_flank_assemble")
    if want is not None:
        fc.assert_matches(c, got, want, what)
    assert last["tasks"] == n_tasks
    assert [int(f != 0) for f in last["flags"]] == [int(x["route"] == 1) for x in plan], what + ": the tasks that left the device are not the plan's"
    assert last["host_tasks"] == sum(1 for x in plan if x["route"] == 1) and last["skipped"] == sum(1 for x in plan if x["route"] == 2)
    assert last["fetched_strings"] == (last["host_tasks"] > 0)
    # the sizes the kernel counted are the host twin's (for the tasks that stayed and were not skipped)
    for t, x in enumerate(plan):
        if x["route"] == 0:
            assert list(last["sizes"][t][:2]) == [x["edges"], x["nodes"]] and last["sizes"][t][3] == x["strings"], "%s: sizes of task %d" % (what, t)
            assert x["k"] < 0 or last["sizes"][t][2] == x["recs"], "%s: records of task %d" % (what, t)
    return got, last, plan


@pytest.mark.parametrize("name", sorted(fc.BATCHES))
def test_device_equals_the_reference_and_the_host_entry_point(hmm, batches, name):
    """All unit cases in one ragged batch of loci; the 200 random tasks in another.  Default caps: nothing leaves the device."""
    c, want = batches[name]
    got, last, plan = check(hmm, c, want, name)
    assert last["host_tasks"] == 0 and not last["fetched_strings"]
    assert name != "random" or len(plan) == 200


def test_shrunk_caps_send_part_of_the_tasks_to_the_host_twin(hmm, batches):
    for name, caps in (("unit", dict(edges=24, recs=40)), ("random", dict(edges=30, nodes=30, recs=48, reads=10, len=36, path_len=36)), ("unit", dict(reads=5)),
                       ("unit", dict(len=31)), ("unit", dict(nodes=23))):
        c, want = batches[name]
        got, last, plan = check(hmm, c, want, "%s %s" % (name, caps), caps=caps)
        live = sum(1 for x in plan if x["route"] != 2)
        assert 0 < last["host_tasks"] < live, (name, caps, last["host_tasks"], live)


def test_parameters_of_the_request(hmm, batches):
    c, _ = batches["unit"]
    for kw in (dict(max_paths=16), dict(min_path_weight=3), dict(max_kmer=11), dict(min_kmer=12, max_kmer=14), dict(max_flank_haplotypes=5, min_flank_freq=0.05),
               dict(max_total_haplotypes=2)):
        got, last, _ = check(hmm, c, None, str(kw), **kw)
        assert last["host_tasks"] == 0
    # what the device does not serve goes to the host twin, all of it, with the same bytes
    for kw in (dict(max_paths=17), dict(max_kmer=16)):
        got, last, plan = check(hmm, c, None, str(kw), **kw)
        assert last["host_tasks"] > 0
    c2 = fc.build([dict(fc.unit_loci()[1])])
    c2.loci[0]["samples"][0]["reads"][0] = fc.rd(c2.loci[0]["samples"][0]["reads"][0]["l"], c2.loci[0]["samples"][0]["reads"][0]["r"].lower())
    c2 = fc.build(c2.loci)
    got, last, plan = check(hmm, c2, None, "lower case")
    assert list(last["flags"]) == [0, capi.FLANK_FLAGS["byte"]]


def test_capacities(hmm, batches):
    c, _ = batches["unit"]
    with Resident(hmm, c) as R:
        full = R.run()
        need = full["need"]
        for short in ("opts", "opt_chars", "paths", "path_chars"):
            caps = dict(opts=sum(len(o) for L in full["opts"] for o in L), opt_chars=sum(len(s) for L in full["opts"] for o in L for s, _ in o),
                        paths=sum(len(p) for p in full["paths"]), path_chars=sum(len(s) for p in full["paths"] for _, s in p))
            want = dict(caps)
            caps[short] -= 1
            fc.same_bytes(R.run(caps=caps), R.host_form(caps=caps), short)
            assert R.run(caps=caps)["rc"] == 3 and R.run(caps=caps)["need"] == want
        slim = R.run(want_paths=False, caps=dict(opts=want["opts"], opt_chars=want["opt_chars"], paths=0, path_chars=0))
        assert slim["rc"] == 0 and slim["opts"] == full["opts"] and np.array_equal(slim["realign_pool"], full["realign_pool"])


def test_refusals(hmm, batches):
    c, _ = batches["unit"]
    with Resident(hmm, c) as R:
        tfh.refusals(lambda **kw: R.run(**kw), c)
        def refused(word, **kw):
            with pytest.raises(RuntimeError, match=word) as e:
                R.run(**kw)
            tfh._untouched(e)
        # messages of the shared checks are the host form's
        rr = c.read_req.copy(); rr[1] = c.n_req
        with pytest.raises(RuntimeError) as h:
            R.host_form(read_req=rr)
        with pytest.raises(RuntimeError) as d:
            R.run(read_req=rr)
        assert str(h.value).split(": ", 1)[1] == str(d.value).split(": ", 1)[1]
        # a handle of another request count, a handle without the FLANKS group
        other = capi.trace_dev_from_host(hmm, dict(flank_seq_off=c.trace["flank_seq_off"][:2 * c.n_req - 1], flank_seq=c.trace["flank_seq"]), c.n_req - 1)
        refused("rq->n_req differs from the trace handle's", td=other)
        other.close()
        bare = capi.trace_dev_from_host(hmm, dict(ll=np.zeros(c.n_req), max_index=np.zeros(c.n_req, np.int32)), c.n_req)
        refused("without flank_seq_off / flank_seq", td=bare)
        bare.close()
        with pytest.raises(RuntimeError, match="null argument"):
            capi.run_flank(hmm, td=C.c_void_p(None), pd=R.pd, **fc.args(c))
        # an offset that leaves the pool: nothing is read outside it, and the call is refused once the host has seen the offsets
        off = c.trace["flank_seq_off"].copy(); off[5] = off[-1] + 1000
        wild = capi.trace_dev_from_host(hmm, dict(flank_seq_off=off, flank_seq=c.trace["flank_seq"]), c.n_req)
        refused("flank_seq_off decreases or leaves the pool", td=wild)
        assert capi.flank_last(hmm, 4)["flags"][1] == capi.FLANK_FLAGS["range"]
        wild.close()
        # the device is as usable as before
        assert R.run()["rc"] == 0


def test_empty_inputs(hmm):
    c = fc.build([])
    with Resident(hmm, c) as R:
        got = R.run()
        assert got["rc"] == 0 and list(got["opt_off"]) == [0]
        fc.same_bytes(got, R.host_form(), "no loci")
    c = fc.build([dict(name="a", ref=("ACGTTGCATGCCATGACTGACTTGA", "TTGACCATGGTACCGATTACAGGAC"), samples=[dict(reads=[]), dict(reads=[])]),
                  dict(name="b", ref=("ACGTTGCATGCCATGACTGACTTGA", ""), samples=[])])
    assert c.n_req == 0
    got, last, _ = check(hmm, c, None, "no requests")
    assert list(got["status"]) == [0, 1] and list(got["task_k"]) == [10] * 4 and last["host_tasks"] == 0


def test_chain_on_real_records(hmm):
    """3 seeded loci of 40 pooled reads: forward -> hipstr_rm_scatter -> posteriors -> hipstr_post_assign(RETRACE) -> hipstr_hmm_trace_resident
    -> hipstr_flank_assemble_dev on the handle as it lies, against hipstr_flank_assemble on the fetched FLANKS group."""
    rng = np.random.default_rng(5)
    sb = capi.SynthBatch(n_loci=3, reads_per_locus=40, n_str_alleles=4, seed=77)
    b = sb.ptr.contents
    A = np.diff(np.ctypeslib.as_array(b.hap_off, shape=(4,))).astype(np.int32)
    pool_off = np.ctypeslib.as_array(b.read_off, shape=(4,)).astype(np.int32)
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
        td = capi.run_trace_resident(hmm, sb.ptr, asg["req_read"], asg["req_allele"], capi.hap_aln_info(hmm, "hipstr_", sb.ptr))
        a = dict(pb=pb, bptr=sb.ptr, seed=seeds, read_req=asg["read_req"], req_read=asg["req_read"], pool_index=pool, min_flank_freq=0.15)
        got = capi.run_flank(hmm, td=td, pd=pd, **a)
        last = capi.flank_last(hmm, 2 * 3 * S)
        tr = capi.trace_dev_fetch(hmm, td, capi.TRACE_F_FLANKS, null_others=True)
        trace = dict(flank_seq_off=tr["flank_seq_off"], flank_seq=tr["flank_seq"])
        host = capi.run_flank(hmm, trace=trace, **a)
        plan = tfp.rows(capi.flank_plan(hmm, trace=trace, **a))
    finally:
        if td:
            td.close()
        if pd:
            hmm.hipstr_post_free(pd)
        if rm:
            rm.close()
        hmm.hipstr_hmm_free(dev)
    fc.same_bytes(got, host, "chain on real records")
    assert last["host_tasks"] == 0 and all(x["flags"] == 0 for x in plan)
    assert got["rc"] == 0 and list(got["status"]) == [0, 0, 0] and sum(1 for k in got["task_k"] if k >= 10) >= 9
    assert max(x["strings"] for x in plan) >= 8 and max(x["len"] for x in plan) >= 40          # real flank strings went through the graphs
    km = capi.flank_kmer_lengths(hmm, sb.ptr)
    assert all(km[l, f] >= 10 and (k < 0 or k >= km[l, f]) for l in range(3) for f in range(2) for k in got["task_k"][2 * S * l + S * f:][:S])
