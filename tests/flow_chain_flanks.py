"""Helper (not a test module): tests/flow_chain.py's driver of SeqStutterGenotyper::genotype() with its LAST statement added — assemble_flanks
(reference src/seq_stutter_genotyper.cpp:40-217, reached from :666-668) on hipstr_flank_assemble / hipstr_flank_assemble_dev — for the six
flank cases of tests/test_genotype_flow.py, against their existing goldens tests/golden/flow_<case>.txt.gz (runs of the compiled reference
with flanks on) from the same runs' inputs (tests/golden/flowin_<case>.txt.gz, --dump-inputs).

After flow_chain.genotype_pass (:603-665, the same rounds with or without flanks):
  retrace_alignments                                      (:42)      assign(RETRACE), trace; the trace cache takes what it did not have
  the assembly and its aggregation                        (:44-180)  Backend.flank: hipstr_flank_assemble[_dev]
  where a pool of a locus realigns                        (:193-214)
    add_and_remove_alleles(none, new flank options, realign_pools, copy_reads)   State.apply; remap; align only the marked pools against the
                                                          new haplotypes; scatter with copy_read; posteriors
    get_unused_alleles(false, true)                       (:207)     retrace (the cache again); the census's `called` marks with
                                                                     sample_uncallable = sample_status != 0
    remove_alleles where an allele is uncalled            (:211)     State.apply; remap; posteriors
The two --recompute flank cases are out of scope here.

Regenerate the inputs (CPU only, needs oracle/_ref/libflow_ref.so): python tests/flow_chain_flanks.py --regen"""
import gzip
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hipstr_amd import capi  # noqa: E402
import flow_chain as fch  # noqa: E402

# case -> arguments of integration/genotype_flow.cpp, as tests/test_genotype_flow.py gives them
CASES = {
    "s1p2": ["--seed", "1", "--period", "2"],
    "s1p3": ["--seed", "1", "--period", "3"],
    "s7p4": ["--seed", "7", "--period", "4"],
    "s2p2": ["--seed", "2", "--period", "2"],
    "s5p2": ["--seed", "5", "--period", "2"],
    "s3p5_24samples": ["--seed", "3", "--period", "5", "--samples", "24", "--reads", "12"],
}
FLANK_KW = dict(max_total_haplotypes=fch.MAX_TOTAL_HAPLOTYPES, max_flank_haplotypes=4, min_flank_freq=0.15)      # genotype(1000, 4, 0.15, ...)


class Inputs(fch.Inputs):
    def __init__(self, name):
        fch.CASES[name] = CASES[name]                                  # (flow_chain.Inputs looks the case's arguments up; its table is left as it was)
        try:
            fch.Inputs.__init__(self, name)
        finally:
            del fch.CASES[name]


class HostBackend(fch.HostBackend):
    """flow_chain.HostBackend and hipstr_flank_assemble on the oracle's trace records."""

    def flank(self, pooled, seeds, asg, tr, k):
        recs = self.traces[tr]
        flat = [x for t in recs for x in (t["flank_left"], t["flank_right"])]
        trace = dict(flank_seq_off=np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int32), flank_seq="".join(flat).encode() + b"?")
        return capi.run_flank(self.hmm, self.pb, pooled.ptr, seeds, asg["read_req"], asg["req_read"], k.pool_index, trace=trace, **FLANK_KW)

    def called(self, pooled, seeds, asg, tr, h2a, states, k, uncallable):
        c = fch.Case(); c.pb = self.pb; c.pool_off = k.pool_off; c.h2a = h2a
        c.loci = [fch.Locus(s.blocks, [None] * s.inp.n_samples, [], n_pooled=int(k.pool_off[l + 1] - k.pool_off[l])) for l, s in enumerate(states)]
        return fch.census_restate(c, self.gt, LL=self.M, trace=self._trace_dict(tr), read_req=asg["read_req"], req_read=asg["req_read"], seed=seeds,
                                  uncallable=uncallable)["called"]


class DeviceBackend(fch.DeviceBackend):
    """flow_chain.DeviceBackend and hipstr_flank_assemble_dev on the resident trace result."""

    def flank(self, pooled, seeds, asg, tr, k):
        return capi.run_flank(self.hmm, self.pb, pooled.ptr, seeds, asg["read_req"], asg["req_read"], k.pool_index, td=self.tds[tr], pd=self.pd, **FLANK_KW)

    def called(self, pooled, seeds, asg, tr, h2a, states, k, uncallable):
        out = capi.run_census(self.hmm, self.pd, pooled.ptr, seeds, asg["read_req"], asg["req_read"], None, hap_to_allele=h2a, n_samp=int(k.samp_off[-1]),
                              td=self.tds[tr], sample_uncallable=uncallable)
        assert out["rc"] == 0
        return out["called"]


def _retrace(states, be, k, pooled, seeds, which):
    """retrace_alignments for the loci of `which`: the picks, the traces, and the cache takes what it did not have."""
    asg = be.assign(seeds, k)
    tr = be.trace(pooled, asg, states)
    for l, s in enumerate(states):
        if which[l]:
            for q in np.nonzero((asg["req_read"] >= k.pool_off[l]) & (asg["req_read"] < k.pool_off[l + 1]))[0]:
                s.cache.setdefault((int(asg["req_read"][q] - k.pool_off[l]), int(asg["req_allele"][q])), (tr, int(q)))
    return asg, tr


def flank_pass(states, be, oracle, k, pooled, seeds, pool_reads, recs):
    """assemble_flanks (:40-217) for the batch, behind genotype_pass."""
    nl = len(states)
    asg, tr = _retrace(states, be, k, pooled, seeds, [True] * nl)      # :42
    fl = be.flank(pooled, seeds, asg, tr, k)
    assert fl["rc"] == 0
    rec = dict(flank_status=fl["status"].copy(), flank_new_n_haps=fl["new_n_haps"].copy(), flank_opts=[[list(o) for o in L] for L in fl["opts"]],
               flank_sample_status=fl["sample_status"].copy(), flank_realign_sample=fl["realign_sample"].copy(), flank_realign_pool=fl["realign_pool"].copy(),
               flank_copy_read=fl["copy_read"].copy(), flank_task_k=fl["task_k"].copy(), flank_paths=[list(p) for p in fl["paths"]])
    if recs is not None:
        recs.append(rec)
    assert not fl["status"].any()                                      # (no case aborts)
    realigns = [bool(fl["realign_pool"][k.pool_off[l]:k.pool_off[l + 1]].any()) for l in range(nl)]       # realign_count > 0 (:198)
    if not any(realigns):
        return pooled
    # ---- add_and_remove_alleles(none, alleles_to_add, realign_pools, copy_reads) (:201)
    none = [[], [], []]
    mapping, masks, new_A = [], [], []
    for l, s in enumerate(states):
        if realigns[l]:
            add = [[o.decode() for o, _ in fl["opts"][l][0]], [], [o.decode() for o, _ in fl["opts"][l][1]]]
            m, r = s.apply(none, add)
        else:
            m, r = list(range(s.A)), [False] * s.A
        mapping += m; masks.append(np.array(r, np.uint8)); new_A.append(len(r))
    copy = np.zeros(k.n, np.uint8)
    reads = []
    for l in range(nl):
        on = realigns[l]
        if on:
            copy[k.read_off[l]:k.read_off[l + 1]] = fl["copy_read"][k.read_off[l]:k.read_off[l + 1]]
        reads.append([dict(rd, realign=bool(on and fl["realign_pool"][k.pool_off[l] + p])) for p, rd in enumerate(pool_reads[l])])
    be.end_posteriors()
    be.remap(new_A, mapping)
    be.align_scatter(fch.build_batch(states, reads, masks), copy, masks)
    pooled = fch.build_batch(states, pool_reads)
    be.posteriors(fch.post_kw(states, k))                              # :414
    # ---- get_unused_alleles(false, true) (:207), for the loci that realigned
    asg, tr = _retrace(states, be, k, pooled, seeds, realigns)
    opts = [s.options() for s in states]
    h2a = [np.concatenate([o[:, b] for o in opts]).astype(np.int32) for b in range(3)]
    called = be.called(pooled, seeds, asg, tr, h2a, states, k, (fl["sample_status"] != 0).astype(np.uint8))
    mapping, new_A = [], []
    ob = 0; any_removed = False
    for l, s in enumerate(states):
        no = s.nopts
        rem = none
        if realigns[l]:
            rem = [[o for o in range(1, no[b]) if not called[ob + sum(no[:b]) + o]] if no[b] > 1 else [] for b in range(3)]      # :255, :305-311
        ob += sum(no)
        if any(rem):
            m, r = s.apply(rem, none); any_removed = True              # remove_alleles (:211)
            assert not any(r)
        else:
            m = list(range(s.A))
        mapping += m; new_A.append(s.A)
    rec.update(flank_called=np.asarray(called).copy(), flank_mapping=np.array(mapping, np.int32), flank_n_req=int(asg["n_req"]), flank_req_read=asg["req_read"].copy(),
               flank_req_allele=asg["req_allele"].copy())
    if any_removed:
        be.end_posteriors()
        be.remap(new_A, mapping)
        pooled = fch.build_batch(states, pool_reads)
        be.posteriors(fch.post_kw(states, k))
    return pooled


def run(names, be, oracle, recs=None):
    """Every case of `names` as one batch through genotype() with flanks -> {name: dump}."""
    states = [fch.State(Inputs(n), oracle) for n in names]
    k, pooled, seeds = fch.genotype_pass(states, be, oracle, recs)
    flank_pass(states, be, oracle, k, pooled, seeds, be._reads, recs)
    fin = fch.finish(states, k, be)
    return {s.inp.name: fch.dump_of(s, k, l, fin) for l, s in enumerate(states)}


def against_gold(got, name):
    """flow_chain.against_gold's criteria (test_genotype_flow._compare's bars, unchanged) on the lines the chain produces."""
    import test_genotype_flow as tgf
    want = "".join(l + "\n" for l in fch.gold(name).splitlines() if l.split(" ")[0] not in ("genotype_ok", "recompute_ok", "log"))
    tgf._compare(got, want, loose_ll=False)


if __name__ == "__main__" and "--regen" in sys.argv:
    import tempfile
    refdir = os.path.join(ROOT, "oracle", "_ref")
    for name, args in CASES.items():
        with tempfile.TemporaryDirectory() as t:
            out, inp = os.path.join(t, "flow.txt"), os.path.join(t, "in.txt")
            r = subprocess.run([os.path.join(refdir, "flow_launcher"), os.path.join(refdir, "libflow_ref.so")] + args + ["--out", out, "--dump-inputs", inp],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            assert r.returncode == 0, r.stdout
            assert open(out).read() == fch.gold(name), name            # the committed reference dump is the yardstick and keeps its bytes
            dst = os.path.join(fch.GOLD, "flowin_%s.txt.gz" % name)
            with gzip.GzipFile(dst, "wb", mtime=0) as f:
                f.write(open(inp).read().encode())
            print(name, "->", os.path.getsize(dst), "bytes")
