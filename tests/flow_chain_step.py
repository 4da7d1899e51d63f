"""Helper (not a test module): flow_chain.genotype_pass and flow_chain_flanks.flank_pass with the caller's bookkeeping between the rounds —
State.step / State.apply per locus, build_batch, the haps_to_alleles concatenation — replaced by ONE library call per round:
hipstr_alleles_step after a census, hipstr_alleles_apply around the flank stage.  Every array the later calls need comes out of the call
before them: allele_mapping and new_n_alleles for the remap, the masked batch for upload / align / scatter, the unmasked batch and
hap_to_allele for the trace, the census and the next step.  What stays with the caller is what the header says stays: copy_read, and the
re-keying of the trace cache through allele_mapping (seq_stutter_genotyper.cpp:401-409).  flow_chain.py and flow_chain_flanks.py are
imported and left as they are; the backends are theirs.
"""
import ctypes as C

import numpy as np

from hipstr_amd import capi
import flow_chain as fc
import flow_chain_flanks as ff
import util


class Pooled:
    """A hipstr_batch_t that came out of a library call, shaped like capi.Batch for the backends: .ptr, and .arrays read through the pointers."""

    def __init__(self, ptr, keep):
        self.ptr, self._keep, self._arrays = ptr, keep, None

    @property
    def arrays(self):
        if self._arrays is None:
            b = self.ptr.contents; nl = int(b.n_loci)
            arr = lambda p, n, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt) if n else np.zeros(0, dt)
            a = dict(blk_start=arr(b.blk_start, 3 * nl, np.int32), blk_end=arr(b.blk_end, 3 * nl, np.int32), blk_nopts=arr(b.blk_nopts, 3 * nl, np.int32),
                     period=arr(b.period, nl, np.int32), stutter=arr(b.stutter, 6 * nl, np.float64), hap_off=arr(b.hap_off, nl + 1, np.int32),
                     read_off=arr(b.read_off, nl + 1, np.int32))
            a["opt_off"] = arr(b.opt_off, int(a["blk_nopts"].sum()) + 1, np.int32)
            n = int(a["read_off"][-1])
            a["base_off"] = arr(b.base_off, n + 1, np.int32); a["read_start"] = arr(b.read_start, n, np.int32); a["cigar_off"] = arr(b.cigar_off, n + 1, np.int32)
            a["cigar_len"] = arr(b.cigar_len, int(a["cigar_off"][-1]), np.int32)
            a["seq"] = C.string_at(b.seq, int(a["opt_off"][-1])); a["bases"] = C.string_at(b.bases, int(a["base_off"][-1]))
            a["quals"] = C.string_at(b.quals, int(a["base_off"][-1])); a["cigar_op"] = C.string_at(b.cigar_op, int(a["cigar_off"][-1]))
            a["realign_hap"] = arr(b.realign_hap, int(a["hap_off"][-1]), np.uint8) if b.realign_hap else None
            a["realign_read"] = arr(b.realign_read, n, np.uint8) if b.realign_read else None
            self._arrays = a
        return self._arrays


def take(states, a, old_A):
    """What the call leaves to the caller: the states' blocks follow the result (the backends and the dump read them), and the trace cache is
    re-keyed through allele_mapping (:401-409)."""
    opts = a.options(); mo = 0
    for l, s in enumerate(states):
        s.blocks = [(st, en, [o.decode() for o in opts[l][b]]) for b, (st, en, _) in enumerate(s.blocks)]
        m = a.mapping[mo:mo + old_A[l]]; mo += old_A[l]
        s.cache = {(p, int(m[h])): v for (p, h), v in s.cache.items() if m[h] != -1}
    assert mo == len(a.mapping)


def masks_of(a):
    return [a.realign_hap[a.hap_off[l]:a.hap_off[l + 1]].copy() for l in range(len(a.new_n_alleles))]


def genotype_pass(states, be, oracle, recs, lib, host):
    """flow_chain.genotype_pass with one hipstr_alleles_step per round."""
    k = fc.layout_of(states); nl = len(states)
    phase = np.zeros(nl, np.int32)                                     # HIPSTR_PHASE_ADD
    unpooled = fc.build_batch(states, [s.inp.reads for s in states])
    pool = be.pool(unpooled, states)
    k.pool_index, k.pool_off, pool_reads = pool["pool_index"], pool["pool_off"], pool["reads"]
    be.create([s.A for s in states], k)
    first = pool.get("batch") or fc.build_batch(states, pool_reads)
    be.align_scatter(first, None, [None] * nl)
    seeds = be.seeds()
    if recs is not None:
        recs.append(dict(matrix_after_scatter=be.matrix()) if be.diag else {})
    # round 1's hap_to_allele: the identity update of the first batch (every locus off)
    a = capi.run_alleles_apply(lib, first.ptr, locus_on=np.zeros(nl, np.uint8), host=host)
    assert np.array_equal(a.mapping, np.concatenate([np.arange(s.A) for s in states]))
    pooled = Pooled(a.ptr_all, (a, first))
    while True:
        be.posteriors(fc.post_kw(states, k))
        if all(p == capi.PHASE_DONE for p in phase):
            break
        asg = be.assign(seeds, k)
        tr = be.trace(pooled, asg, states)
        cen = be.census(pooled, seeds, asg, tr, a.h2a, states, k)
        old_A = [int(x) for x in a.new_n_alleles]
        rec = dict(read_off=k.read_off.copy(), n_alleles=np.array(old_A, np.int32), cand=cen["cand"], called=cen["called"].copy(),
                   spanned=cen["spanned"].copy(), new_n_haps=np.asarray(cen["new_n_haps"]).copy(),
                   n_req=int(asg["n_req"]), req_read=asg["req_read"].copy(), req_allele=asg["req_allele"].copy(), read_req=asg["read_req"].copy())
        for l, s in enumerate(states):
            if phase[l] != capi.PHASE_DONE:                            # this locus' retrace_alignments ran: the cache takes what it did not have
                for q in np.nonzero((asg["req_read"] >= k.pool_off[l]) & (asg["req_read"] < k.pool_off[l + 1]))[0]:
                    s.cache.setdefault((int(asg["req_read"][q] - k.pool_off[l]), int(asg["req_allele"][q])), (tr, int(q)))
        nxt = capi.run_alleles_step(lib, pooled.ptr, cen, phase, max_total_haplotypes=fc.MAX_TOTAL_HAPLOTYPES, host=host)
        assert not nxt.status.any()                                    # (no case aborts)
        take(states, nxt, old_A)
        copy = np.zeros(k.n, np.uint8)
        for l in np.nonzero(nxt.added)[0]:                             # copy_read: every read of a locus a sequence was added to (:320, :397-398)
            copy[k.read_off[l]:k.read_off[l + 1]] = 1
        rec.update(mapping=nxt.mapping.copy(), new_n_alleles=nxt.new_n_alleles.copy(), n_added=nxt.n_added.copy(), n_removed=nxt.n_removed.copy(),
                   n_affected_blocks=nxt.n_affected_blocks.copy(), phase=phase.copy())
        be.end_posteriors()
        be.remap(list(nxt.new_n_alleles), nxt.mapping)
        if recs is not None and be.diag:
            rec["matrix_after_remap"] = be.matrix()
        if nxt.any_added:
            be.align_scatter(Pooled(nxt.ptr, nxt), copy, masks_of(nxt))
        pooled = Pooled(nxt.ptr_all, (nxt, first)); a = nxt
        if recs is not None:
            if be.diag:
                rec["matrix_after_scatter"] = be.matrix()
            recs.append(rec)
    for s in states:
        s.phase = fc.DONE
    return k, pooled, seeds, a


def with_realign_read(bptr, flags, keep):
    """the batch with the caller's realign_read (assemble_flanks' realign_pools): a copy of the struct, one pointer changed"""
    s = capi.HipstrBatch()
    C.memmove(C.byref(s), bptr, C.sizeof(s))
    s.realign_read = flags.ctypes.data_as(capi._u8p)
    s._keepalive = (flags, keep)
    return Pooled(C.pointer(s), (s, flags, keep))


def flank_pass(states, be, oracle, k, pooled, seeds, a, recs, lib, host):
    """flow_chain_flanks.flank_pass with hipstr_alleles_apply for both of its updates (:201, :207-211)."""
    nl = len(states)
    asg, tr = ff._retrace(states, be, k, pooled, seeds, [True] * nl)
    fl = be.flank(pooled, seeds, asg, tr, k)
    assert fl["rc"] == 0
    rec = dict(flank_status=fl["status"].copy(), flank_new_n_haps=fl["new_n_haps"].copy(), flank_opts=[[list(o) for o in L] for L in fl["opts"]],
               flank_sample_status=fl["sample_status"].copy(), flank_realign_sample=fl["realign_sample"].copy(), flank_realign_pool=fl["realign_pool"].copy(),
               flank_copy_read=fl["copy_read"].copy(), flank_task_k=fl["task_k"].copy(), flank_paths=[list(p) for p in fl["paths"]])
    if recs is not None:
        recs.append(rec)
    assert not fl["status"].any()
    realigns = np.array([bool(fl["realign_pool"][k.pool_off[l]:k.pool_off[l + 1]].any()) for l in range(nl)])
    if not realigns.any():
        return pooled
    # ---- add_and_remove_alleles(none, alleles_to_add, realign_pools, copy_reads) (:201): flank.opt_* as the adds
    add = [[[o for o, _ in fl["opts"][l][0]], [], [o for o, _ in fl["opts"][l][1]]] if realigns[l] else [[], [], []] for l in range(nl)]
    old_A = [int(x) for x in a.new_n_alleles]
    nxt = capi.run_alleles_apply(lib, pooled.ptr, locus_on=realigns.astype(np.uint8), add=add, host=host)
    take(states, nxt, old_A)
    copy = np.zeros(k.n, np.uint8); pool_flags = np.zeros(int(k.pool_off[-1]), np.uint8)
    for l in np.nonzero(realigns)[0]:
        copy[k.read_off[l]:k.read_off[l + 1]] = fl["copy_read"][k.read_off[l]:k.read_off[l + 1]]
        pool_flags[k.pool_off[l]:k.pool_off[l + 1]] = fl["realign_pool"][k.pool_off[l]:k.pool_off[l + 1]] != 0
    be.end_posteriors()
    be.remap(list(nxt.new_n_alleles), nxt.mapping)
    be.align_scatter(with_realign_read(nxt.ptr, pool_flags, nxt), copy, masks_of(nxt))
    pooled = Pooled(nxt.ptr_all, nxt); a = nxt
    be.posteriors(fc.post_kw(states, k))
    # ---- get_unused_alleles(false, true) (:207) for the loci that realigned: census.called as keep
    asg, tr = ff._retrace(states, be, k, pooled, seeds, list(realigns))
    called = np.asarray(be.called(pooled, seeds, asg, tr, a.h2a, states, k, (fl["sample_status"] != 0).astype(np.uint8)))
    keep = np.ones(len(called), np.uint8); on = np.zeros(nl, np.uint8); ob = 0
    for l in range(nl):
        no = [int(x) for x in a.blk_nopts[3 * l:3 * l + 3]]
        for b in range(3):
            if realigns[l] and no[b] > 1:                              # :255, :305-311
                keep[ob + 1:ob + no[b]] = called[ob + 1:ob + no[b]] != 0
            ob += no[b]
        on[l] = 1 if not keep[ob - sum(no):ob].all() else 0
    old_A = [int(x) for x in a.new_n_alleles]
    nxt = capi.run_alleles_apply(lib, pooled.ptr, locus_on=on, keep=keep, keep_blocks=7, host=host)      # remove_alleles (:211)
    assert not nxt.realign_hap.any() and not nxt.added.any()
    take(states, nxt, old_A)
    rec.update(flank_called=called.copy(), flank_mapping=nxt.mapping.copy(), flank_n_req=int(asg["n_req"]), flank_req_read=asg["req_read"].copy(),
               flank_req_allele=asg["req_allele"].copy())
    if on.any():
        be.end_posteriors()
        be.remap(list(nxt.new_n_alleles), nxt.mapping)
        pooled = Pooled(nxt.ptr_all, nxt)
        be.posteriors(fc.post_kw(states, k))
    return pooled


def run(names, be, oracle, lib, host, recs=None):
    """flow_chain.run: every case as one batch through genotype() [and, for the --recompute cases, recompute_stutter_models()] -> {name: dump}"""
    states = [fc.State(fc.Inputs(n), oracle) for n in names]
    k, pooled, seeds, _ = genotype_pass(states, be, oracle, recs, lib, host)
    again = [l for l, s in enumerate(states) if s.inp.recompute]
    em = None
    if again:                                                          # recompute_stutter_models :1545-1577, on the whole batch
        asg = be.assign(seeds, k)
        tr = be.trace(pooled, asg, states)
        em = be.em(pooled, seeds, asg, tr, k)
        if recs is not None:
            recs.append(dict(em_trained=em[0].copy(), em_stutter=em[1].copy(), n_req=int(asg["n_req"]), req_read=asg["req_read"].copy(),
                             req_allele=asg["req_allele"].copy(), read_req=asg["read_req"].copy()))
    fin = fc.finish(states, k, be)
    out = {s.inp.name: fc.dump_of(s, k, l, fin) for l, s in enumerate(states) if l not in again}
    if again:
        sub = [states[l] for l in again]
        for l, s in zip(again, sub):
            assert em[0][l], "EM did not train"
            s.stutter = em[1][l].copy()
            s.cache = {}
        k2, _, _, _ = genotype_pass(sub, be, oracle, recs, lib, host)
        fin = fc.finish(sub, k2, be)
        out.update({s.inp.name: fc.dump_of(s, k2, i, fin, stutter_model=s.stutter) for i, s in enumerate(sub)})
    return out


def run_flanks(names, be, oracle, lib, host, recs=None):
    """flow_chain_flanks.run: genotype() with flanks"""
    states = [fc.State(ff.Inputs(n), oracle) for n in names]
    k, pooled, seeds, a = genotype_pass(states, be, oracle, recs, lib, host)
    flank_pass(states, be, oracle, k, pooled, seeds, a, recs, lib, host)
    fin = fc.finish(states, k, be)
    return {s.inp.name: fc.dump_of(s, k, l, fin) for l, s in enumerate(states)}
