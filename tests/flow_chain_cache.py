"""Helper (not a test module): tests/flow_chain.py's device backend with the trace cache of INTEGRATION.md §2a in the place of the plain
traceback call — hipstr_trace_cache_round for hipstr_hmm_trace_resident (locus_takes from the states' phases: a locus that is DONE gets its
records for the round, its cache does not take them, flow_chain.py's line for seq_stutter_genotyper.cpp:828-835), hipstr_trace_cache_remap
beside hipstr_rm_remap, a fresh cache for the second pass of recompute_stutter_models (:1579).

The driver's own dictionary (flow_chain.State.cache, re-keyed by State.apply) stays what it is: the restatement.  Both backends here count,
per trace call and before the call, the requests whose key that dictionary does not hold — the misses the reference's retrace_alignments
would trace.  CountingHostBackend does so without a device."""
import numpy as np

from hipstr_amd import capi
import flow_chain as fc


def request_keys(asg, k):
    """The distinct (locus, pool, haplotype) keys of a request list, in order of first occurrence."""
    out = {}
    for r, a in zip(asg["req_read"][:asg["n_req"]], asg["req_allele"][:asg["n_req"]]):
        l = int(np.searchsorted(k.pool_off, r, side="right")) - 1
        out.setdefault((l, int(r - k.pool_off[l]), int(a)))
    return list(out)


def restated_misses(asg, states, k):
    """The keys of the request list that the states' dictionaries do not hold.  A locus that is DONE takes nothing (flow_chain.py:
    `if s.phase != DONE`), so what it misses it misses again in the next call."""
    return sum(1 for (l, p, h) in request_keys(asg, k) if (p, h) not in states[l].cache)


class CountingHostBackend(fc.HostBackend):
    """The host backend; calls: per trace call (requests, misses by the dictionary restatement, misses if every locus took its records —
    a second dictionary kept here, re-keyed like the first: the reference's own count, which never asks a locus that is done)."""

    def __init__(self, hmm_host, oracle):
        super().__init__(hmm_host, oracle)
        self.calls = []; self.every = None

    def create(self, A, k):
        super().create(A, k)
        self.every = set()                                             # (:1579: a pass starts from an empty cache)

    def trace(self, pooled, asg, states):
        keys = request_keys(asg, self.k)
        self.calls.append((int(asg["n_req"]), restated_misses(asg, states, self.k), sum(1 for key in keys if key not in self.every)))
        self.every.update(keys)
        return super().trace(pooled, asg, states)

    def remap(self, new_A, mapping):
        base = np.concatenate([[0], np.cumsum(self.A)])
        self.every = {(l, p, int(mapping[base[l] + h])) for (l, p, h) in self.every if mapping[base[l] + h] != -1}      # :401-409
        super().remap(new_A, mapping)


class CachedDeviceBackend(fc.DeviceBackend):
    """calls: per trace call (requests, misses by the restatement, the stats of hipstr_trace_cache_round); finals: per pass what the cache
    itself holds at the end — its entries and its view, fetched — and the pass' pool_off."""

    def __init__(self, hmm, pool_flags=0, diag=False):
        super().__init__(hmm, pool_flags, diag)
        self.tc = None; self.calls = []; self.finals = []

    def create(self, A, k):
        super().create(A, k)
        if self.tc is not None:
            self.tc.close()                                            # :1579: the second pass starts from an empty cache
        self.tc = capi.TraceCache(self.hmm, k.pool_off, A)

    def trace(self, pooled, asg, states):
        h2r = capi.hap_aln_info(self.hmm, "hipstr_", pooled.ptr)
        takes = np.array([s.phase != fc.DONE for s in states], np.uint8)
        want = restated_misses(asg, states, self.k)
        td, st = self.tc.round(pooled.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, locus_takes=takes)
        self.calls.append((int(asg["n_req"]), want, st))
        self.tds.append(td)
        return len(self.tds) - 1

    def remap(self, new_A, mapping):
        super().remap(new_A, mapping)
        self.tc.remap(new_A, mapping)

    def final(self):
        er, ea = self.tc.entries()
        td = self.tc.view()
        try:
            recs = capi.unpack_trace(capi.trace_dev_fetch(self.hmm, td), td.sizes()[0])
        finally:
            td.close()
        self.finals.append(dict(ent_read=er, ent_allele=ea, records=recs, pool_off=self.k.pool_off.copy(), stats=self.tc.stats()))
        return super().final()

    def close(self):
        if self.tc is not None:
            self.tc.close(); self.tc = None
        super().close()


def trace_lines(final, l):
    """The `trace p h ...` lines of flow_chain.dump_of for locus l of a pass, from the cache's own entries and view."""
    po = final["pool_off"]; out = []
    for r, h, t in zip(final["ent_read"], final["ent_allele"], final["records"]):
        if not (po[l] <= r < po[l + 1]):
            continue
        nostr = t["stutter_size"] == fc.NO_STR
        out.append("trace %d %d %s %d %s %d %d %s" % (r - po[l], h, t["hap_aln"], t["stutter_size"], t["cigar"], t["aln_start"], t["aln_stop"], "-" if nostr else t["str_seq"]))
    return out
