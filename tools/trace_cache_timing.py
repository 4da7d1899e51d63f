"""What the trace cache (hipstr_trace_cache_round, include/hipstr_hmm.h) costs and saves against the plain resident traceback call, which it
does not change and which is therefore the yardstick.  One device, one process:

  synthetic batch   NL loci x P reads x A alleles, one request per read (about NL*P requests):
                      hipstr_hmm_trace_resident on the full list
                      hipstr_trace_cache_round, first round (empty cache: all misses), second round (a cache that lacks 2 % of the keys),
                      all-hit round; the gather's own kernel time (events, HIPSTR_TRACE_GATHER_TIMING) and the bytes that cross the host link
  twelve flow loci  tests/flow_chain.py's batch through genotype() on the device backend and on tests/flow_chain_cache.py's: the first
                    pass' four trace calls (three rounds and the EM's retrace), each call's wall time, summed, both ways

Synthetic batch: only the C calls are timed (arguments converted before).  Flow loci: the capi wrapper of either call, its argument
conversion included (the same on both sides).  One warm-up, then REPS runs, the median with the fastest and the slowest beside it.
Usage: python tools/trace_cache_timing.py [OUT.txt [COMMIT]]   (default profiles/trace_cache_timing.txt; needs an MI355X)."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi

NL, P, A_STR, REPS = 256, 40, 8, 9
FLOW_REPS = REPS


def med(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def fmt(v):
    m, lo, hi = med(v)
    return "%8.3f ms  (%.3f .. %.3f)" % (m * 1e3, lo * 1e3, hi * 1e3)


class Calls:
    """The C calls with their arguments converted once."""

    def __init__(self, hmm, bptr, rr, aa, h2r_list):
        self.hmm, self.bptr = hmm, bptr
        self.rr = np.ascontiguousarray(rr, np.int32); self.aa = np.ascontiguousarray(aa, np.int32); self.n = len(self.rr)
        self.h2r = (C.c_char_p * len(h2r_list))(*h2r_list)
        self.st = capi.HipstrTraceCacheStats()

    def fresh(self, n=None):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = self.hmm.hipstr_hmm_trace_resident(self.bptr, self.n if n is None else n, self.rr.ctypes.data_as(capi._i32p), self.aa.ctypes.data_as(capi._i32p), None, self.h2r, 0, C.byref(h))
        t = time.perf_counter() - t0
        assert rc == 0, self.hmm.hipstr_last_error()
        self.hmm.hipstr_trace_dev_free(h)
        return t

    def round(self, tc, rr=None, aa=None):
        rr = self.rr if rr is None else rr; aa = self.aa if aa is None else aa
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = self.hmm.hipstr_trace_cache_round(tc.h, self.bptr, len(rr), rr.ctypes.data_as(capi._i32p), aa.ctypes.data_as(capi._i32p), None, self.h2r, None, C.byref(h), C.byref(self.st))
        t = time.perf_counter() - t0
        assert rc == 0, self.hmm.hipstr_last_error()
        self.hmm.hipstr_trace_dev_free(h)
        return t, int(self.st.n_misses)


def synthetic(hmm, oracle):
    sb = capi.SynthBatch(n_loci=NL, reads_per_locus=P, n_str_alleles=A_STR, seed=1000)
    seeds = np.zeros(sb.n_reads, np.int32)
    assert hmm.hipstr_calc_seed_bases(sb.ptr, seeds.ctypes.data_as(capi._i32p)) == 0, hmm.hipstr_last_error()
    A = sb.n_out // sb.n_reads
    reads = np.nonzero(seeds >= 0)[0].astype(np.int32)
    rr = reads; aa = (reads % A).astype(np.int32)
    pool_off = capi.batch_arrays(sb.ptr)["read_off"].astype(np.int32)
    h2r = capi.hap_aln_info(hmm, "hipstr_", sb.ptr)
    c = Calls(hmm, sb.ptr, rr, aa, h2r)
    most = np.ones(len(rr), bool); most[::50] = False                 # 2 % of the keys are left out of the second round's cache
    new = lambda: capi.TraceCache(hmm, pool_off, np.full(NL, A, np.int32))
    t_fresh, t_first, t_second, t_hit = [], [], [], []
    miss = {}
    for rep in range(REPS + 1):
        f = c.fresh()
        tc = new(); a, miss["first"] = c.round(tc); tc.close()
        tc = new(); c.round(tc, c.rr[most], c.aa[most]); b, miss["second"] = c.round(tc)
        h, miss["hit"] = c.round(tc); tc.close()
        if rep:                                                        # (the first turn is the warm-up)
            t_fresh.append(f); t_first.append(a); t_second.append(b); t_hit.append(h)
    os.environ["HIPSTR_TRACE_GATHER_TIMING"] = "1"
    tc = new(); c.round(tc)
    k_ms = []
    for rep in range(REPS + 1):
        c.round(tc)
        last = capi.trace_gather_last(hmm)
        if rep:
            k_ms.append(last["kernel_ms"] * 1e-3)
    del os.environ["HIPSTR_TRACE_GATHER_TIMING"]
    td, _ = tc.round(sb.ptr, rr, aa, hap_to_ref=h2r)
    _, tot = td.sizes(); td.close(); tc.close()
    rec_bytes = int(tot[[0, 1, 2, 6]].sum() + 8 * tot[3] + 5 * tot[4] + 5 * tot[5]) + c.n * (8 + 6 * 4 + 8 * 4)
    sb.close()
    return dict(n=c.n, A=A, fresh=t_fresh, first=t_first, second=t_second, hit=t_hit, miss=miss, kernel=k_ms, last=last, rec_bytes=rec_bytes)


def flow(hmm, oracle):
    import flow_chain as fc
    import flow_chain_cache as fcc

    class Timed:
        def trace(self, pooled, asg, states):
            h2r = capi.hap_aln_info(self.hmm, "hipstr_", pooled.ptr)
            t0 = time.perf_counter()
            td = self.call(pooled, asg, states, h2r)
            self.times.append(time.perf_counter() - t0)
            self.tds.append(td)
            return len(self.tds) - 1

    class Plain(Timed, fc.DeviceBackend):
        def call(self, pooled, asg, states, h2r):
            self.misses.append((int(asg["n_req"]), int(asg["n_req"])))
            return capi.run_trace_resident(self.hmm, pooled.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, flags=0)

    class Cached(Timed, fcc.CachedDeviceBackend):
        def call(self, pooled, asg, states, h2r):
            takes = np.array([s.phase != fc.DONE for s in states], np.uint8)
            td, st = self.tc.round(pooled.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, locus_takes=takes)
            self.misses.append((int(asg["n_req"]), st["n_misses"]))
            return td

    out = {}
    for name, cls in (("plain", Plain), ("cached", Cached)):
        sums, per_call = [], []
        for rep in range(FLOW_REPS + 1):
            be = cls(hmm); be.times = []; be.misses = []
            try:
                fc.run(list(fc.CASES), be, oracle, None)
            finally:
                be.close()
            if rep:
                sums.append(sum(be.times[:4])); per_call.append(be.times[:4])
        out[name] = dict(sums=sums, per_call=per_call, misses=be.misses[:4], n_calls=len(be.times))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "trace_cache_timing.txt")
    commit = sys.argv[2] if len(sys.argv) > 2 else "a tree whose commit was not given"
    hmm = capi.load_hmm(); oracle = capi.load_oracle()
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
    s = synthetic(hmm, oracle); f = flow(hmm, oracle)
    hit_m, fresh_m = med(s["hit"])[0], med(s["fresh"])[0]
    plain_m, cached_m = med(f["plain"]["sums"])[0], med(f["cached"]["sums"])[0]
    L = ["Trace cache: only the (pool, haplotype) pairs not yet seen are traced (tools/trace_cache_timing.py)",
         "==================================================================================================", "",
         "STATUS: MEASURED on one MI355X, %s.  Wall time of the C calls alone, one warm-up, then the median of %d runs (fastest .. slowest)." % (commit, REPS), "",
         "Synthetic batch: %d loci x %d reads x %d haplotypes, one request per seeded read: %d requests." % (NL, P, s["A"], s["n"]),
         "  hipstr_hmm_trace_resident, the full list (the yardstick)     %s" % fmt(s["fresh"]),
         "  hipstr_trace_cache_round, first round   (%6d misses)       %s" % (s["miss"]["first"], fmt(s["first"])),
         "  hipstr_trace_cache_round, second round  (%6d misses)       %s" % (s["miss"]["second"], fmt(s["second"])),
         "  hipstr_trace_cache_round, all-hit round (%6d misses)       %s" % (s["miss"]["hit"], fmt(s["hit"])),
         "  the gather's three kernels in the all-hit round (events)     %s" % fmt(s["kernel"]),
         "  bytes over the host link per gather: %d up (out_src, out_idx, the sources' pointer table), %d down (the pool totals);" % (s["last"]["bytes_up"], s["last"]["bytes_home"]),
         "  the records it moves device-to-device: %d bytes." % s["rec_bytes"], "",
         "Twelve flow loci (tests/flow_chain.py) as one batch, first pass: four trace calls of %d requests, median of %d runs of the whole chain." % (f["plain"]["misses"][0][0], FLOW_REPS),
         "  misses per call with the cache: %s" % " / ".join(str(m) for _, m in f["cached"]["misses"]),
         "  hipstr_hmm_trace_resident x 4, summed                        %s" % fmt(f["plain"]["sums"]),
         "  hipstr_trace_cache_round x 4, summed                         %s" % fmt(f["cached"]["sums"])]
    for name in ("plain", "cached"):
        calls = np.median(np.array(f[name]["per_call"]), axis=0)
        L.append("    %-6s per call: %s ms" % (name, "  ".join("%.3f" % (x * 1e3) for x in calls)))
    L += ["",
          "The two claims:",
          "  an all-hit round costs less than the fresh trace of the same list: %s (%.3f ms against %.3f ms)" % ("HOLDS" if hit_m < fresh_m else "DOES NOT HOLD", hit_m * 1e3, fresh_m * 1e3),
          "  the first pass' trace time drops: %s (%.3f ms against %.3f ms, %.2fx)" % ("HOLDS" if cached_m < plain_m else "DOES NOT HOLD", cached_m * 1e3, plain_m * 1e3, plain_m / cached_m),
          "  the first round pays the gather on top of the same traceback: %.3f ms against %.3f ms." % (med(s["first"])[0] * 1e3, fresh_m * 1e3)]
    text = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
