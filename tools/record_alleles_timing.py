"""The record's device calls of include/hipstr_hmm.h — hipstr_cigar_bp_diffs, hipstr_sample_histograms, hipstr_post_extract_vcf — each
against its host form on one thread.

Shapes: 256 loci x 1000 samples and 1000 loci x 100 samples, 5 reads per sample, V = 32 variants on 32 haplotypes, GL + PL requested.
  hipstr_cigar_bp_diffs       a read is 40M, an indel of up to three repeat units in every second read, 110M; the indel lies inside the region
  hipstr_sample_histograms    value = those sizes, every tenth read skipped
  hipstr_post_extract_vcf     on a launched posterior run; the host form is hipstr_post_extract followed by the gather through the index
                              rules in numpy, one fancy-indexed copy per locus and array (compiled loops; the python around them runs once
                              per locus)
Per call: wall time around the call with its results fetched, median of 9 after one warm-up call, device and host calls alternating.
Writes profiles/record_alleles_timing.txt.

Usage: python tools/record_alleles_timing.py [OUT_DIR]   (default profiles/; needs an MI355X)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi  # noqa: E402
import post_extract_vcf_cases as pc  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
med = lambda v: sorted(v)[len(v) // 2]
DEPTH, V, REPS = 5, 32, 9


def timed(dev, host, same):
    t_dev, t_host = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter(); a = dev(); t1 = time.perf_counter(); b = host(); t2 = time.perf_counter()
        if rep >= 1:
            t_dev.append(t1 - t0); t_host.append(t2 - t1)
        if rep == 0:
            same(a, b)
        del a, b
    return t_dev, t_host


def report(name, t_dev, t_host, n, unit, extra=""):
    d, h = med(t_dev), med(t_host)
    return ["  %s" % name,
            "    device call   %10.3f ms   (min %.3f, max %.3f)%s" % (d * 1e3, min(t_dev) * 1e3, max(t_dev) * 1e3, extra),
            "    host form     %10.3f ms   (min %.3f, max %.3f)   %.3f us per %s on one thread" % (h * 1e3, min(t_host) * 1e3, max(t_host) * 1e3, h / n * 1e6, unit),
            "    the device form %s at this shape: %.2f x the host form's time" % ("pays for itself" if d < h else "does NOT pay for itself", d / h)]


def host_gather(plain, S_of, n_variants, n2o_all):
    """hipstr_post_extract's flat gls / pls into the new order, a locus at a time (diploid loci of V variants each)."""
    gls = np.empty_like(plain["gls"]); pls = np.empty_like(plain["pls"])
    best = plain["best_gt"].copy()
    g0 = 0; s0 = 0; vo = 0
    for S, Vl in zip(S_of, n_variants):
        n2o = n2o_all[vo:vo + Vl].astype(np.int64)
        o2n = np.empty(Vl, np.int64); o2n[n2o] = np.arange(Vl)
        i, j = np.tril_indices(Vl)
        a = np.minimum(n2o[i], n2o[j]); b = np.maximum(n2o[i], n2o[j])
        src = b * (b + 1) // 2 + a
        G = len(src)
        gls[g0:g0 + S * G].reshape(S, G)[:] = plain["gls"][g0:g0 + S * G].reshape(S, G)[:, src]
        pls[g0:g0 + S * G].reshape(S, G)[:] = plain["pls"][g0:g0 + S * G].reshape(S, G)[:, src]
        best[s0:s0 + S] = o2n[best[s0:s0 + S]]
        g0 += S * G; s0 += S; vo += Vl
    return gls, pls, best


lines = ["The record's device calls against their host forms on one thread (tools/record_alleles_timing.py)",
         "wall time: host clock around the call (a device call ends with its results fetched); median of %d after one warm-up call" % REPS, ""]
for n_loci, S in ((256, 1000), (1000, 100)):
    rng = np.random.default_rng(n_loci)
    n_samp = n_loci * S; n = n_samp * DEPTH
    lines.append("%d loci x %d samples, %d reads per sample (%d reads), V = %d" % (n_loci, S, DEPTH, n, V))
    # ---- CIGARs: built as arrays (three or two runs per read)
    unit = rng.integers(2, 7, size=n_loci)
    indel = rng.integers(-3, 4, size=n) * np.repeat(unit, S * DEPTH) * (np.arange(n) % 2)
    runs = np.where(indel != 0, 3, 2)
    coff = np.concatenate([[0], np.cumsum(runs)]).astype(np.int32)
    op = np.full(coff[-1], ord("M"), np.uint8); ln = np.full(coff[-1], 40, np.int32)
    ln[coff[1:] - 1] = 110
    mid = coff[:-1][indel != 0] + 1
    op[mid] = np.where(indel[indel != 0] > 0, ord("I"), ord("D")); ln[mid] = np.abs(indel[indel != 0])
    rs = rng.integers(1000, 100000, size=n_loci).astype(np.int32)
    start = (np.repeat(rs, S * DEPTH) - rng.integers(20, 36, size=n)).astype(np.int32)
    rq = dict(n_loci=n_loci, read_off=(np.arange(n_loci + 1) * S * DEPTH).astype(np.int32), read_start=start, cigar_off=coff, cigar_op=op, cigar_len=ln,
              region_start=rs, region_stop=(rs + 40).astype(np.int32), pad=unit.astype(np.int32))
    def same_cigars(a, b):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].all() and np.array_equal(a[1], indel)
    td, th = timed(lambda: capi.run_cigar_bp_diffs(hmm, rq), lambda: capi.run_cigar_bp_diffs(hmm, rq, host=True), same_cigars)
    last = capi.record_reads_last(hmm)
    lines += report("hipstr_cigar_bp_diffs", td, th, n, "read", "   %d bytes up, %d bytes down" % (last["bytes_up"], last["bytes_down"]))
    # ---- histograms
    lab = np.tile(np.repeat(np.arange(S), DEPTH), n_loci)
    pb_kw = dict(n_alleles=np.full(n_loci, V, np.int32), n_samples=np.full(n_loci, S, np.int32), read_off=rq["read_off"], sample_label=lab,
                 log_p1=-rng.random(n), log_p2=-rng.random(n), read_weight=np.ones(n, np.int32))
    pb = capi.PostBatch(log_aln_probs=(-rng.random(n * V) * 30), **pb_kw)
    value = np.where(np.arange(n) % 10 == 9, capi.NO_ML_BP, indel).astype(np.int32)
    def same_hist(a, b):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[0][-1] > 0
    td, th = timed(lambda: capi.run_sample_histograms(hmm, pb, value, capi.NO_ML_BP), lambda: capi.run_sample_histograms(hmm, pb, value, capi.NO_ML_BP, host=True), same_hist)
    last = capi.record_reads_last(hmm)
    lines += report("hipstr_sample_histograms", td, th, n_samp, "sample", "   %d bytes up, %d bytes down" % (last["bytes_up"], last["bytes_down"]))
    # ---- the genotype outputs in the record's order
    nv = np.full(n_loci, V, np.int32); h2a = np.tile(np.arange(V, dtype=np.int32), n_loci)
    n2o, o2n = pc.orders(7, nv)
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd, hmm.hipstr_last_error()
    assert hmm.hipstr_post_launch(pd, None) == 0, hmm.hipstr_last_error()
    kw = dict(calc_gls=True, calc_pls=True, calc_phased_gls=False, pd=pd, room_for_unrequested=False)
    t_plain = []
    def host_form():
        t0 = time.perf_counter()
        plain = capi.run_post_extract_flat(hmm, pb, nv, h2a, **kw)
        t_plain.append(time.perf_counter() - t0)
        return host_gather(plain, [S] * n_loci, nv, n2o)
    def same_gt(a, b):
        assert np.array_equal(a["gls"].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a["pls"], b[1]) and np.array_equal(a["best_gt"], b[2])
    td, th = timed(lambda: capi.run_post_extract_flat(hmm, pb, nv, h2a, order=(n2o, o2n), **kw), host_form, same_gt)
    hmm.hipstr_post_free(pd)
    lines += report("hipstr_post_extract_vcf (GL + PL: %d values per sample)" % (V * (V + 1) // 2), td, th, n_samp, "sample")
    lines += ["    (of the host form, hipstr_post_extract takes %.3f ms in the same calls: the gather is the rest)" % (med(t_plain[1:]) * 1e3), ""]
    print("\n".join(lines[-16:]), flush=True)
lines.append("(all times include the python wrapper, which allocates and fills the output arrays per call)")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "record_alleles_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
