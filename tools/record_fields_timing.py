"""hipstr_record_fields on the device against its host form on one thread, and the parity record of hipstr_bias_pvalues.

Shapes: 256 loci x 1000 samples at 5 reads per sample and 1000 loci x 100 samples at 6 reads per sample — the per-sample depths of bench.py's
c4 and c3 (the locus' reads dealt to its samples in equal blocks) — and, for scale, the same two shapes at 30 reads per sample.  Of a
sample's reads 80 % fall inside the strand tolerance (uniq_one + uniq_two), split between the haplotypes and the strands by fair coins.
Every sample's MAP pair is forced heterozygous by two reads of a real hipstr_post_upload + hipstr_post_launch, so every sample's p-values
are computed: the most work the shape can ask for.

Per shape: wall time of the device call (a host clock around the call, which ends in the fetch of its results: median of 9 after 2 warm-up
calls, device and host calls alternating), bytes up and down (hipstr_debug_record_last), the host form's wall time and microseconds per
sample.  Writes profiles/record_fields_timing.txt and profiles/record_fields_parity.txt (the values of hipstr_bias_pvalues on
tests/golden/record_pvalues.npz that are not bit-identical to the host form, and their largest distance in ulps).

Usage: python tools/record_fields_timing.py [OUT_DIR]   (default profiles/; needs an MI355X)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi  # noqa: E402
import record_cases as rc  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
med = lambda v: sorted(v)[len(v) // 2]


def shape(n_loci, S, depth, seed):
    rng = np.random.RandomState(seed)
    n, A = n_loci * S, 4
    ha = rng.randint(0, A, n); hb = (ha + 1 + rng.randint(0, A - 1, n)) % A            # heterozygous pairs
    ll = np.full((n, 2, A), -50.0)
    ll[np.arange(n), 0, ha] = 0.0; ll[np.arange(n), 1, hb] = 0.0
    p1 = np.tile([0.0, -1000.0], n); p2 = np.tile([-1000.0, 0.0], n)
    lab = np.tile(np.repeat(np.arange(S), 2), n_loci)
    pb = capi.PostBatch(np.full(n_loci, A, np.int32), np.full(n_loci, S, np.int32), np.arange(n_loci + 1, dtype=np.int32) * 2 * S, lab, p1, p2,
                        np.ones(2 * n, np.int32), ll.reshape(-1))
    tot = rng.binomial(depth, 0.8, n)
    u1 = rng.binomial(tot, 0.5); u2 = tot - u1
    counts = dict(n_aligned=np.full(n, depth), n_snp=rng.binomial(depth, 0.3, n), n_stutter=rng.binomial(depth, 0.1, n),
                  n_flank_indel=rng.binomial(depth, 0.02, n), uniq_one=u1, uniq_two=u2, rv_uniq_one=rng.binomial(u1, 0.5), rv_uniq_two=rng.binomial(u2, 0.5))
    return pb, np.stack([ha, hb], 1).astype(np.int32), counts, np.full(n_loci, A, np.int32), np.tile(np.arange(A, dtype=np.int32), n_loci)


lines = ["hipstr_record_fields: device call against hipstr_record_fields_host on one thread (tools/record_fields_timing.py)",
         "wall time: host clock around the call (the device call ends with its results fetched); median of 9 after 2 warm-up calls", ""]
for n_loci, S, depth in ((256, 1000, 5), (1000, 100, 6), (256, 1000, 30), (1000, 100, 30)):
    pb, pairs, counts, nv, h2a = shape(n_loci, S, depth, 11)
    n = n_loci * S
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd, hmm.hipstr_last_error()
    assert hmm.hipstr_post_launch(pd, None) == 0, hmm.hipstr_last_error()
    post = np.zeros(int(pb.post_off[-1])); tt = np.zeros(n); gt = np.zeros(2 * n, np.int32); lt = np.zeros(n_loci)
    assert hmm.hipstr_post_fetch(pd, post.ctypes.data_as(capi._f64p), tt.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p), lt.ctypes.data_as(capi._f64p)) == 0
    assert np.array_equal(gt.reshape(-1, 2), pairs)
    t_dev, t_host = [], []
    for rep in range(11):
        t0 = time.perf_counter()
        got = capi.run_record_fields(hmm, pb, nv, h2a, counts, pd=pd)
        t1 = time.perf_counter()
        want = capi.run_record_fields(hmm, pb, nv, h2a, counts, map_gt=gt)
        t2 = time.perf_counter()
        if rep >= 2:
            t_dev.append(t1 - t0); t_host.append(t2 - t1)
    last = capi.record_last(hmm)
    for key in rc.INT_KEYS:
        assert np.array_equal(got[key], want[key]), key
    for key in ("ab", "fs"):
        fin = np.isfinite(want[key])
        assert np.array_equal(np.isfinite(got[key]), fin) and np.all(np.abs(got[key][fin] - want[key][fin]) <= 1e-9), key
    d, h = med(t_dev), med(t_host)
    lines += ["%d loci x %d samples, %d reads per sample (%d samples, every p-value computed)" % (n_loci, S, depth, n),
              "  device call   %9.3f ms   (min %.3f, max %.3f)   %d bytes up, %d bytes down" % (d * 1e3, min(t_dev) * 1e3, max(t_dev) * 1e3, last["bytes_up"], last["bytes_down"]),
              "  host form     %9.3f ms   (min %.3f, max %.3f)   %.3f us per sample on one thread" % (h * 1e3, min(t_host) * 1e3, max(t_host) * 1e3, h / n * 1e6),
              "  the device form %s at this shape: %.2f x the host form's time" % ("pays for itself" if d < h else "does NOT pay for itself", d / h), ""]
    print("\n".join(lines[-5:]), flush=True)
    hmm.hipstr_post_free(pd)
lines.append("(both times include the python wrapper, which allocates the output arrays per call and, for the device call, packs nothing: the library packs)")
os.makedirs(OUT, exist_ok=True)
with open(os.path.join(OUT, "record_fields_timing.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")

# ---- parity of hipstr_bias_pvalues on the golden
u1, u2, r1, r2, ab_g, fs_g = rc.all_quadruples()
dev = capi.bias_pvalues(hmm, u1, u2, r1, r2); host = capi.bias_pvalues(hmm, u1, u2, r1, r2, host=True)
par = ["hipstr_bias_pvalues on tests/golden/record_pvalues.npz: device against the host form (tools/record_fields_timing.py)",
       "%d quadruples; a record, not a threshold (the bound is 1e-9 absolute, tests/test_record_gpu.py)" % len(u1)]
for nm, d, h in (("ab", dev[0], host[0]), ("fs", dev[1], host[1])):
    fin = np.isfinite(h)
    assert np.array_equal(np.isfinite(d), fin)
    differ = fin & (d.view(np.uint64) != h.view(np.uint64))
    ul = rc.ulps(d[differ], h[differ])
    par.append("%s: %d of %d finite values not bit-identical; largest distance %d ulp, largest absolute difference %.3g; by distance: %s"
               % (nm, int(differ.sum()), int(fin.sum()), int(ul.max()) if len(ul) else 0, float(np.max(np.abs(d[differ] - h[differ]))) if differ.any() else 0.0,
                  ", ".join("%d ulp: %d" % (k, int(np.sum(ul == k))) for k in sorted(set(ul.tolist()))[:8])))
print("\n".join(par), flush=True)
with open(os.path.join(OUT, "record_fields_parity.txt"), "w") as f:
    f.write("\n".join(par) + "\n")
