"""The haplotype generator in front of the pooler, timed on one device: hipstr_hapgen at the flow shape (768 loci x ~100 reads x 10 samples)
and at the north-star read count (1000 loci x 500 reads) — the call (wall time, ctypes wrapper and output allocation included), its kernels
from HIP events (HIPSTR_HAPGEN_TIMING), the bytes each way and the host's staging; beside it hipstr_hapgen_host on one thread (this
library's code: no baseline) and the baseline: the REFERENCE's own HaplotypeGenerator, timed inside `genotype_flow --hapgen-cases --time`
(oracle/_ref, one host thread, the Alignment objects built outside the timed part) on the same machine.  One warm-up call, then the median
of five, as the measuring guide asks; the outputs of device and host twin are checked to be identical, the reference's blocks to equal them.
A measurement, not a test.  Usage: python tools/hapgen_timing.py [OUT.txt]  (default profiles/hapgen_timing.txt; needs an MI355X)."""
import os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi
import hapgen_cases as hc

os.environ["HIPSTR_HAPGEN_TIMING"] = "1"
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
REPS = 5
REFDIR = os.path.join(ROOT, "oracle", "_ref")
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
med = lambda v: sorted(v)[len(v) // 2]


def loci_of(n_loci, n_reads, n_samples, seed):
    """Loci as integration/genotype_flow.cpp simulates them: periods 2..5, about 40 bases of repeat, reads of 100-125 bases on a coarse grid
    of starts, 80 % spanning, stutter of one unit in 14 % of the reads, two alleles per sample."""
    rng = np.random.default_rng(seed)
    loci = []
    for l in range(n_loci):
        period = 2 + l % 4
        motif = hc.rand_seq(rng, period)
        while motif == motif[0] * period:
            motif = hc.rand_seq(rng, period)
        copies = max(3, 40 // period)
        chrom, a, b = hc.chrom_with_repeat(rng, 300, motif, copies, tail=300)
        rs, re = a - 5, b + 5
        genotype = rng.integers(-2, 3, (n_samples, 2))
        reads = []
        for k in range(n_reads + int(rng.integers(-2, 3))):
            s = int(rng.integers(0, n_samples))
            d = int(genotype[s, int(rng.integers(0, 2))])
            u = rng.random()
            d += 1 if u < 0.06 else -1 if u < 0.14 else 0
            edits = [("I", 5, d * period)] if d > 0 else [("D", 5, -d * period)] if d < 0 and copies + d >= 1 else []
            length = 100 + 5 * int(rng.integers(0, 6))
            if rng.random() < 0.8:
                start = a - 22 - 6 * int(rng.integers(0, 7)); end = max(start + length, re + 2)
                reads.append(hc.padded_read(chrom, rs, re, edits, start=start, end=end, sample=s, ins=motif * 3))
            else:
                start = a - int(rng.integers(70, 96)) if rng.random() < 0.5 else a + int(rng.integers(4, 20))
                reads.append(hc.read(chrom, start, [("=", length)], sample=s))
        loci.append(hc.locus("l%d" % l, chrom, a, b, period, n_samples, reads))
    return loci


def shape(title, n_loci, n_reads, n_samples, n_ref):
    loci = loci_of(n_loci, n_reads, n_samples, 7)
    b = hc.ReadsBatch(loci); rq = hc.request_of(loci)
    say("%s: %d loci, %d reads, %d samples per locus, %.1f MB of bases" % (title, n_loci, b.n_reads, n_samples, len(b.a["bases"]) / 1e6))
    dev_t, ker, up, down, stage = [], [], [], [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter(); got = capi.run_hapgen(hmm, b.ptr, rq); dt = time.perf_counter() - t0
        tm = capi.hapgen_last_timing(hmm)
        if rep:          # (the first call fills the block caches)
            dev_t.append(dt); ker.append(tm["kernel_ms"]); up.append(tm["bytes_up"]); down.append(tm["bytes_down"]); stage.append(tm["stage_s"])
    last = capi.hapgen_last(hmm)
    host_t = []
    for rep in range(3):
        t0 = time.perf_counter(); host = capi.run_hapgen(hmm, b.ptr, rq, host=True); host_t.append(time.perf_counter() - t0)
    hc.assert_same(got, host, "device and host twin disagree")
    say("  hipstr_hapgen (median of %d after a warm-up): %.2f ms per call = %.4f ms per locus; kernels %.3f ms; staging on the host %.2f ms; %.1f MB up, %.1f MB down; "
        "last call: %s" % (REPS, 1e3 * med(dev_t), 1e3 * med(dev_t) / n_loci, med(ker), 1e3 * med(stage), med(up) / 1e6, med(down) / 1e6, last))
    say("  hipstr_hapgen_host (this library's host twin, one thread; for information): %.2f ms per call = %.4f ms per locus" % (1e3 * med(host_t), 1e3 * med(host_t) / n_loci))
    launcher = os.path.join(REFDIR, "flow_launcher")
    if os.path.exists(launcher) and os.path.exists(os.path.join(REFDIR, "libflow_ref.so")):
        sub = loci[:n_ref]
        with tempfile.TemporaryDirectory() as tmp:
            src, dst = os.path.join(tmp, "cases.txt"), os.path.join(tmp, "records.txt")
            open(src, "w").write(hc.case_text(sub))
            subprocess.run([launcher, os.path.join(REFDIR, "libflow_ref.so"), "--hapgen-cases", src, "--out", dst, "--time", str(REPS)], check=True)
            text = open(dst).read()
        recs = hc.parse_records(text)
        for l, lc in enumerate(sub):
            assert recs[lc["name"]]["status"] == int(got["status"][l]) and (recs[lc["name"]]["blocks"] or [(0, 0, [])] * 3) == hc.blocks_of(got, l), "the reference disagrees"
        secs, cases, reps = [x for x in text.splitlines() if x.startswith("time ")][0].split(" ")[1:]
        t_ref = float(secs) / (int(cases) * int(reps))
        say("  baseline: the reference's HaplotypeGenerator, one host thread (%d loci x %d repeats, mean): %.4f ms per locus; the device call takes %.2fx of that per locus, "
            "its kernels %.3fx" % (int(cases), int(reps), 1e3 * t_ref, med(dev_t) / n_loci / t_ref, 1e-3 * med(ker) / n_loci / t_ref))
    else:
        say("  baseline: the compiled reference is not built here: NOT MEASURED")


shape("flow shape", 768, 100, 10, 768)
shape("north-star read count", 1000, 500, 10, 100)
say("outputs of device and host twin are identical; the reference's blocks equal them on the loci it was given")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "hapgen_timing.txt")
open(OUT, "w").write("\n".join(lines) + "\n")
