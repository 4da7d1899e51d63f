"""The read pooler in front of the forward pass, timed on one device: hipstr_pool_reads at the north-star shape with two reads per pool
(1000 loci x 1000 un-pooled reads x 150 bp), at the per-locus shape of BASELINE configs[2] (600 reads in 260 pools; 2000 loci per call) and
at one NS locus per call — the call, its kernels from HIP events (HIPSTR_POOL_TIMING), the bytes each way over the host link and the host's
staging of the reads.  Baseline: the compiled reference's ReadPooler (ref_pool of oracle/_ref/libhipstr_ref.so, looped over the loci) on
the same machine's host, one thread; skipped where the reference is not built.  hipstr_pool_reads_host is printed beside them for
information: it is this library's code, so it is no baseline.  The outputs of the three are checked to be identical.
A measurement, not a test.  Usage: python tools/pool_timing.py [OUT.txt]  (default profiles/pool_timing.txt; needs an MI355X)."""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hipstr_amd import capi

os.environ["HIPSTR_POOL_TIMING"] = "1"
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
REPS = 5
lines = []
def say(s):
    print(s, flush=True); lines.append(s)
med = lambda v: sorted(v)[len(v) // 2]


def unpooled(nl, reads, pools, length=150, seed=1):
    """nl loci of `reads` reads of `length` bases in `pools` pools each (every pool has a member; the rest are dealt at random), qualities
    of Phred 30..40 written as Phred+33 (bytes 63..73); the haplotype tables are the smallest consistent ones (the pooler does not read them)."""
    rng = np.random.default_rng(seed)
    seqs = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (nl, pools, length))]
    which = np.concatenate([np.tile(np.arange(pools), (nl, 1)), rng.integers(0, pools, (nl, reads - pools))], axis=1)
    which = rng.permuted(which, axis=1)
    bases = np.take_along_axis(seqs, which[:, :, None], axis=1)
    quals = rng.integers(63, 74, bases.shape).astype(np.uint8)
    n = nl * reads
    a = dict(blk_start=np.tile([100, 110, 120], nl).astype(np.int32), blk_end=np.tile([110, 120, 130], nl).astype(np.int32),
             blk_nopts=np.ones(3 * nl, np.int32), period=np.full(nl, 4, np.int32), stutter=np.tile([0.9, 0.05, 0.05, 0.7, 0.005, 0.005], nl),
             opt_off=(np.arange(3 * nl + 1) * 10).astype(np.int32), seq=b"ACGTACGTAC" * (3 * nl) + b"\0", hap_off=np.arange(nl + 1, dtype=np.int32),
             read_off=(np.arange(nl + 1) * reads).astype(np.int32), base_off=(np.arange(n + 1) * length).astype(np.int32),
             bases=bases.tobytes() + b"\0", quals=quals.tobytes() + b"\0", read_start=np.zeros(n, np.int32),
             cigar_off=np.arange(n + 1, dtype=np.int32), cigar_op=b"=" * n + b"\0", cigar_len=np.full(n, length, np.int32))
    return a


def struct_of(a, l0=None):
    """hipstr_batch_t over the arrays; l0: the one-locus batch of locus l0 (offsets rebased: ref_pool takes one locus)."""
    s = capi.HipstrBatch()
    if l0 is None:
        v = a
    else:
        r0, r1 = int(a["read_off"][l0]), int(a["read_off"][l0 + 1]); b0, b1 = int(a["base_off"][r0]), int(a["base_off"][r1])
        v = dict(a, blk_start=a["blk_start"][3 * l0:3 * l0 + 3].copy(), blk_end=a["blk_end"][3 * l0:3 * l0 + 3].copy(), blk_nopts=a["blk_nopts"][:3].copy(),
                 period=a["period"][:1].copy(), stutter=a["stutter"][:6].copy(), opt_off=a["opt_off"][:4].copy(), hap_off=a["hap_off"][:2].copy(),
                 read_off=np.array([0, r1 - r0], np.int32), base_off=(a["base_off"][r0:r1 + 1] - b0).astype(np.int32),
                 bases=a["bases"][b0:b1] + b"\0", quals=a["quals"][b0:b1] + b"\0", read_start=a["read_start"][r0:r1].copy(),
                 cigar_off=np.arange(r1 - r0 + 1, dtype=np.int32), cigar_op=b"=" * (r1 - r0) + b"\0", cigar_len=a["cigar_len"][r0:r1].copy())
    s.n_loci = len(v["period"])
    for k in ("blk_start", "blk_end", "blk_nopts", "period", "opt_off", "hap_off", "read_off", "base_off", "read_start", "cigar_off", "cigar_len"):
        setattr(s, k, v[k].ctypes.data_as(capi._i32p))
    s.stutter = v["stutter"].ctypes.data_as(capi._f64p)
    s.seq, s.bases, s.quals, s.cigar_op = v["seq"], v["bases"], v["quals"], v["cigar_op"]
    s._keepalive = v
    return s


def timed_pool(s, host):
    t0 = time.perf_counter(); out = capi.run_pool(hmm, C.byref(s), host=host); return time.perf_counter() - t0, out


def shape(title, nl, reads, pools, per_call=None):
    a = unpooled(nl, reads, pools)
    s = struct_of(a)
    nbytes = int(a["base_off"][-1])
    say("%s: %d loci x %d reads x 150 bp in %d pools per locus (%.0f MB of bases + as many of qualities)" % (title, nl, reads, pools, nbytes / 1e6))
    calls = [s] if per_call is None else [struct_of(a, l) for l in range(per_call)]
    dev_t, ker, up, down, stage = [], [], [], [], []
    for rep in range(REPS + 1):
        t = k = u = d = st = 0.0
        for c in calls:
            dt, out = timed_pool(c, False); tm = capi.pool_last_timing(hmm)
            t += dt; k += tm["kernel_ms"]; u += tm["bytes_up"]; d += tm["bytes_down"]; st += tm["stage_s"]
        if rep:          # (the first pass fills the block caches)
            dev_t.append(t / len(calls)); ker.append(k / len(calls)); up.append(u / len(calls)); down.append(d / len(calls)); stage.append(st / len(calls))
    last = capi.pool_last(hmm)
    host_t = []
    for rep in range(3):
        t = 0.0
        for c in calls:
            dt, hout = timed_pool(c, True); t += dt
        host_t.append(t / len(calls))
    assert all(np.array_equal(out[k], hout[k]) for k in capi.POOL_FIELDS), "device and host twin disagree"
    loci_per_call = nl if per_call is None else 1
    say("  hipstr_pool_reads (median of %d, per call of %d loci; ctypes wrapper and output allocation included): %.2f ms = %.4f ms per locus; kernels %.3f ms; staging the reads on the host %.2f ms; %.1f MB up, %.1f MB down; last call: %s"
        % (REPS, loci_per_call, 1e3 * med(dev_t), 1e3 * med(dev_t) / loci_per_call, med(ker), 1e3 * med(stage), med(up) / 1e6, med(down) / 1e6, last))
    say("  hipstr_pool_reads_host (this library's host twin, one thread; for information): %.2f ms per call = %.4f ms per locus" % (1e3 * med(host_t), 1e3 * med(host_t) / loci_per_call))
    if capi.have_ref():
        ref = capi.load_ref()
        ref.ref_pool.restype = C.c_int; ref.ref_pool.argtypes = [capi._BP, capi._i32p, capi._i32p, C.c_char_p, capi._i32p, C.c_int32]
        n_ref = min(nl, 100)
        ones = [struct_of(a, l) for l in range(n_ref)]
        cap = reads * 151 + 16
        pi = np.zeros(reads, np.int32); npl = np.zeros(1, np.int32); pq = C.create_string_buffer(cap); pqo = np.zeros(reads + 1, np.int32)
        t0 = time.perf_counter()
        for l, o in enumerate(ones):
            assert ref.ref_pool(C.byref(o), pi.ctypes.data_as(capi._i32p), npl.ctypes.data_as(capi._i32p), pq, pqo.ctypes.data_as(capi._i32p), cap) == 0
            if l == 0:
                P = int(npl[0]); h0 = capi.run_pool(hmm, C.byref(o), host=True)
                assert np.array_equal(pi, h0["pool_index"]) and P == h0["n_pools"][0] and pq.raw[:pqo[P]] == h0["pool_quals"][:pqo[P]].tobytes(), "the reference disagrees"
        t_ref = (time.perf_counter() - t0) / n_ref
        say("  baseline: the compiled reference's ReadPooler, one host thread (%d loci, one Alignment object per read built from the batch included): %.3f ms per locus; "
            "the device call takes %.2fx of that per locus" % (n_ref, 1e3 * t_ref, med(dev_t) / loci_per_call / t_ref))
    else:
        say("  baseline: the compiled reference is not built here: NOT MEASURED")


shape("NS, two reads per pool", 1000, 1000, 500)
shape("configs[2] per-locus shape", 2000, 600, 260)
shape("one NS locus per call", 64, 1000, 500, per_call=64)
say("outputs of device, host twin and (first locus) the reference's pooler are identical")
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pool_timing.txt")
open(OUT, "w").write("\n".join(lines) + "\n")
