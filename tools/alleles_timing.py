"""hipstr_alleles_step on the host and on the device — wall time, bytes up, bytes home — at the two shapes that decide which form flags = 0
runs, each beside the kernel time of the forward round the step prepares (hipstr_hmm_align_timed over hipstr_alleles_batch: only the added
haplotypes are aligned):
  north   1000 loci, A = 32 -> 36, haplotypes of about 150 bp: the north-star round
  wide      64 loci, A = 500 -> 1000, STR alleles of 500 bp
The census is synthetic: every locus is in phase ADD and gets its candidates (options of block 1 with a tail no option has), so the call
adds them and computes mapping, mask and hap_to_allele for every locus.  The two forms are timed alternately in one process, the C call
alone (the ctypes structures are built once); each call's result is freed inside the timed window, as a caller would.
Usage: python tools/alleles_timing.py [OUT.txt [COMMIT]]   (default profiles/alleles_step_timing.txt; needs an MI355X)
       python tools/alleles_timing.py --rehearse            (tiny shapes, host form only, no device: checks the script)"""
import ctypes as C
import os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hipstr_amd import capi

REHEARSE = "--rehearse" in sys.argv
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
SHAPES = [("north", dict(n_loci=1000, reads_per_locus=100, n_str_alleles=32, read_len=150, flank_len=55, str_bp=40), 4),
          ("wide", dict(n_loci=64, reads_per_locus=100, n_str_alleles=500, read_len=150, flank_len=35, str_bp=500, own=True), 500)]
if REHEARSE:
    SHAPES = [("north", dict(n_loci=5, reads_per_locus=4, n_str_alleles=6, read_len=60, flank_len=20, str_bp=16), 2),
              ("wide", dict(n_loci=2, reads_per_locus=4, n_str_alleles=12, read_len=60, flank_len=20, str_bp=40, own=True), 12)]
REPS = 3 if REHEARSE else 15
hmm = capi.load_hmm()
capi._alleles_sigs(hmm)
if not REHEARSE:
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
med = lambda v: sorted(v)[len(v) // 2]


class WideBatch:
    """n_str_alleles STR alleles of ONE length (the synthetic generator's alleles differ in copy number, so 500 of them cannot all have 500 bp):
    a period-4 repeat with one base changed at a position of its own per allele; reads of read_len bases down the first haplotype."""

    def __init__(self, n_loci, reads_per_locus, n_str_alleles, read_len, flank_len, str_bp, seed):
        rng = np.random.default_rng(seed); b = capi.Batch()
        for l in range(n_loci):
            motif = "".join(rng.choice(list("ACGT"), 4)); ref = (motif * (str_bp // 4 + 1))[:str_bp]
            opts = [ref]
            for i in range(1, n_str_alleles):
                at = (i * 7919) % str_bp
                opts.append(ref[:at] + ("A" if ref[at] != "A" else "C") + ref[at + 1:])
            assert len(set(opts)) == len(opts)
            fl = ["".join(rng.choice(list("ACGT"), flank_len)) for _ in range(2)]
            hap = fl[0] + ref + fl[1]
            reads = [dict(seq=hap[:read_len], qual="F" * read_len, start=10000, cigar=[("=", read_len)]) for _ in range(reads_per_locus)]
            b.add_locus([(10000, 10000 + flank_len, [fl[0]]), (10000 + flank_len, 10000 + flank_len + str_bp, opts),
                         (10000 + flank_len + str_bp, 10000 + 2 * flank_len + str_bp, [fl[1]])], 4, [0.9, 0.05, 0.05, 0.7, 0.005, 0.005], reads)
        self.b = b.finalize(); self.ptr = C.pointer(self.b.struct)

    def close(self):
        pass


def census_of(sb, n_add, own):
    """every locus: n_add candidates in orderByLengthAndSequence order, all options called and spanned"""
    b = sb.ptr.contents; nl = int(b.n_loci)
    nopts = np.ctypeslib.as_array(b.blk_nopts, shape=(3 * nl,)).reshape(nl, 3)
    opt_off = np.ctypeslib.as_array(b.opt_off, shape=(int(nopts.sum()) + 1,))
    seq = C.string_at(b.seq, int(opt_off[-1]))
    cand = []; o = 0
    for l in range(nl):
        o1 = o + int(nopts[l][0])
        opts = [seq[opt_off[o1 + i]:opt_off[o1 + i + 1]] for i in range(int(nopts[l][1]))]
        tail = b"" if own else b"ACGTT"                               # (own: same length, one base changed to N; else a tail no option has)
        swap = lambda s, i: s[:(i * 7919 + 3) % len(s)] + b"N" + s[(i * 7919 + 3) % len(s) + 1:]
        new = sorted({(swap(opts[i % len(opts)], i) if own else opts[i % len(opts)]) + tail + b"G" * (i // len(opts)) for i in range(n_add)} - set(opts),
                     key=lambda s: (len(s), s))
        assert len(new) == n_add
        cand.append(new); o += int(nopts[l].sum())
    flat = [s for L in cand for s in L]
    k = dict(cand_off=np.concatenate([[0], np.cumsum([len(L) for L in cand])]).astype(np.int32),
             cand_seq_off=np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int32), cand_seq=b"".join(flat) + b"\0",
             new_n_haps=(nopts[:, 0].astype(np.int64) * (nopts[:, 1] + n_add) * nopts[:, 2]), called=np.ones(int(nopts.sum()), np.uint8),
             spanned=np.ones(int(nopts.sum()), np.uint8))
    cen = capi.HipstrCensusOut()
    cen.cand_off = k["cand_off"].ctypes.data_as(capi._i32p); cen.cand_seq_off = k["cand_seq_off"].ctypes.data_as(capi._i32p); cen.cand_seq = k["cand_seq"]
    cen.new_n_haps = k["new_n_haps"].ctypes.data_as(C.POINTER(C.c_int64)); cen.called = k["called"].ctypes.data_as(capi._u8p); cen.spanned = k["spanned"].ctypes.data_as(capi._u8p)
    hap_bytes = int(opt_off[-1])
    return cen, k, nopts, hap_bytes


def step(sb, cen, nl, flags, free=True):
    phase = np.zeros(nl, np.int32); o = [np.zeros(nl, np.int32) for _ in range(4)]
    so = capi.HipstrAllelesStepOut(*[x.ctypes.data_as(capi._i32p) for x in o], 0)
    t0 = time.perf_counter()
    h = hmm.hipstr_alleles_step(sb.ptr, C.byref(cen), phase.ctypes.data_as(capi._i32p), 0, flags, C.byref(so))
    assert h, hmm.hipstr_last_error()
    if free:
        hmm.hipstr_alleles_free(h); h = None
    dt = time.perf_counter() - t0
    assert so.any_added == 1 and (phase == 0).all()
    return dt, h


def last_timing():
    t = (C.c_double * 4)(); assert hmm.hipstr_debug_alleles_last_timing(t) == 0
    return [float(x) for x in t]


lines = []
verdict = []
for name, kw, n_add in SHAPES:
    kw = dict(kw); own = kw.pop("own", False)
    sb = WideBatch(seed=777, **kw) if own else capi.SynthBatch(seed=777, **kw)
    nl = kw["n_loci"]
    cen, keep, nopts, opt_bytes = census_of(sb, n_add, own)
    A0 = int((nopts[:, 0] * nopts[:, 1] * nopts[:, 2]).max()); A1 = int((nopts[:, 0] * (nopts[:, 1] + n_add) * nopts[:, 2]).max())
    forms = [("host", capi.ALLELES_ON_HOST)] + ([] if REHEARSE else [("device", 0)])
    t = {f: [] for f, _ in forms}
    for f, fl in forms:
        step(sb, cen, nl, fl)                                          # warm-up: code objects, the caches' blocks
    for rep in range(REPS):                                            # alternating
        for f, fl in forms:
            t[f].append(step(sb, cen, nl, fl)[0])
    lines.append("shape %s: %d loci, A = %d -> %d, %d options' bytes before the step, %d candidates per locus" % (name, nl, A0, A1, opt_bytes, n_add))
    for f, _ in forms:
        lines.append("  hipstr_alleles_step %-6s wall time: median %.3f ms of %d calls (fastest %.3f ms, slowest %.3f ms)" %
                     (f, med(t[f]) * 1e3, REPS, min(t[f]) * 1e3, max(t[f]) * 1e3))
    if not REHEARSE:
        os.environ["HIPSTR_ALLELES_TIMING"] = "1"
        km = []
        for rep in range(5):
            step(sb, cen, nl, 0); tm = last_timing(); km.append(tm[0])
        del os.environ["HIPSTR_ALLELES_TIMING"]
        last = capi.alleles_last(hmm)
        lines.append("  device form: kernel %.3f ms (median of 5, HIP events), %.0f bytes up, %.0f bytes home, %d loci on the device, %d by the host code" %
                     (med(km), tm[1], tm[2], last["device_loci"], last["host_loci"]))
        lines.append("  host form: 0 bytes up, 0 bytes home")
        # the forward round the step prepares: only the new haplotypes are aligned
        _, h = step(sb, cen, nl, 0, free=False)
        dev = hmm.hipstr_hmm_upload(hmm.hipstr_alleles_batch(h)); assert dev, hmm.hipstr_last_error()
        ms_total, ms_kernel = C.c_float(0), C.c_float(0)
        assert hmm.hipstr_hmm_align_timed(dev, 5, C.byref(ms_total), C.byref(ms_kernel)) == 0, hmm.hipstr_last_error()
        hmm.hipstr_hmm_free(dev); hmm.hipstr_alleles_free(h)
        lines.append("  forward round at this shape (%d pooled reads per locus x the added haplotypes): kernels %.3f ms per pass (hipstr_hmm_align_timed, 5 passes)" %
                     (kw["reads_per_locus"], ms_kernel.value / 5))
        verdict.append(med(t["host"]) < med(t["device"]))
    sb.close()
if not REHEARSE:
    lines.append("flags = 0: %s (the device form unless the host form is faster at both shapes)" % ("host form" if all(verdict) else "device form"))
try:
    commit = ARGS[1] if len(ARGS) > 1 else subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
except Exception:
    commit = "unknown"
head = ["hipstr_alleles_step, host form beside device form (tools/alleles_timing.py)", "commit: %s" % commit]
text = "\n".join(head + lines) + "\n"
print(text)
if not REHEARSE:
    OUT = ARGS[0] if ARGS else os.path.join(ROOT, "profiles", "alleles_step_timing.txt")
    open(OUT, "w").write(text)
