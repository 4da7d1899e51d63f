"""Traceback throughput: hipstr_hmm_trace with one request per read (its source allele) on NS-shaped loci — per-locus calls and
one call for all loci — with the compiled reference's trace_optimal_aln (1 thread) beside it when oracle/_ref is present.
--assemble host|device: the host replay (hipstr_hmm_trace) or the records assembled on the device (hipstr_hmm_trace_ex with
HIPSTR_TRACE_ASSEMBLE_DEVICE).  --repeats N: N timed calls after the warm-up; "call_ms" / "locus_100_ms" are their medians with the
fastest and the slowest beside them (the whole request list, and the first 100 requests of locus 0 as a call of its own).
Prints one JSON line."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from hipstr_amd import capi, shard
import util

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("n_loci", nargs="?", type=int, default=64)
ap.add_argument("--assemble", choices=("host", "device"), default="host")
ap.add_argument("--repeats", type=int, default=1)
args = ap.parse_args()
n_loci = args.n_loci
FLAGS = dict(flags=capi.TRACE_ASSEMBLE_DEVICE) if args.assemble == "device" else {}     # host: hipstr_hmm_trace itself
hmm = capi.load_hmm(); ora = capi.load_oracle()
assert hmm.hipstr_hmm_init(0) == 0
sb = capi.SynthBatch(n_loci=n_loci, reads_per_locus=500, n_str_alleles=32, seed=1000)
seeds = np.zeros(sb.n_reads, np.int32)
hmm.hipstr_calc_seed_bases(sb.ptr, seeds.ctypes.data_as(capi._i32p))
src = sb.src_allele()
rr = [r for r in range(sb.n_reads) if seeds[r] >= 0]; aa = [int(src[r]) for r in rr]
whole = util.synth_to_batch(sb); a = whole.arrays
h2r = []
ones = []
for l in range(n_loci):
    one = shard.batch_from_arrays(shard.subset_arrays(a, l, l + 1)); ones.append(one)
    h2r += util.synthetic_hap_to_ref(ora, one.ptr)
cap = 1 << 26
capi.run_trace(hmm, "hipstr_hmm_", whole.ptr, rr[:500], aa[:500], h2r, cap=cap, unpack=False, **FLAGS)     # warm-up
tb = {}
capi.run_trace(hmm, "hipstr_hmm_", whole.ptr, rr, aa, h2r, cap=cap, timing=tb, unpack=False, **FLAGS)
def spread(xs):
    return dict(median=float(np.median(xs)), min=min(xs), max=max(xs), n=len(xs))
extra = {}
if args.repeats > 1:
    ts = []
    for _ in range(args.repeats):
        t = {}; capi.run_trace(hmm, "hipstr_hmm_", whole.ptr, rr, aa, h2r, cap=cap, timing=t, unpack=False, **FLAGS); ts.append(1e3 * t["call_s"])
    extra["call_ms"] = spread(ts)
    r1 = int(a["read_off"][1]); sel = [i for i, r in enumerate(rr) if r < r1][:100]
    h0 = h2r[:int(a["hap_off"][1])]; ts = []
    for i in range(args.repeats + 1):
        t = {}; capi.run_trace(hmm, "hipstr_hmm_", ones[0].ptr, [rr[j] for j in sel], [aa[j] for j in sel], h0, cap=1 << 22, timing=t, unpack=False, **FLAGS)
        if i: ts.append(1e3 * t["call_s"])
    extra["locus_100_ms"] = spread(ts); extra["locus_100_requests"] = len(sel)
out = dict(assemble=args.assemble, host_threads=os.environ.get("HIPSTR_HOST_THREADS"), **extra)
out.update(metric="tracebacks_per_sec", value=len(rr) / tb["call_s"], loci=n_loci, requests=len(rr), ms_per_locus=1e3 * tb["call_s"] / n_loci,
           note="one C call for all loci, end to end: host prep + H2D + kernels + D2H + replay/stitch (host threads or device)")
# the same requests, one call per locus (what a per-locus caller sees)
tl = {}; n1 = 0
for l in range(min(n_loci, 8)):
    r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1])
    sel = [i for i, r in enumerate(rr) if r0 <= r < r1]
    capi.run_trace(hmm, "hipstr_hmm_", ones[l].ptr, [rr[i] - r0 for i in sel], [aa[i] for i in sel], h2r[int(a["hap_off"][l]):int(a["hap_off"][l + 1])],
                   cap=1 << 22, timing=tl, unpack=False, **FLAGS)
    n1 += len(sel)
out["per_locus_calls"] = n1 / tl["call_s"]
if os.path.exists(capi.REF_LIB):
    ref = capi.load_ref(); tr_ = {}
    r0, r1 = int(a["read_off"][0]), int(a["read_off"][1])
    sel = [i for i, r in enumerate(rr) if r0 <= r < r1][:200]
    capi.run_trace(ref, "ref_", ones[0].ptr, [rr[i] - r0 for i in sel], [aa[i] for i in sel], cap=1 << 22, timing=tr_, unpack=False)
    out["cpu_reference_1thread"] = len(sel) / tr_["call_s"]
print(json.dumps(out))
