"""The hand-over between the forward pass and the posteriors at the north-star shape (1000 loci x 500 pooled reads x 32 haplotypes) with two
reads per pool (1000 reads per locus, every fourth read a second mate), timed two ways on one device:
  host path     hipstr_hmm_fetch of the pooled rows + the scatter and mate sums on the host (numpy, vectorised per batch) + hipstr_post_upload
                of the R x A matrix from host memory — what every round cost before hipstr_rm_*;
  resident path hipstr_rm_scatter + hipstr_post_upload given the matrix' device pointer, until the stream is idle.
A measurement, not a test.  Usage: python tools/readmat_timing.py [OUT.txt]  (default profiles/readmat_timing.txt; needs an MI355X)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipstr_amd import capi

hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
NL, P, A_STR, PER_POOL, S, REPS = 1000, 500, 32, 2, 5, 7
lines = []
def say(s):
    print(s, flush=True); lines.append(s)

sb = capi.SynthBatch(n_loci=NL, reads_per_locus=P, n_str_alleles=A_STR, seed=4242)
A = np.diff(np.ctypeslib.as_array(sb.ptr.contents.hap_off, shape=(NL + 1,))).astype(np.int32)
assert len(set(A.tolist())) == 1
a = int(A[0]); R = P * PER_POOL; n = NL * R
dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev
assert hmm.hipstr_hmm_align(dev, None) == 0
pool_l = np.arange(R, dtype=np.int32) // PER_POOL
mates_l = (np.arange(R) % 4 == 3).astype(np.uint8)
read_off = (np.arange(NL + 1) * R).astype(np.int32)
pool = np.tile(pool_l, NL); mates = np.tile(mates_l, NL)
rng = np.random.default_rng(1)
lab = np.tile(np.repeat(np.arange(S), R // S), NL)
kw = dict(n_alleles=A, n_samples=np.full(NL, S, np.int32), read_off=read_off, sample_label=lab, log_p1=-rng.random(n), log_p2=-rng.random(n),
          read_weight=1 - mates.astype(np.int32))
say("shape: %d loci x %d pooled reads x %d haplotypes, %d reads per pool: pooled rows %.1f MB, read matrix %.1f MB, %d mate pairs"
    % (NL, P, a, PER_POOL, sb.n_out * 8 / 1e6, n * a * 8 / 1e6, int(mates.sum())))

def host_round():
    t0 = time.perf_counter()
    ll = np.zeros(sb.n_out); sd = np.zeros(sb.n_reads, np.int32)
    assert hmm.hipstr_hmm_fetch(dev, ll.ctypes.data_as(capi._f64p), sd.ctypes.data_as(capi._i32p)) == 0
    t1 = time.perf_counter()
    M = ll.reshape(NL, P, a)[:, pool_l, :]                         # seq_stutter_genotyper.cpp:532-543
    second = np.nonzero(mates_l)[0]
    tot = M[:, second - 1, :] + M[:, second, :]                    # :551-564
    M[:, second - 1, :] = tot; M[:, second, :] = tot
    seeds = sd.reshape(NL, P)[:, pool_l].ravel()
    t2 = time.perf_counter()
    pb = capi.PostBatch(log_aln_probs=M.ravel(), **kw)
    pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd
    t3 = time.perf_counter()
    hmm.hipstr_post_free(pd)
    return (t1 - t0, t2 - t1, t3 - t2), M.ravel(), seeds

rm = capi.ReadMatrix(hmm, A, read_off, pool, mates)
pb_dev = capi.PostBatch(log_aln_probs=None, **kw)
def resident_round():
    t0 = time.perf_counter()
    rm.scatter(dev)
    t1 = time.perf_counter()
    pd = hmm.hipstr_post_upload(pb_dev.ptr, rm.dev_ll); assert pd
    assert hmm.hipstr_rm_fetch(rm.h, None, None) == 0              # (copies nothing: waits until the matrix' stream is idle)
    t2 = time.perf_counter()
    hmm.hipstr_post_free(pd)
    return (t1 - t0, t2 - t1)

host = []; res = []
for rep in range(REPS):
    t, M, seeds = host_round(); host.append(t)
for rep in range(REPS):
    res.append(resident_round())
got, gs = rm.fetch()
assert np.array_equal(got.view(np.uint64), M.view(np.uint64)) and np.array_equal(gs, seeds), "the two paths disagree"
med = lambda v: sorted(v)[len(v) // 2]
h = [med([x[i] for x in host]) for i in range(3)]
say("host path     (median of %d): fetch %.1f ms + host scatter %.1f ms + hipstr_post_upload from host memory %.1f ms = %.1f ms"
    % (REPS, 1e3 * h[0], 1e3 * h[1], 1e3 * h[2], 1e3 * med([sum(x) for x in host])))
say("resident path (median of %d): hipstr_rm_scatter queued in %.2f ms, with hipstr_post_upload on the device pointer and the stream idle %.2f ms"
    % (REPS, 1e3 * med([x[0] for x in res]), 1e3 * med([sum(x) for x in res])))
# the scatter kernel alone: queue, then wait
ts = []
for rep in range(REPS):
    assert hmm.hipstr_rm_fetch(rm.h, None, None) == 0
    t0 = time.perf_counter(); rm.scatter(dev); assert hmm.hipstr_rm_fetch(rm.h, None, None) == 0; ts.append(time.perf_counter() - t0)
moved = (sb.n_out + n * a) * 8
say("hipstr_rm_scatter alone, call to idle stream (host checks and staging included): %.2f ms; %.0f MB read + written by the kernel: %.0f GB/s over the whole call"
    % (1e3 * med(ts), moved / 1e6, moved / med(ts) / 1e9))
say("the matrices of the two paths are identical bit for bit")
rm.close(); hmm.hipstr_hmm_free(dev); sb.close()
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "readmat_timing.txt")
open(OUT, "w").write("\n".join(lines) + "\n")
