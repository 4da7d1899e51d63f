"""The handle calls every genotype() round goes through, timed with a given build of libhipstr_hmm.so, to set two builds side by side
(profiles/handles_ab.txt: parent / branch / parent): hipstr_post_run on one locus (the small, staged form) and on 64 haplotypes x 128
samples (a block per array), hipstr_post_extract on the north-star shape of tests/test_genotypes_gpu.py, one round of a read matrix
(scatter, remap, fetch of the seeds, remap back) and hipstr_hmm_process_reads on one locus.  One line per measurement: label, name,
median and 10th percentile in microseconds per call through the ctypes wrapper, calls.
A measurement, not a test.  Usage: python tools/handles_timing.py LIBRARY LABEL  (needs an MI355X)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from hipstr_amd import capi

capi.HMM_LIB = os.path.abspath(sys.argv[1]); label = sys.argv[2]
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
import test_readmat_gpu as trm
import test_cache_balance_gpu as tcb


def measure(name, fn, n, warm=20):
    for _ in range(warm):
        fn()
    t = np.empty(n)
    for i in range(n):
        t0 = time.perf_counter(); fn(); t[i] = time.perf_counter() - t0
    print("%-8s %-34s median %10.1f us   p10 %10.1f us   calls %d" % (label, name, np.median(t) * 1e6, np.percentile(t, 10) * 1e6, n), flush=True)


def post_run_of(pb):
    k, ptrs = tcb.post_results(pb)
    def f():
        assert hmm.hipstr_post_run(pb.ptr, None, *ptrs) == 0
    return f


rng = np.random.default_rng(1)
one = capi.PostBatch([8], [4], [0, 24], np.repeat(np.arange(4), 6), -rng.random(24), -rng.random(24), np.ones(24, np.int32), -40 * rng.random(24 * 8))
measure("post_run one locus (small form)", post_run_of(one), 3000, warm=200)
measure("post_run 64 hap x 128 samples", post_run_of(tcb.large_pb()), 300)

# hipstr_post_extract on the north-star shape of tests/test_genotypes_gpu.py, every output on
rng = np.random.default_rng(11)
nl, A, S, V = 3, 32, 100, 8
R = S * 6; n = nl * R
pb = capi.PostBatch(n_alleles=[A] * nl, n_samples=[S] * nl, read_off=np.arange(nl + 1) * R, sample_label=np.tile(np.repeat(np.arange(S), 6), nl),
                    log_p1=-rng.random(n), log_p2=-rng.random(n), read_weight=np.ones(n, np.int32), log_aln_probs=-rng.random(n * A) * 40, haploid=[0, 1, 0])
h2a = np.ascontiguousarray(np.tile((np.arange(A) // 2) % V, nl), np.int32); nv = np.full(nl, V, np.int32)
rq = capi.HipstrGtRequest(nv.ctypes.data_as(capi._i32p), h2a.ctypes.data_as(capi._i32p), 1, 1, 1)
NS = nl * S
k = dict(best_hap=np.zeros(2 * NS, np.int32), best_gt=np.zeros(2 * NS, np.int32), gls=np.zeros(NS * V * V), pls=np.zeros(NS * V * V, np.int32), phased_gls=np.zeros(NS * V * V))
for nm in ("log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff"):
    k[nm] = np.zeros(NS)
o = capi.HipstrGtOut(*[k[f].ctypes.data_as(t) for f, t in capi.HipstrGtOut._fields_])
hmm.hipstr_post_extract.restype = C.c_int; hmm.hipstr_post_extract.argtypes = [C.c_void_p, C.POINTER(capi.HipstrGtRequest), C.POINTER(capi.HipstrGtOut)]
pd = hmm.hipstr_post_upload(pb.ptr, None); assert pd
assert hmm.hipstr_post_launch(pd, None) == 0
def extract():
    assert hmm.hipstr_post_extract(pd, C.byref(rq), C.byref(o)) == 0
measure("post_extract north-star shape", extract, 1000, warm=50)
hmm.hipstr_post_free(pd)

# one round of the read matrix: scatter, remap, fetch of the seeds (the second remap restores the first shape)
small = trm.pooled_batch(trm.SHAPES1[1:3], [5, 2], [None, None])
dev = trm.upload_and_align(hmm, small)
rm = capi.ReadMatrix(hmm, [3, 4], [0, 7, 9], [0, 1, 2, 3, 4, 4, 0, 0, 1], [0, 1, 0, 0, 0, 1, 0, 0, 1])
seeds = np.zeros(9, np.int32)
up = (np.array([5, 4], np.int32), np.array([4, 0, 2, 0, 1, 2, 3], np.int32)); down = (np.array([3, 4], np.int32), np.array([1, -1, 2, -1, 0, 0, 1, 2, 3], np.int32))
def rm_round():
    assert hmm.hipstr_rm_scatter(rm.h, dev, None) == 0
    assert hmm.hipstr_rm_remap(rm.h, up[0].ctypes.data_as(capi._i32p), up[1].ctypes.data_as(capi._i32p)) == 0
    assert hmm.hipstr_rm_fetch(rm.h, None, seeds.ctypes.data_as(capi._i32p)) == 0
    assert hmm.hipstr_rm_remap(rm.h, down[0].ctypes.data_as(capi._i32p), down[1].ctypes.data_as(capi._i32p)) == 0
measure("read matrix: scatter remap fetch remap", rm_round, 1000, warm=50)
rm.close(); hmm.hipstr_hmm_free(dev)

sb = capi.SynthBatch(n_loci=1, reads_per_locus=50, n_str_alleles=4, seed=1)
n_reads, n_out, _ = capi.batch_dims(sb.ptr)
probs = np.zeros(n_out); sd = np.zeros(n_reads, np.int32)
def pr():
    assert hmm.hipstr_hmm_process_reads(sb.ptr, probs.ctypes.data_as(capi._f64p), sd.ctypes.data_as(capi._i32p)) == 0
measure("process_reads one locus", pr, 2000, warm=100)
