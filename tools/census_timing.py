"""One hipstr_post_census call at 1000 loci x 500 reads x 32 alleles on a resident read x haplotype matrix, beside hipstr_rm_fetch of the same
matrix — the copy home that was the only way to the spanned marks before, and that this call makes unnecessary.  Trace fields are synthetic
(a locus' reads share 40 requests; most span the repeat, a third of the requests carry stutter, their STR sequences are the block's longest
option with a repeat unit added or its shortest with one removed, so that several requests of a locus have one content and none is an option).
Usage: python tools/census_timing.py [OUT.txt [COMMIT]]   (default profiles/census_timing.txt; needs an MI355X)."""
import os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hipstr_amd import capi

NL, P, S, A_STR, NREQ = 1000, 500, 5, 32, 40
hmm = capi.load_hmm()
assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
sb = capi.SynthBatch(n_loci=NL, reads_per_locus=P, n_str_alleles=A_STR, seed=4242)
b = sb.ptr.contents
A = np.diff(np.ctypeslib.as_array(b.hap_off, shape=(NL + 1,))).astype(np.int32)
nopts = np.ctypeslib.as_array(b.blk_nopts, shape=(3 * NL,)).reshape(NL, 3)
opt_off = np.ctypeslib.as_array(b.opt_off, shape=(int(nopts.sum()) + 1,))
seq = b.seq
bs = np.ctypeslib.as_array(b.blk_start, shape=(3 * NL,)).reshape(NL, 3)[:, 1]; be = np.ctypeslib.as_array(b.blk_end, shape=(3 * NL,)).reshape(NL, 3)[:, 1]
period = np.ctypeslib.as_array(b.period, shape=(NL,))
n = NL * P
rng = np.random.default_rng(1)
read_off = np.arange(NL + 1, dtype=np.int32) * P
lab = np.tile(np.repeat(np.arange(S), P // S), NL)
# the resident matrix: every read favours one of two haplotypes of its sample
ll = -20 - 10 * rng.random(int((A.astype(np.int64) * P).sum()))
pos = np.concatenate([[0], np.cumsum(A.astype(np.int64) * P)])
for l in range(NL):
    M = ll[pos[l]:pos[l + 1]].reshape(P, A[l])
    pair = rng.integers(0, A[l], (S, 2))
    M[np.arange(P), pair[lab[:P], rng.integers(0, 2, P)]] = -1 - rng.random(P)
seeds = np.where(rng.random(n) < 0.05, -1, 7).astype(np.int32)
rm = capi.ReadMatrix(hmm, A, read_off, np.tile(np.arange(P), NL), init_ll=ll, init_seeds=seeds)
pb = capi.PostBatch(A, np.full(NL, S, np.int32), read_off, lab, -rng.random(n), -rng.random(n), np.ones(n, np.int32), None)
pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error()
assert hmm.hipstr_post_launch(pd, None) == 0


def gray_h2a(no):
    out = [[], [], []]
    for i in range(int(no[0]) * int(no[1]) * int(no[2])):
        q = i
        for k in range(3):
            d = q % no[k]; q //= no[k]
            out[k].append(int(no[k] - 1 - d if q % 2 else d))
    return out


h2a = [[], [], []]; strs = []; start = []; stop = []; stut = []; o = 0
for l in range(NL):
    g = gray_h2a(nopts[l])
    for k in range(3):
        h2a[k] += g[k]
    o1 = o + int(nopts[l][0]); unit = seq[opt_off[o1]:opt_off[o1] + int(period[l])]
    opts = [seq[opt_off[o1 + i]:opt_off[o1 + i + 1]] for i in range(int(nopts[l][1]))]
    longest = max(opts, key=len); shortest = min(opts, key=len)
    for q in range(NREQ):
        st = int(rng.choice([0, 0, 0, 0, -1, 1])) * int(period[l])
        strs.append(longest + unit if st > 0 else (shortest[:st] if st < 0 else opts[q % len(opts)])); stut.append(st)
        spans = rng.random() < 0.9
        start.append(int(bs[l]) - (10 if spans else 0)); stop.append(int(be[l]) + 10)
    o += int(nopts[l].sum())
req_read = (np.repeat(np.arange(NL), NREQ) * P + np.tile(np.arange(NREQ), NL)).astype(np.int32)
read_req = (np.repeat(np.arange(NL), P) * NREQ + rng.integers(0, NREQ, n)).astype(np.int32)
read_req[seeds < 0] = -1
trace = capi.census_trace(start, stop, stut, strs)
h2a = [np.array(x, np.int32) for x in h2a]


def census():
    return capi.run_census(hmm, pd, sb.ptr, seeds, read_req, req_read, trace, hap_to_allele=h2a, n_samp=NL * S)


med = lambda v: sorted(v)[len(v) // 2]
t_c = []
for rep in range(9):
    t0 = time.perf_counter(); out = census(); t_c.append(time.perf_counter() - t0)
assert out["rc"] == 0
t_f = []
for rep in range(5):
    t0 = time.perf_counter(); m, _ = rm.fetch(); t_f.append(time.perf_counter() - t0)
assert np.array_equal(m.view(np.uint64), ll.view(np.uint64))
hmm.hipstr_post_free(pd); rm.close()
try:
    import ctypes as C
    hip = C.CDLL("libamdhip64.so"); name = C.create_string_buffer(256)
    assert hip.hipDeviceGetName(name, 256, 0) == 0
    device = name.value.decode() or "gfx950 device (the runtime reports no marketing name; the library holds gfx950 code only)"
except Exception as e:
    device = "unknown (%s)" % type(e).__name__
commit = sys.argv[2] if len(sys.argv) > 2 else None
if commit is None:
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
lines = ["hipstr_post_census beside hipstr_rm_fetch of the same resident matrix (tools/census_timing.py)",
         "commit: %s" % commit, "device: %s" % device,
         "shape: %d loci x %d reads x %d alleles (A = %d..%d), %d samples per locus, %d requests per locus, matrix %.1f MB" %
         (NL, P, A_STR, A.min(), A.max(), S, NREQ, ll.nbytes / 1e6),
         "found: %d candidates, %d spanning reads, %d of them with stutter, %d called and %d spanned marks" %
         (int(out["cand_off"][-1]), int(out["n_spanning"].sum()), int(out["n_span_stutter"].sum()), int((out["called"] == 1).sum()), int((out["spanned"] == 1).sum())),
         "hipstr_post_census wall time: median %.3f ms of 9 calls (first %.3f ms, fastest %.3f ms; the Python wrapper's marshalling included)" %
         (med(t_c) * 1e3, t_c[0] * 1e3, min(t_c) * 1e3),
         "hipstr_rm_fetch    wall time: median %.3f ms of 5 calls (fastest %.3f ms; into a fresh numpy array)" % (med(t_f) * 1e3, min(t_f) * 1e3)]
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "census_timing.txt")
open(OUT, "w").write("\n".join(lines) + "\n")
print("\n".join(lines))
