"""The two steps of SeqStutterGenotyper::genotype() that read traceback records, each both ways on one device in one process, at
bench_trace.py's shape (32 loci x 500 reads x 32 alleles: about 16 k requests) on a resident read x haplotype matrix:
  between two rounds   (a) hipstr_hmm_trace_ex(DEVICE) + hipstr_post_census            (b) hipstr_hmm_trace_resident + hipstr_post_census_dev + free
  for a VCF record     (a) hipstr_hmm_trace_ex(DEVICE) + hipstr_assign_trace_stats     (b) hipstr_hmm_trace_resident + hipstr_assign_trace_stats_dev
                                                                                           + hipstr_trace_dev_fetch(FLANKS) + free
Only the C calls are timed (every buffer is allocated before): one warm-up, then 9 calls, the median with the fastest and the slowest beside
it, at HIPSTR_HOST_THREADS 2 and 16 (a fresh child process each: the library reads the variable once).  The bytes either path moves over
PCIe are computed from hipstr_trace_dev_sizes and the array sizes.
Usage: python tools/trace_resident_timing.py [OUT.txt [COMMIT]]   (default profiles/trace_resident_timing.txt; needs an MI355X)."""
import ctypes as C
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hipstr_amd import capi

NL, P, S, A_STR, REPS = 32, 500, 5, 32, 9
THREADS = (2, 16)


def gray_h2a(no):
    out = [[], [], []]
    for i in range(int(no[0]) * int(no[1]) * int(no[2])):
        q = i
        for k in range(3):
            d = q % no[k]; q //= no[k]
            out[k].append(int(no[k] - 1 - d if q % 2 else d))
    return out


def child():
    hmm = capi.load_hmm()
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
    capi._trace_dev_sigs(hmm)
    sb = capi.SynthBatch(n_loci=NL, reads_per_locus=P, n_str_alleles=A_STR, seed=1000)
    b = sb.ptr.contents
    A = np.diff(np.ctypeslib.as_array(b.hap_off, shape=(NL + 1,))).astype(np.int32)
    nopts = np.ctypeslib.as_array(b.blk_nopts, shape=(3 * NL,)).reshape(NL, 3)
    bs = np.ctypeslib.as_array(b.blk_start, shape=(3 * NL,)).reshape(NL, 3)[:, 1]; be = np.ctypeslib.as_array(b.blk_end, shape=(3 * NL,)).reshape(NL, 3)[:, 1]
    n = NL * P; ns = NL * S
    rng = np.random.default_rng(1)
    read_off = np.arange(NL + 1, dtype=np.int32) * P
    lab = np.tile(np.repeat(np.arange(S), P // S), NL)
    pool = np.tile(np.arange(P), NL).astype(np.int32)                # every read its own pool: the batch is the pooled batch
    # forward pass -> resident matrix -> posteriors -> the request list of retrace_alignments
    dev = hmm.hipstr_hmm_upload(sb.ptr); assert dev, hmm.hipstr_last_error()
    assert hmm.hipstr_hmm_align(dev, None) == 0
    rm = capi.ReadMatrix(hmm, A, read_off, pool); rm.scatter(dev)
    pb = capi.PostBatch(A, np.full(NL, S, np.int32), read_off, lab, -rng.random(n), -rng.random(n), np.ones(n, np.int32), None)
    pd = hmm.hipstr_post_upload(pb.ptr, rm.dev_ll); assert pd, hmm.hipstr_last_error()
    assert hmm.hipstr_post_launch(pd, None) == 0
    _, seeds = rm.fetch(); seeds = np.ascontiguousarray(seeds, np.int32)
    asg = capi.run_assign(hmm, pd, seeds, pool_index=pool, pool_off=read_off, rule=capi.ASSIGN_RETRACE, n_reads=n, n_samp=ns)
    assert asg["rc"] == 0
    nq = asg["n_req"]
    rr = np.ascontiguousarray(asg["req_read"], np.int32); aa = np.ascontiguousarray(asg["req_allele"], np.int32)
    read_req = np.ascontiguousarray(asg["read_req"], np.int32); best = np.ascontiguousarray(asg["best_hap"], np.int32)
    h2r_list = capi.hap_aln_info(hmm, "hipstr_", sb.ptr)
    h2r = (C.c_char_p * len(h2r_list))(*h2r_list)
    h2a = [[], [], []]
    for l in range(NL):
        g = gray_h2a(nopts[l])
        for k in range(3):
            h2a[k] += g[k]
    h2a = [np.array(x, np.int32) for x in h2a]
    n_opts = int(nopts.sum())
    i32p = capi._i32p; p = lambda x: x.ctypes.data_as(i32p)

    # ---- buffers, once: sized by a first resident call
    td = capi.run_trace_resident(hmm, sb.ptr, rr, aa, h2r_list)
    _, tot = td.sizes(); td.close()
    room = int(tot.max())
    o = capi.HipstrTraceOut(); keep = {}
    for arrays in capi.TRACE_GROUPS.values():
        for nm, kind, pl in arrays:
            if kind == "chr":
                keep[nm] = C.create_string_buffer(room); setattr(o, nm, C.cast(keep[nm], C.c_char_p))
            else:
                m = {"f8": nq, "i4": nq, "off": (2 * nq if pl == 2 else nq) + 1, "i4p": room}[kind]
                keep[nm] = np.zeros(m, np.float64 if kind == "f8" else np.int32)
                setattr(o, nm, keep[nm].ctypes.data_as(capi._f64p if kind == "f8" else i32p))
    o.cap_chars = room
    rq = capi.HipstrCensusRequest(C.cast(sb.ptr, C.POINTER(capi.HipstrBatch)), p(seeds), p(read_req), nq, p(rr), None,
                                  (i32p * 3)(*[p(x) for x in h2a]), None, 0, 0.01)
    ck = dict(cand_off=np.zeros(NL + 1, np.int32), cand_req=np.zeros(nq, np.int32), cand_seq_off=np.zeros(nq + 1, np.int32), new_n_haps=np.zeros(NL, np.int64),
              n_spanning=np.zeros(ns, np.int32), n_span_stutter=np.zeros(ns, np.int32), called=np.zeros(n_opts, np.uint8), spanned=np.zeros(n_opts, np.uint8))
    cseq = C.create_string_buffer(max(int(tot[1]), 1))
    co = capi.HipstrCensusOut(p(ck["cand_off"]), p(ck["cand_req"]), p(ck["cand_seq_off"]), C.cast(cseq, C.c_char_p), ck["new_n_haps"].ctypes.data_as(C.POINTER(C.c_int64)),
                              p(ck["n_spanning"]), p(ck["n_span_stutter"]), ck["called"].ctypes.data_as(capi._u8p), ck["spanned"].ctypes.data_as(capi._u8p), nq, int(tot[1]))
    capi._sig(hmm.hipstr_post_census, C.c_int, [C.c_void_p, C.POINTER(capi.HipstrCensusRequest), C.POINTER(capi.HipstrCensusOut)])
    capi._sig(hmm.hipstr_post_census_dev, C.c_int, [C.c_void_p, C.POINTER(capi.HipstrCensusRequest), C.c_void_p, C.POINTER(capi.HipstrCensusOut)])
    capi._sig(hmm.hipstr_hmm_trace_ex, C.c_int, [capi._BP, C.c_int32, i32p, i32p, i32p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(capi.HipstrTraceOut)])
    capi._sig(hmm.hipstr_assign_trace_stats, C.c_int, [capi._PBP, i32p, C.POINTER(capi.HipstrTraceOut)] + [i32p] * 9)
    st_h2a = np.concatenate([np.arange(a) for a in A]).astype(np.int32); st_bp = np.concatenate([3 * np.arange(a) - 3 for a in A]).astype(np.int32)
    st_v = A.copy(); st_start = np.ascontiguousarray(bs, np.int32); st_stop = np.ascontiguousarray(be, np.int32)
    res = [[np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(n, np.int32)] for _ in range(2)]
    why = lambda: hmm.hipstr_last_error().decode()

    def trace_ex():
        assert hmm.hipstr_hmm_trace_ex(sb.ptr, nq, p(rr), p(aa), None, h2r, capi.TRACE_ASSEMBLE_DEVICE, C.byref(o)) == 0, why()

    def trace_res():
        h = C.c_void_p()
        assert hmm.hipstr_hmm_trace_resident(sb.ptr, nq, p(rr), p(aa), None, h2r, 0, C.byref(h)) == 0, why()
        return h

    def round_a():
        trace_ex(); rq.trace = C.pointer(o)
        assert hmm.hipstr_post_census(pd, C.byref(rq), C.byref(co)) == 0, why()

    def round_b():
        h = trace_res(); rq.trace = None
        assert hmm.hipstr_post_census_dev(pd, C.byref(rq), h, C.byref(co)) == 0, why()
        hmm.hipstr_trace_dev_free(h)

    def record_a():
        trace_ex()
        assert hmm.hipstr_assign_trace_stats(pb.ptr, p(read_req), C.byref(o), p(best), p(st_h2a), p(st_bp), p(st_v), p(st_start), p(st_stop), *[p(x) for x in res[0]]) == 0, why()

    def record_b():
        h = trace_res()
        assert hmm.hipstr_assign_trace_stats_dev(pb.ptr, p(read_req), h, p(best), p(st_h2a), p(st_bp), p(st_v), p(st_start), p(st_stop), *[p(x) for x in res[1]]) == 0, why()
        assert hmm.hipstr_trace_dev_fetch(h, capi.TRACE_F_FLANKS, C.byref(o)) == 0, why()
        hmm.hipstr_trace_dev_free(h)

    def timed(fn):
        fn()                                                          # warm-up
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
        return dict(median=float(np.median(ts)), min=min(ts), max=max(ts))

    out = dict(host_threads=os.environ.get("HIPSTR_HOST_THREADS"), requests=int(nq), reads=int(n))
    # the two paths give the same answers: checked once before anything is timed
    round_a(); want = {k: v.copy() for k, v in ck.items()}; want_seq = cseq.raw
    round_b()
    assert all(np.array_equal(ck[k], want[k]) for k in ck) and cseq.raw[:int(ck["cand_seq_off"][ck["cand_off"][-1]])] == want_seq[:int(want["cand_seq_off"][want["cand_off"][-1]])]
    record_a(); record_b()
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1]))
    out["candidates"] = int(ck["cand_off"][-1]); out["spanning_reads"] = int(ck["n_spanning"].sum())
    for name, fn in (("round_a", round_a), ("round_b", round_b), ("record_a", record_a), ("record_b", record_b)):
        out[name] = timed(fn)
    # ---- bytes over PCIe, from the sizes (arrays of hipstr_trace_out_t: 8 + 6 x 4 bytes per request, the seven offset arrays, the ten pools)
    chunks = len(capi.trace_plan(hmm, sb.ptr, rr, aa)["chunks"])
    esz = dict(zip(range(7), (1, 1, 1, 8, 5, 5, 1)))                  # bytes per element of a pool: indel 4+4, snp 4+1, cigar 1+4
    trace_home = 32 * nq + 4 * (8 * nq + 7) + sum(int(tot[i]) * esz[i] for i in range(7)) + 64 * chunks
    census_up = 4 * (3 * nq + nq + 1) + int(tot[1])
    cand_chars = int(ck["cand_seq_off"][ck["cand_off"][-1]])
    stats_up = 8 * n + 4 * (len(st_h2a) + len(st_bp)) + 16 * ns + 24 * NL          # read_req, best_hap, the tables, a unit per sample, the loci
    out["bytes"] = dict(
        round_a=dict(d2h=trace_home, h2d=census_up), round_b=dict(d2h=64 * chunks + 4 * (nq + 1) + cand_chars, h2d=0),
        record_a=dict(d2h=trace_home, h2d=0), record_b=dict(d2h=64 * chunks + 8 * ns + 4 * n + 4 * (2 * nq + 1) + int(tot[2]), h2d=stats_up),
        note="trace-related traffic only: the request list, the per-read arrays and the census' counts and marks travel the same way on both paths")
    out["totals"] = [int(x) for x in tot]; out["chunks"] = chunks
    hmm.hipstr_post_free(pd); rm.close(); hmm.hipstr_hmm_free(dev)
    print("RESULT " + json.dumps(out))


def main():
    runs = []
    for t in THREADS:
        env = dict(os.environ, HIPSTR_HOST_THREADS=str(t))
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, stdout=subprocess.PIPE).stdout.decode()
        runs.append(json.loads([l for l in txt.splitlines() if l.startswith("RESULT ")][-1][7:]))
    commit = sys.argv[2] if len(sys.argv) > 2 else None
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    r0 = runs[0]
    fmt = lambda d: "%8.3f ms (%.3f .. %.3f)" % (d["median"], d["min"], d["max"])
    lines = ["Traceback records kept on the device for the census and the read counts (tools/trace_resident_timing.py)",
             "commit: %s" % commit,
             "shape: %d loci x %d reads x %d STR alleles on a resident matrix; %d requests of %d reads in %d chunk(s); %d candidates, %d spanning reads" %
             (NL, P, A_STR, r0["requests"], r0["reads"], r0["chunks"], r0["candidates"], r0["spanning_reads"]),
             "wall time of the C calls alone: 1 warm-up, then %d calls: median (fastest .. slowest)" % REPS,
             "  (a) hipstr_hmm_trace_ex(DEVICE) + hipstr_post_census | + hipstr_assign_trace_stats",
             "  (b) hipstr_hmm_trace_resident + hipstr_post_census_dev + free | + hipstr_assign_trace_stats_dev + hipstr_trace_dev_fetch(FLANKS) + free", ""]
    for r in runs:
        lines += ["HIPSTR_HOST_THREADS=%s" % r["host_threads"],
                  "  between rounds  (a) %s   (b) %s   (b)/(a) %.2f" % (fmt(r["round_a"]), fmt(r["round_b"]), r["round_b"]["median"] / r["round_a"]["median"]),
                  "  for a record    (a) %s   (b) %s   (b)/(a) %.2f" % (fmt(r["record_a"]), fmt(r["record_b"]), r["record_b"]["median"] / r["record_a"]["median"])]
    by = r0["bytes"]
    lines += ["", "bytes over PCIe per step (%s):" % by["note"]]
    for k, name in (("round_a", "between rounds (a)"), ("round_b", "between rounds (b)"), ("record_a", "for a record   (a)"), ("record_b", "for a record   (b)")):
        lines.append("  %s  device to host %10d   host to device %10d" % (name, by[k]["d2h"], by[k]["h2d"]))
    lines.append("pool elements (hap_aln, str_seq, flank_seq, indel, snp, cigar, aln_str): %s" % r0["totals"])
    slower = [(r["host_threads"], k) for r in runs for k in ("round", "record") if r[k + "_b"]["median"] >= r[k + "_a"]["median"]]
    lines.append("(b) not faster than (a): %s" % (", ".join("%s at %s threads" % (k, t) for t, k in slower) if slower else "nowhere"))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "trace_resident_timing.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
