"""SeqStutterGenotyper::recompute_stutter_models both ways on one device in one process, on one seeded batch (32 loci x 500 reads x 16 STR
alleles, 5 samples per locus, on a resident read x haplotype matrix and a resident traceback result):
  (a) the host chain   hipstr_trace_dev_fetch(SCALARS | STR_SEQ) + hipstr_em_batch_from_traces + hipstr_em_train
  (b) the resident call hipstr_em_train_dev
  (c) hipstr_em_train alone on the batch (a) built: the EM loop's own time (with its host preparation and uploads), part of both
Only the C calls are timed (every buffer is allocated before): one warm-up, then 9 calls, the median with the fastest and the slowest beside
it, at HIPSTR_HOST_THREADS 2 and 16 (a fresh child process each: the library reads the variable once).  The bytes either path moves over
the host link are computed from the array sizes.  No ratio is promised: what is reported is (b) against (a) of the same commit.
Usage: python tools/em_resident_timing.py [OUT.txt [COMMIT]]   (default profiles/em_resident_timing.txt; needs an MI355X)."""
import ctypes as C
import json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hipstr_amd import capi

NL, P, S, A_STR, REPS = 32, 500, 5, 16, 9
THREADS = (2, 16)


def child():
    hmm = capi.load_hmm()
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
    sb = capi.SynthBatch(n_loci=NL, reads_per_locus=P, n_str_alleles=A_STR, seed=1000)
    b = sb.ptr.contents
    A = np.diff(np.ctypeslib.as_array(b.hap_off, shape=(NL + 1,))).astype(np.int32)
    period = np.ctypeslib.as_array(b.period, shape=(NL,)).astype(np.int32)
    n = NL * P; ns = NL * S
    rng = np.random.default_rng(1)
    read_off = np.arange(NL + 1, dtype=np.int32) * P
    lab = np.tile(np.repeat(np.arange(S), P // S), NL)
    pool = np.tile(np.arange(P), NL).astype(np.int32)                # every read its own pool: the batch is the pooled batch
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
    read_req = np.ascontiguousarray(asg["read_req"], np.int32)
    td = capi.run_trace_resident(hmm, sb.ptr, rr, aa, capi.hap_aln_info(hmm, "hipstr_", sb.ptr))
    _, tot = td.sizes()
    i32p, f64p, u8p = capi._i32p, capi._f64p, capi._u8p
    p = lambda x: x.ctypes.data_as(i32p); pf = lambda x: x.ctypes.data_as(f64p)

    # ---- buffers, once
    o = capi.HipstrTraceOut(); keep = {}
    for bit in (capi.TRACE_F_SCALARS, capi.TRACE_F_STR_SEQ):
        for nm, kind, pl in capi.TRACE_GROUPS[bit]:
            if kind == "chr":
                keep[nm] = C.create_string_buffer(max(int(tot[1]), 1)); setattr(o, nm, C.cast(keep[nm], C.c_char_p))
            else:
                keep[nm] = np.zeros(nq + 1, np.float64 if kind == "f8" else np.int32)
                setattr(o, nm, keep[nm].ctypes.data_as(f64p if kind == "f8" else i32p))
    o.cap_chars = max(int(tot[1]), 1)
    rq = capi.HipstrEmTraceRequest(C.cast(sb.ptr, C.POINTER(capi.HipstrBatch)), p(seeds), p(read_req), nq, p(rr), 0, 100, 0.01, 0.001)
    e_off = np.zeros(NL + 1, np.int32); e_lab = np.zeros(n, np.int32); e_bps = np.zeros(n, np.int32); e_p1 = np.zeros(n); e_p2 = np.zeros(n)
    n_samples = np.full(NL, S, np.int32)
    eb = capi.HipstrEmBatch(NL, p(period), None, p(n_samples), p(e_off), p(e_lab), p(e_bps), pf(e_p1), pf(e_p2), 0, 100, 0.01, 0.001)
    res = [[np.zeros(NL, np.uint8), np.zeros(6 * NL), np.zeros(NL, np.int32), np.zeros(NL)] for _ in range(2)]
    d_off = np.zeros(NL + 1, np.int32); d_ns = np.zeros(NL, np.int32)
    outs = lambda r: (r[0].ctypes.data_as(u8p), pf(r[1]), p(r[2]), pf(r[3]))
    eo = capi.HipstrEmTraceOut(*outs(res[1]), p(d_off), p(d_ns))
    capi._sig(hmm.hipstr_em_train, C.c_int, [C.POINTER(capi.HipstrEmBatch), u8p, f64p, i32p, f64p])
    why = lambda: hmm.hipstr_last_error().decode()

    def em_alone():
        assert hmm.hipstr_em_train(C.byref(eb), *outs(res[0])) == 0, why()

    def chain_a():
        assert hmm.hipstr_trace_dev_fetch(td.h, capi.TRACE_F_SCALARS | capi.TRACE_F_STR_SEQ, C.byref(o)) == 0, why()
        assert hmm.hipstr_em_batch_from_traces(pb.ptr, C.byref(rq), C.byref(o), p(e_off), p(e_lab), p(e_bps), pf(e_p1), pf(e_p2)) == 0, why()
        em_alone()

    def call_b():
        assert hmm.hipstr_em_train_dev(pd, C.byref(rq), td.h, C.byref(eo)) == 0, why()

    def timed(fn):
        fn()                                                          # warm-up
        ts = []
        for _ in range(REPS):
            t0 = time.perf_counter(); fn(); ts.append(1e3 * (time.perf_counter() - t0))
        return dict(median=float(np.median(ts)), min=min(ts), max=max(ts))

    # the two paths give the same answers: checked once before anything is timed
    chain_a(); call_b()
    assert all(np.array_equal(x, y) for x, y in zip(res[0], res[1])) and np.array_equal(d_off, e_off)
    m = int(e_off[-1]); n_alleles = int(d_ns.sum())
    out = dict(host_threads=os.environ.get("HIPSTR_HOST_THREADS"), requests=int(nq), reads=int(n), entering=m, alleles=n_alleles,
               trained=int(res[1][0].sum()), rounds=[int(res[1][2].min()), int(res[1][2].max())])
    for name, fn in (("chain_a", chain_a), ("call_b", call_b), ("em_alone", em_alone)):
        out[name] = timed(fn)
    # ---- bytes over the host link.  hipstr_em_train sends seven per-read and per-allele arrays (sizes, indices, labels, weights, log_p1,
    # log_p2: 32 bytes a read; sizes and log frequencies: 12 bytes an allele); both paths send the loop's locus records and units and bring
    # the four results home (not counted: the same on both)
    em_up = 32 * m + 12 * n_alleles
    out["bytes"] = dict(chain_a=dict(d2h=32 * nq + 4 * (nq + 1) + int(tot[1]), h2d=em_up),
                        call_b=dict(d2h=4 * ns + 4 * (4 * NL + 2), h2d=8 * n + 24 * NL + 4 * ns))
    td.close(); hmm.hipstr_post_free(pd); rm.close(); hmm.hipstr_hmm_free(dev)
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
    lines = ["The stutter model retrained from resident tracebacks (tools/em_resident_timing.py)",
             "commit: %s" % commit,
             "shape: %d loci x %d reads x %d STR alleles, %d samples per locus; %d requests; %d of %d reads enter the EM, %d allele sizes in all; %d loci trained in %d .. %d rounds" %
             (NL, P, A_STR, S, r0["requests"], r0["entering"], r0["reads"], r0["alleles"], r0["trained"], r0["rounds"][0], r0["rounds"][1]),
             "wall time of the C calls alone: 1 warm-up, then %d calls: median (fastest .. slowest)" % REPS,
             "  (a) hipstr_trace_dev_fetch(SCALARS | STR_SEQ) + hipstr_em_batch_from_traces + hipstr_em_train",
             "  (b) hipstr_em_train_dev",
             "  (c) hipstr_em_train alone on the batch of (a): the EM itself, part of both", ""]
    for r in runs:
        lines += ["HIPSTR_HOST_THREADS=%s" % r["host_threads"],
                  "  (a) %s   (b) %s   (c) %s   (b)/(a) %.2f" % (fmt(r["chain_a"]), fmt(r["call_b"]), fmt(r["em_alone"]), r["call_b"]["median"] / r["chain_a"]["median"])]
    by = r0["bytes"]
    lines += ["", "bytes over the host link per step (the loop's locus records and units up and its four results home are the same on both and not counted):"]
    for k, name in (("chain_a", "(a)"), ("call_b", "(b)")):
        lines.append("  %s  device to host %10d   host to device %10d" % (name, by[k]["d2h"], by[k]["h2d"]))
    slower = [r["host_threads"] for r in runs if r["call_b"]["median"] >= r["chain_a"]["median"]]
    lines.append("(b) not faster than (a): %s" % (", ".join("at %s threads" % t for t in slower) if slower else "nowhere"))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "em_resident_timing.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
