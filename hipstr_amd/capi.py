"""ctypes view of include/hipstr_hmm.h plus a small numpy batch builder.

This module is plumbing for tests and bench.py: it mirrors the two C structs of
the boundary (hipstr_batch_t, hipstr_post_batch_t), loads the product library
(hipstr_amd/csrc/libhipstr_hmm.so — HIP, no CPU fallback) and the bench/test
support libraries.  Loading anything under oracle/ is restricted to tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg (see load_oracle /
load_ref docstrings).
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMM_LIB = os.environ.get("HIPSTR_HMM_LIB") or os.path.join(ROOT, "hipstr_amd", "csrc", "libhipstr_hmm.so")     # the override: variant builds (tools/build_variant.sh)
SYNTH_LIB = os.path.join(ROOT, "hipstr_amd", "synth", "libhipstr_synth.so")
ORACLE_LIB = os.path.join(ROOT, "oracle", "libhipstr_oracle.so")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libhipstr_ref.so")

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)


class HipstrBatch(C.Structure):
    _fields_ = [
        ("n_loci", C.c_int32),
        ("blk_start", _i32p), ("blk_end", _i32p), ("blk_nopts", _i32p), ("period", _i32p),
        ("stutter", _f64p), ("opt_off", _i32p), ("seq", C.c_char_p), ("hap_off", _i32p), ("realign_hap", _u8p),
        ("read_off", _i32p), ("base_off", _i32p), ("bases", C.c_char_p), ("quals", C.c_char_p),
        ("read_start", _i32p), ("cigar_off", _i32p), ("cigar_op", C.c_char_p), ("cigar_len", _i32p),
        ("realign_read", _u8p),
    ]


class HipstrPostBatch(C.Structure):
    _fields_ = [
        ("n_loci", C.c_int32),
        ("n_alleles", _i32p), ("n_samples", _i32p), ("read_off", _i32p), ("sample_label", _i32p),
        ("log_p1", _f64p), ("log_p2", _f64p), ("read_weight", _i32p), ("log_aln_probs", _f64p), ("haploid", _u8p), ("log_prior", _f64p),
    ]


class HipstrNwBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("ref_off", _i32p), ("ref_seqs", C.c_char_p), ("read_off", _i32p), ("read_seqs", C.c_char_p),
                ("use_ref_end_penalty", C.c_int32)]


class HipstrNwOut(C.Structure):
    _fields_ = [("score", C.POINTER(C.c_float)), ("ok", _u8p), ("aln_off", C.POINTER(C.c_int64)), ("ref_al", C.c_char_p), ("read_al", C.c_char_p),
                ("cigar_off", C.POINTER(C.c_int64)), ("cigar_op", C.c_char_p), ("cigar_len", _i32p), ("cap_aln", C.c_int64), ("cap_cigar", C.c_int64)]


def run_nw(lib, prefix, pairs, use_ref_end_penalty=False, unpack=True, timing=None):
    """<prefix>nw_align on [(ref, read), ...] (str) -> list of (score, ok, ref_al, read_al, cigar string)."""
    import time
    n = len(pairs)
    refs = [r.encode() for r, _ in pairs]; reads = [q.encode() for _, q in pairs]
    ro = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    qo = np.concatenate([[0], np.cumsum([len(q) for q in reads])]).astype(np.int32)
    rb = b"".join(refs); qb = b"".join(reads)
    nb = HipstrNwBatch(n, ro.ctypes.data_as(_i32p), rb, qo.ctypes.data_as(_i32p), qb, int(use_ref_end_penalty))
    cap = int(ro[-1] + qo[-1] + 16)
    score = np.zeros(max(n, 1), np.float32); ok = np.zeros(max(n, 1), np.uint8)
    ao = np.zeros(n + 1, np.int64); co = np.zeros(n + 1, np.int64)
    ra = C.create_string_buffer(cap); qa = C.create_string_buffer(cap); cop = C.create_string_buffer(cap); cl = np.zeros(cap, np.int32)
    i64p = C.POINTER(C.c_int64)
    o = HipstrNwOut(score.ctypes.data_as(C.POINTER(C.c_float)), ok.ctypes.data_as(_u8p), ao.ctypes.data_as(i64p), C.cast(ra, C.c_char_p),
                    C.cast(qa, C.c_char_p), co.ctypes.data_as(i64p), C.cast(cop, C.c_char_p), cl.ctypes.data_as(_i32p), cap, cap)
    fn = getattr(lib, prefix + "nw_align")
    _sig(fn, C.c_int, [C.POINTER(HipstrNwBatch), C.POINTER(HipstrNwOut)])
    t0 = time.perf_counter()
    rc = fn(C.byref(nb), C.byref(o))
    if timing is not None:
        timing["call_s"] = timing.get("call_s", 0.0) + time.perf_counter() - t0
    if rc != 0:
        why = lib.hipstr_last_error().decode() if prefix == "hipstr_" else ""
        raise RuntimeError("%snw_align failed rc=%d %s" % (prefix, rc, why))
    if not unpack:
        return None
    out = []
    copr, rar, qar = cop.raw, ra.raw, qa.raw
    for i in range(n):
        cig = "".join("%d%s" % (cl[k], copr[k:k + 1].decode()) for k in range(co[i], co[i + 1]))
        out.append((float(score[i]), bool(ok[i]), rar[ao[i]:ao[i + 1]].decode(), qar[ao[i]:ao[i + 1]].decode(), cig))
    return out


class HipstrEmBatch(C.Structure):
    _fields_ = [("n_loci", C.c_int32), ("period", _i32p), ("haploid", _u8p), ("n_samples", _i32p), ("read_off", _i32p), ("sample_label", _i32p),
                ("num_bps", _i32p), ("log_p1", _f64p), ("log_p2", _f64p), ("ref_allele", C.c_int32), ("max_iter", C.c_int32),
                ("min_ll_abs_change", C.c_double), ("min_ll_frac_change", C.c_double)]


def _em_batch(period, n_samples, read_off, sample_label, num_bps, log_p1, log_p2, haploid=None, ref_allele=0, max_iter=100,
              min_ll_abs_change=0.01, min_ll_frac_change=0.001):
    """(HipstrEmBatch, the arrays it points into, loci)."""
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32)); f64 = lambda x: np.ascontiguousarray(np.asarray(x, np.float64))
    a = dict(period=i32(period), n_samples=i32(n_samples), read_off=i32(read_off), sample_label=i32(sample_label), num_bps=i32(num_bps),
             log_p1=f64(log_p1), log_p2=f64(log_p2), haploid=None if haploid is None else np.ascontiguousarray(np.asarray(haploid, np.uint8)))
    nl = len(a["period"])
    eb = HipstrEmBatch(nl, a["period"].ctypes.data_as(_i32p), _ptr(a["haploid"], _u8p), a["n_samples"].ctypes.data_as(_i32p),
                       a["read_off"].ctypes.data_as(_i32p), a["sample_label"].ctypes.data_as(_i32p), a["num_bps"].ctypes.data_as(_i32p),
                       a["log_p1"].ctypes.data_as(_f64p), a["log_p2"].ctypes.data_as(_f64p), ref_allele, max_iter, min_ll_abs_change, min_ll_frac_change)
    return eb, a, nl


def em_plan(lib, **kw):
    """The launch decisions hipstr_em_train takes for run_em's keyword arguments (host only: hipstr_debug_em_plan) as a dict; a batch the
    call refuses raises with the call's message."""
    eb, a, nl = _em_batch(**kw)
    return _plan_json(lib, "hipstr_debug_em_plan", lambda buf, cap: lib.hipstr_debug_em_plan(C.byref(eb), buf, cap))


def run_em(lib, prefix, period, n_samples, read_off, sample_label, num_bps, log_p1, log_p2, haploid=None, ref_allele=0, max_iter=100,
           min_ll_abs_change=0.01, min_ll_frac_change=0.001):
    """<prefix>em_train on a batch of loci -> (trained[n_loci] bool, stutter[n_loci, 6], n_iter[n_loci], final_ll[n_loci])."""
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32)); f64 = lambda x: np.ascontiguousarray(np.asarray(x, np.float64))
    a = dict(period=i32(period), n_samples=i32(n_samples), read_off=i32(read_off), sample_label=i32(sample_label), num_bps=i32(num_bps),
             log_p1=f64(log_p1), log_p2=f64(log_p2), haploid=None if haploid is None else np.ascontiguousarray(np.asarray(haploid, np.uint8)))
    nl = len(a["period"])
    eb = HipstrEmBatch(nl, a["period"].ctypes.data_as(_i32p), _ptr(a["haploid"], _u8p), a["n_samples"].ctypes.data_as(_i32p),
                       a["read_off"].ctypes.data_as(_i32p), a["sample_label"].ctypes.data_as(_i32p), a["num_bps"].ctypes.data_as(_i32p),
                       a["log_p1"].ctypes.data_as(_f64p), a["log_p2"].ctypes.data_as(_f64p), ref_allele, max_iter, min_ll_abs_change, min_ll_frac_change)
    trained = np.zeros(max(nl, 1), np.uint8); st = np.zeros(max(6 * nl, 6)); it = np.zeros(max(nl, 1), np.int32); ll = np.zeros(max(nl, 1))
    fn = getattr(lib, prefix + "em_train")
    _sig(fn, C.c_int, [C.POINTER(HipstrEmBatch), _u8p, _f64p, _i32p, _f64p])
    rc = fn(C.byref(eb), trained.ctypes.data_as(_u8p), st.ctypes.data_as(_f64p), it.ctypes.data_as(_i32p), ll.ctypes.data_as(_f64p))
    if rc != 0:
        why = lib.hipstr_last_error().decode() if prefix == "hipstr_" else ""
        raise RuntimeError("%sem_train failed rc=%d %s" % (prefix, rc, why))
    return trained[:nl].astype(bool), st[:6 * nl].reshape(-1, 6), it[:nl], ll[:nl]


class HipstrGtRequest(C.Structure):
    _fields_ = [("n_variants", _i32p), ("hap_to_allele", _i32p), ("calc_gls", C.c_int32), ("calc_pls", C.c_int32), ("calc_phased_gls", C.c_int32)]


class HipstrGtOut(C.Structure):
    _fields_ = [("best_hap", _i32p), ("best_gt", _i32p), ("log_phased_post", _f64p), ("log_unphased_post", _f64p),
                ("hap_log_phased_post", _f64p), ("hap_log_unphased_post", _f64p), ("gl_diff", _f64p), ("gls", _f64p), ("pls", _i32p),
                ("phased_gls", _f64p)]


def run_gt_extract(lib, prefix, pb, n_variants, hap_to_allele, calc_gls=True, calc_pls=True, calc_phased_gls=True):
    """Genotype calls of a PostBatch: <prefix>gt_extract(pb, request, out) for the oracle / reference probe (which compute
    the posteriors themselves), hipstr_post_upload + launch + hipstr_post_extract for the product.  Returns a dict of arrays;
    gls / pls / phased_gls are lists with one array per sample."""
    nl = pb.struct.n_loci
    S = int(pb.samp_off[-1])
    nv = np.ascontiguousarray(np.asarray(n_variants, np.int32)); h2a = np.ascontiguousarray(np.asarray(hap_to_allele, np.int32))
    rq = HipstrGtRequest(nv.ctypes.data_as(_i32p), h2a.ctypes.data_as(_i32p), int(calc_gls), int(calc_pls), int(calc_phased_gls))
    hap = pb.a["haploid"] if pb.a["haploid"] is not None else np.zeros(nl, np.uint8)
    gl_off = [0]; pgl_off = [0]
    for l in range(nl):
        V = int(nv[l])
        for _ in range(int(pb.a["n_samples"][l])):
            gl_off.append(gl_off[-1] + (V if hap[l] else V * (V + 1) // 2)); pgl_off.append(pgl_off[-1] + (V if hap[l] else V * V))
    k = dict(best_hap=np.zeros(max(2 * S, 2), np.int32), best_gt=np.zeros(max(2 * S, 2), np.int32))
    for nm in ("log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff"):
        k[nm] = np.zeros(max(S, 1))
    k["gls"] = np.zeros(max(gl_off[-1], 1)); k["pls"] = np.zeros(max(gl_off[-1], 1), np.int32); k["phased_gls"] = np.zeros(max(pgl_off[-1], 1))
    o = HipstrGtOut(*[k[f].ctypes.data_as(t) for f, t in HipstrGtOut._fields_])
    if prefix == "hipstr_":
        _sig(lib.hipstr_post_extract, C.c_int, [C.c_void_p, C.POINTER(HipstrGtRequest), C.POINTER(HipstrGtOut)])
        _sig(lib.hipstr_gt_offsets, C.c_int, [C.POINTER(HipstrPostBatch), C.POINTER(HipstrGtRequest), C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
        go = np.zeros(S + 1, np.int64); pgo = np.zeros(S + 1, np.int64)
        i64p = C.POINTER(C.c_int64)
        assert lib.hipstr_gt_offsets(pb.ptr, C.byref(rq), go.ctypes.data_as(i64p), pgo.ctypes.data_as(i64p)) == 0
        assert list(go) == gl_off and list(pgo) == pgl_off
        pd = lib.hipstr_post_upload(pb.ptr, None)
        if not pd:
            raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())
        try:
            rc = lib.hipstr_post_launch(pd, None)
            if rc == 0:
                rc = lib.hipstr_post_extract(pd, C.byref(rq), C.byref(o))
        finally:
            lib.hipstr_post_free(pd)
        if rc != 0:
            raise RuntimeError("hipstr_post_extract failed: " + lib.hipstr_last_error().decode())
    else:
        fn = getattr(lib, prefix + "gt_extract")
        _sig(fn, C.c_int, [C.POINTER(HipstrPostBatch), C.POINTER(HipstrGtRequest), C.POINTER(HipstrGtOut)])
        rc = fn(pb.ptr, C.byref(rq), C.byref(o))
        if rc != 0:
            raise RuntimeError("%sgt_extract failed rc=%d" % (prefix, rc))
    out = dict(best_hap=k["best_hap"][:2 * S].reshape(-1, 2), best_gt=k["best_gt"][:2 * S].reshape(-1, 2))
    for nm in ("log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff"):
        out[nm] = k[nm][:S]
    out["gls"] = [k["gls"][gl_off[s]:gl_off[s + 1]] for s in range(S)]
    out["pls"] = [k["pls"][gl_off[s]:gl_off[s + 1]] for s in range(S)]
    out["phased_gls"] = [k["phased_gls"][pgl_off[s]:pgl_off[s + 1]] for s in range(S)]
    return out


class HipstrAssignRequest(C.Structure):
    _fields_ = [("seed", _i32p), ("reverse", _u8p), ("pool_index", _i32p), ("pool_off", _i32p), ("rule", C.c_int32), ("strand_tolerance", C.c_double)]


class HipstrAssignOut(C.Structure):
    _fields_ = [("best_hap", _i32p), ("read_strand", _i32p), ("log_phase_one", _f64p),
                ("n_aligned", _i32p), ("n_snp", _i32p), ("n_strand_one", _i32p), ("n_strand_two", _i32p),
                ("uniq_one", _i32p), ("uniq_two", _i32p), ("rv_uniq_one", _i32p), ("rv_uniq_two", _i32p),
                ("phase1_reads", _f64p), ("phase2_reads", _f64p),
                ("n_req", _i32p), ("req_read", _i32p), ("req_allele", _i32p), ("read_req", _i32p), ("cap_req", C.c_int32)]


ASSIGN_VCF, ASSIGN_RETRACE = 0, 1
ASSIGN_COUNTERS = ("n_aligned", "n_snp", "n_strand_one", "n_strand_two", "uniq_one", "uniq_two", "rv_uniq_one", "rv_uniq_two")
NO_ML_BP = -2 ** 31
UNTOUCHED = -7          # what run_assign fills the integer outputs with before the call (log_phase_one: NaN)


def run_assign(lib, pd_or_pb, seed, reverse=None, pool_index=None, pool_off=None, rule=ASSIGN_VCF, strand_tolerance=0.0, cap_req=None,
               n_reads=None, n_samp=None, dev_ll=None):
    """hipstr_post_assign -> dict of arrays (+ "rc": 0, or 3 when cap_req was too small: then only "n_req" means anything).
    pd_or_pb: a PostBatch (uploaded, launched, assigned and freed here; dev_ll = device pointer of the likelihoods or None) or a
    hipstr_post_dev_t handle after hipstr_post_launch (then n_reads and n_samp say how long the outputs are).  Outputs the call leaves
    untouched keep UNTOUCHED (integers) / NaN (log_phase_one).  Raises on any other failure."""
    _sig(lib.hipstr_post_assign, C.c_int, [C.c_void_p, C.POINTER(HipstrAssignRequest), C.POINTER(HipstrAssignOut)])
    own = isinstance(pd_or_pb, PostBatch)
    if own:
        n_reads = int(pd_or_pb.a["read_off"][-1]) if len(pd_or_pb.a["read_off"]) else 0
        n_samp = int(pd_or_pb.samp_off[-1])
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    k_in = dict(seed=i32(seed), reverse=None if reverse is None else np.ascontiguousarray(np.asarray(reverse, np.uint8)),
                pool_index=i32(pool_index), pool_off=i32(pool_off))
    rq = HipstrAssignRequest(_ptr(k_in["seed"], _i32p), _ptr(k_in["reverse"], _u8p), _ptr(k_in["pool_index"], _i32p), _ptr(k_in["pool_off"], _i32p),
                             int(rule), float(strand_tolerance))
    if cap_req is None:
        cap_req = n_reads
    k = dict(best_hap=np.full(max(n_reads, 1), UNTOUCHED, np.int32), read_strand=np.full(max(n_reads, 1), UNTOUCHED, np.int32),
             log_phase_one=np.full(max(n_reads, 1), np.nan), phase1_reads=np.full(max(n_samp, 1), np.nan), phase2_reads=np.full(max(n_samp, 1), np.nan),
             n_req=np.full(1, UNTOUCHED, np.int32), req_read=np.full(max(cap_req, 1), UNTOUCHED, np.int32),
             req_allele=np.full(max(cap_req, 1), UNTOUCHED, np.int32), read_req=np.full(max(n_reads, 1), UNTOUCHED, np.int32))
    for nm in ASSIGN_COUNTERS:
        k[nm] = np.full(max(n_samp, 1), UNTOUCHED, np.int32)
    o = HipstrAssignOut(*([k[f].ctypes.data_as(t) for f, t in HipstrAssignOut._fields_[:-1]] + [int(cap_req)]))
    pd = pd_or_pb
    if own:
        pd = lib.hipstr_post_upload(pd_or_pb.ptr, dev_ll)
        if not pd:
            raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())
    try:
        rc = lib.hipstr_post_launch(pd, None) if own else 0
        if rc != 0:
            raise RuntimeError("hipstr_post_launch failed: " + lib.hipstr_last_error().decode())
        rc = lib.hipstr_post_assign(pd, C.byref(rq), C.byref(o))
    finally:
        if own:
            lib.hipstr_post_free(pd)
    if rc not in (0, 3):
        raise RuntimeError("hipstr_post_assign failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    out = {nm: k[nm][:n_reads] for nm in ("best_hap", "read_strand", "log_phase_one", "read_req")}
    for nm in ASSIGN_COUNTERS + ("phase1_reads", "phase2_reads"):
        out[nm] = k[nm][:n_samp]
    out["n_req"] = int(k["n_req"][0])
    nq = out["n_req"] if (rc == 0 and pool_index is not None) else 0
    out["req_read"] = k["req_read"][:nq]; out["req_allele"] = k["req_allele"][:nq]
    out["rc"] = rc
    return out


def run_assign_trace_stats(lib, pb, read_req, trace, best_hap, hap_to_allele, allele_bp_diff, n_variants, region_start, region_stop):
    """hipstr_assign_trace_stats (host only) -> (n_stutter[n_samp], n_flank_indel[n_samp], ml_bp[n_reads]).  trace: dict with the arrays
    stutter_size, flank_ins, flank_del, aln_start, aln_stop per request (run_trace(..., unpack=False) returns such a dict)."""
    _sig(lib.hipstr_assign_trace_stats, C.c_int, [_PBP, _i32p, C.POINTER(HipstrTraceOut)] + [_i32p] * 9)
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))
    t = HipstrTraceOut(); keep = {}
    for nm in ("stutter_size", "flank_ins", "flank_del", "aln_start", "aln_stop"):
        if trace.get(nm) is not None:
            keep[nm] = i32(trace[nm]); setattr(t, nm, keep[nm].ctypes.data_as(_i32p))
    n_reads = int(pb.a["read_off"][-1]) if len(pb.a["read_off"]) else 0
    n_samp = int(pb.samp_off[-1])
    a = [i32(x) for x in (read_req, best_hap, hap_to_allele, allele_bp_diff, n_variants, region_start, region_stop)]
    ns = np.full(max(n_samp, 1), UNTOUCHED, np.int32); nf = np.full(max(n_samp, 1), UNTOUCHED, np.int32); ml = np.full(max(n_reads, 1), UNTOUCHED, np.int32)
    p = lambda x: x.ctypes.data_as(_i32p)
    rc = lib.hipstr_assign_trace_stats(pb.ptr, p(a[0]), C.byref(t), p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), p(ns), p(nf), p(ml))
    if rc != 0:
        raise RuntimeError("hipstr_assign_trace_stats failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    return ns[:n_samp], nf[:n_samp], ml[:n_reads]


class HipstrReadLayout(C.Structure):
    _fields_ = [("n_loci", C.c_int32), ("n_alleles", _i32p), ("read_off", _i32p), ("pool_index", _i32p), ("second_mate", _u8p)]


class ReadMatrix:
    """hipstr_rm_*: the read x haplotype matrix of a batch of loci resident on the device (include/hipstr_hmm.h).  Every call raises
    with hipstr_last_error() when the library refuses it."""

    def __init__(self, lib, n_alleles, read_off, pool_index, second_mate=None, init_ll=None, init_seeds=None):
        self.lib = lib; self.h = None
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))
        self.n_alleles = i32(n_alleles); self.read_off = i32(read_off)
        keep = [self.n_alleles, self.read_off, i32(pool_index), None if second_mate is None else np.ascontiguousarray(np.asarray(second_mate, np.uint8)),
                None if init_ll is None else np.ascontiguousarray(np.asarray(init_ll, np.float64)), None if init_seeds is None else i32(init_seeds)]
        lay = HipstrReadLayout(len(self.n_alleles), _ptr(keep[0], _i32p), _ptr(keep[1], _i32p), _ptr(keep[2], _i32p), _ptr(keep[3], _u8p))
        self.h = lib.hipstr_rm_create(C.byref(lay), _ptr(keep[4], _f64p), _ptr(keep[5], _i32p))
        if not self.h:
            raise RuntimeError("hipstr_rm_create failed: " + lib.hipstr_last_error().decode())

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed rc=%d: %s" % (what, rc, self.lib.hipstr_last_error().decode()))

    def scatter(self, dev, copy_read=None):
        c = None if copy_read is None else np.ascontiguousarray(np.asarray(copy_read, np.uint8))
        self._check(self.lib.hipstr_rm_scatter(self.h, dev, _ptr(c, _u8p)), "hipstr_rm_scatter")

    def remap(self, new_n_alleles, allele_mapping):
        na = np.ascontiguousarray(np.asarray(new_n_alleles, np.int32)); am = np.ascontiguousarray(np.asarray(allele_mapping, np.int32))
        self._check(self.lib.hipstr_rm_remap(self.h, _ptr(na, _i32p), _ptr(am, _i32p)), "hipstr_rm_remap")
        self.n_alleles = na

    @property
    def dev_ll(self):
        return self.lib.hipstr_rm_dev_log_aln_probs(self.h)

    def fetch(self):
        """(log_aln_probs, seeds) as they lie on the device."""
        R = np.diff(self.read_off).astype(np.int64)
        ll = np.zeros(max(int((R * self.n_alleles).sum()), 1)); seeds = np.zeros(max(int(R.sum()), 1), np.int32)
        self._check(self.lib.hipstr_rm_fetch(self.h, ll.ctypes.data_as(_f64p), seeds.ctypes.data_as(_i32p)), "hipstr_rm_fetch")
        return ll[:int((R * self.n_alleles).sum())], seeds[:int(R.sum())]

    def close(self):
        if self.h:
            self.lib.hipstr_rm_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rm_plan(lib, n_alleles, n_items):
    """hipstr_debug_rm_plan (host only) as a dict: the route of a locus of n_alleles haplotypes and n_items mate groups / rows."""
    out = np.zeros(5, np.int64)
    if lib.hipstr_debug_rm_plan(int(n_alleles), int(n_items), out.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise RuntimeError("hipstr_debug_rm_plan failed: " + lib.hipstr_last_error().decode())
    return dict(route="wide" if out[0] else "narrow", lanes=int(out[1]), items_per_wave=int(out[2]), waves=int(out[3]), column_steps=int(out[4]))


class HipstrTraceOut(C.Structure):
    _fields_ = [("ll", _f64p), ("max_index", _i32p), ("hap_aln_off", _i32p), ("hap_aln", C.c_char_p), ("stutter_size", _i32p),
                ("str_seq_off", _i32p), ("str_seq", C.c_char_p), ("flank_seq_off", _i32p), ("flank_seq", C.c_char_p),
                ("flank_ins", _i32p), ("flank_del", _i32p), ("indel_off", _i32p), ("indel_pos", _i32p), ("indel_size", _i32p),
                ("snp_off", _i32p), ("snp_pos", _i32p), ("snp_base", C.c_char_p), ("aln_start", _i32p), ("aln_stop", _i32p),
                ("cigar_off", _i32p), ("cigar_op", C.c_char_p), ("cigar_len", _i32p), ("aln_str_off", _i32p), ("aln_str", C.c_char_p),
                ("cap_chars", C.c_int32)]


class HipstrCensusRequest(C.Structure):
    _fields_ = [("pooled", C.POINTER(HipstrBatch)), ("seed", _i32p), ("read_req", _i32p), ("n_req", C.c_int32), ("req_read", _i32p),
                ("trace", C.POINTER(HipstrTraceOut)), ("hap_to_allele", _i32p * 3), ("sample_uncallable", _u8p), ("min_reads", C.c_int32),
                ("min_frac", C.c_double)]


class HipstrCensusOut(C.Structure):
    _fields_ = [("cand_off", _i32p), ("cand_req", _i32p), ("cand_seq_off", _i32p), ("cand_seq", C.c_char_p), ("new_n_haps", C.POINTER(C.c_int64)),
                ("n_spanning", _i32p), ("n_span_stutter", _i32p), ("called", _u8p), ("spanned", _u8p), ("cap_cand", C.c_int32), ("cap_chars", C.c_int32)]


CENSUS_ROUTES = ("wave", "lds", "global")
CENSUS_FILL = 0xAA      # what run_census fills called / spanned with before the call


def census_trace(aln_start, aln_stop, stutter_size, str_seqs):
    """Hand-made trace fields for run_census: str_seqs is a list of bytes, one per request."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in str_seqs])]).astype(np.int32) if len(str_seqs) else np.zeros(1, np.int32)
    return dict(aln_start=aln_start, aln_stop=aln_stop, stutter_size=stutter_size, str_seq_off=off, str_seq=b"".join(str_seqs))


def run_census(lib, pd_or_pb, bptr, seed, read_req, req_read, trace, hap_to_allele=(None, None, None), sample_uncallable=None, min_reads=0,
               min_frac=0.0, cap_cand=None, cap_chars=None, n_samp=None, dev_ll=None, td=None):
    """hipstr_post_census -> dict: "rc" (0, or 3 when cap_cand / cap_chars was too small: then only "cand_off" means anything), "cand_off",
    "cand_req", "cand" (per locus the list of candidate strings, bytes), "new_n_haps", "n_spanning", "n_span_stutter", "called", "spanned"
    (uint8 per option; CENSUS_FILL where the call wrote nothing).  pd_or_pb: a PostBatch (uploaded, launched and freed here; dev_ll = device
    pointer of the likelihoods or None) or a hipstr_post_dev_t handle after hipstr_post_launch (then n_samp says how long the per-sample
    outputs are).  bptr: the pooled batch (Batch.ptr / SynthBatch.ptr).  trace: dict with aln_start, aln_stop, stutter_size, str_seq_off and
    str_seq (bytes, or run_trace(..., unpack=False)'s buffer).  td: a TraceDev instead of `trace` (then None): hipstr_post_census_dev reads
    the five fields from the resident result.  Raises on any other failure."""
    _sig(lib.hipstr_post_census, C.c_int, [C.c_void_p, C.POINTER(HipstrCensusRequest), C.POINTER(HipstrCensusOut)])
    _sig(lib.hipstr_post_census_dev, C.c_int, [C.c_void_p, C.POINTER(HipstrCensusRequest), C.c_void_p, C.POINTER(HipstrCensusOut)])
    fn_name = "hipstr_post_census" if td is None else "hipstr_post_census_dev"
    own = isinstance(pd_or_pb, PostBatch)
    if own:
        n_samp = int(pd_or_pb.samp_off[-1])
    b = bptr.contents if hasattr(bptr, "contents") else (bptr._obj if hasattr(bptr, "_obj") else bptr)
    nl = int(b.n_loci)
    nopts = np.ctypeslib.as_array(b.blk_nopts, shape=(3 * nl,)) if nl else np.zeros(0, np.int32)
    n_opts = int(nopts.sum())
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    keep = dict(seed=i32(seed), read_req=i32(read_req), req_read=i32(req_read))
    n_req = 0 if keep["req_read"] is None else len(keep["req_read"])
    t = HipstrTraceOut()
    for nm in ("aln_start", "aln_stop", "stutter_size", "str_seq_off"):
        if trace is not None and trace.get(nm) is not None:
            keep[nm] = i32(trace[nm]); setattr(t, nm, keep[nm].ctypes.data_as(_i32p))
    if trace is not None and trace.get("str_seq") is not None:
        keep["str_seq"] = trace["str_seq"]
        t.str_seq = keep["str_seq"] if isinstance(keep["str_seq"], bytes) else C.cast(keep["str_seq"], C.c_char_p)
    h2a = [i32(x) for x in hap_to_allele]
    unc = None if sample_uncallable is None else np.ascontiguousarray(np.asarray(sample_uncallable, np.uint8))
    rq = HipstrCensusRequest(C.cast(bptr, C.POINTER(HipstrBatch)) if not hasattr(bptr, "_obj") else C.pointer(bptr._obj), _ptr(keep["seed"], _i32p),
                             _ptr(keep["read_req"], _i32p), n_req, _ptr(keep["req_read"], _i32p), C.pointer(t) if trace is not None else None,
                             (_i32p * 3)(*[_ptr(x, _i32p) for x in h2a]), _ptr(unc, _u8p), int(min_reads), float(min_frac))
    if cap_cand is None:
        cap_cand = n_req
    if cap_chars is None and td is not None:
        cap_chars = int(td.sizes()[1][1])
    if cap_chars is None:
        cap_chars = int(keep["str_seq_off"][-1]) if "str_seq_off" in keep and len(keep["str_seq_off"]) else 0
    k = dict(cand_off=np.full(nl + 1, UNTOUCHED, np.int32), cand_req=np.full(max(cap_cand, 1), UNTOUCHED, np.int32),
             cand_seq_off=np.full(max(cap_cand, 0) + 1, UNTOUCHED, np.int32), new_n_haps=np.full(max(nl, 1), UNTOUCHED, np.int64),
             n_spanning=np.full(max(n_samp, 1), UNTOUCHED, np.int32), n_span_stutter=np.full(max(n_samp, 1), UNTOUCHED, np.int32),
             called=np.full(max(n_opts, 1), CENSUS_FILL, np.uint8), spanned=np.full(max(n_opts, 1), CENSUS_FILL, np.uint8))
    seq = C.create_string_buffer(max(cap_chars, 1))
    o = HipstrCensusOut(k["cand_off"].ctypes.data_as(_i32p), k["cand_req"].ctypes.data_as(_i32p), k["cand_seq_off"].ctypes.data_as(_i32p),
                        C.cast(seq, C.c_char_p), k["new_n_haps"].ctypes.data_as(C.POINTER(C.c_int64)), k["n_spanning"].ctypes.data_as(_i32p),
                        k["n_span_stutter"].ctypes.data_as(_i32p), k["called"].ctypes.data_as(_u8p), k["spanned"].ctypes.data_as(_u8p),
                        int(cap_cand), int(cap_chars))
    pd = pd_or_pb
    if own:
        pd = lib.hipstr_post_upload(pd_or_pb.ptr, dev_ll)
        if not pd:
            raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())
    try:
        rc = lib.hipstr_post_launch(pd, None) if own else 0
        if rc != 0:
            raise RuntimeError("hipstr_post_launch failed: " + lib.hipstr_last_error().decode())
        rc = lib.hipstr_post_census(pd, C.byref(rq), C.byref(o)) if td is None else lib.hipstr_post_census_dev(pd, C.byref(rq), td.h, C.byref(o))
    finally:
        if own:
            lib.hipstr_post_free(pd)
    if rc not in (0, 3):
        e = RuntimeError("%s failed rc=%d: %s" % (fn_name, rc, lib.hipstr_last_error().decode()))
        e.outputs = dict(k, cand_seq=seq.raw)          # what the refused call left in the output arrays (pre-filled above)
        raise e
    out = dict(rc=rc, cand_off=k["cand_off"], new_n_haps=k["new_n_haps"][:nl], n_spanning=k["n_spanning"][:n_samp],
               n_span_stutter=k["n_span_stutter"][:n_samp], called=k["called"][:n_opts], spanned=k["spanned"][:n_opts])
    nc = int(k["cand_off"][nl]) if rc == 0 else 0
    out["cand_req"] = k["cand_req"][:nc]
    raw = seq.raw
    flat = [raw[k["cand_seq_off"][i]:k["cand_seq_off"][i + 1]] for i in range(nc)]
    out["cand"] = [flat[k["cand_off"][l]:k["cand_off"][l + 1]] for l in range(nl)] if rc == 0 else None
    return out


# ---- the allele-set update between two rounds (hipstr_alleles_apply / _step): the constants are include/hipstr_hmm.h's HIPSTR_PHASE_* / HIPSTR_ALLELES_*
PHASE_ADD, PHASE_UNCALLED, PHASE_UNSPANNED, PHASE_DONE, PHASE_ABORTED = range(5)
ALLELES_ON_HOST = 1


class HipstrAllelesRequest(C.Structure):
    _fields_ = [("pooled", C.POINTER(HipstrBatch)), ("locus_on", _u8p), ("keep", _u8p), ("keep_blocks", C.c_uint32), ("add_off", _i32p),
                ("add_seq_off", _i32p), ("add_seq", C.c_char_p)]


class HipstrAllelesStepOut(C.Structure):
    _fields_ = [("status", _i32p), ("n_added", _i32p), ("n_removed", _i32p), ("n_affected_blocks", _i32p), ("any_added", C.c_int32)]


def _alleles_sigs(lib):
    _sig(lib.hipstr_alleles_apply, C.c_void_p, [C.POINTER(HipstrAllelesRequest)])
    _sig(lib.hipstr_alleles_apply_host, C.c_void_p, [C.POINTER(HipstrAllelesRequest)])
    _sig(lib.hipstr_alleles_step, C.c_void_p, [C.POINTER(HipstrBatch), C.POINTER(HipstrCensusOut), _i32p, C.c_int32, C.c_uint32, C.POINTER(HipstrAllelesStepOut)])
    for nm in ("hipstr_alleles_batch", "hipstr_alleles_batch_all"):
        _sig(getattr(lib, nm), C.POINTER(HipstrBatch), [C.c_void_p])
    _sig(lib.hipstr_alleles_mapping, _i32p, [C.c_void_p]); _sig(lib.hipstr_alleles_new_n_alleles, _i32p, [C.c_void_p])
    _sig(lib.hipstr_alleles_hap_to_allele, _i32p, [C.c_void_p, C.c_int]); _sig(lib.hipstr_alleles_added, _u8p, [C.c_void_p])
    _sig(lib.hipstr_alleles_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_alleles_hash_bits, C.c_int, [C.c_int])
    for nm, typ in (("hipstr_debug_alleles_last", C.c_int64), ("hipstr_debug_alleles_last_timing", C.c_double), ("hipstr_debug_alleles_limits", C.c_int64)):
        _sig(getattr(lib, nm), C.c_int, [C.POINTER(typ)])
    _sig(lib.hipstr_last_error, C.c_char_p, [])


def _batch_ptr(bptr):
    return C.cast(bptr, C.POINTER(HipstrBatch)) if not hasattr(bptr, "_obj") else C.pointer(bptr._obj)


class Alleles:
    """A hipstr_alleles_t: its arrays copied into numpy (mapping, new_n_alleles, h2a[3], added, realign_hap, blk_nopts, opt_off, seq, hap_off),
    .ptr / .ptr_all the two batches for the calls that follow (valid until free(); the pooled batch it came from must outlive it)."""

    def __init__(self, lib, h, old_bptr, keepalive):
        self.lib, self.h, self._keep = lib, h, (old_bptr, keepalive)
        old = old_bptr.contents
        nl = int(old.n_loci)
        self.ptr, self.ptr_all = lib.hipstr_alleles_batch(h), lib.hipstr_alleles_batch_all(h)
        nb = self.ptr.contents
        arr = lambda p, n, dt: (np.ctypeslib.as_array(p, shape=(n,)).astype(dt) if n else np.zeros(0, dt))
        old_A = int(old.hap_off[nl]) if nl else 0
        self.hap_off = arr(nb.hap_off, nl + 1, np.int32) if nl else np.zeros(1, np.int32)
        new_A = int(self.hap_off[-1])
        self.blk_nopts = arr(nb.blk_nopts, 3 * nl, np.int32)
        n_opts = int(self.blk_nopts.sum())
        self.opt_off = arr(nb.opt_off, n_opts + 1, np.int32) if nl else np.zeros(1, np.int32)
        self.seq = C.string_at(nb.seq, int(self.opt_off[-1])) if nl else b""
        self.realign_hap = arr(nb.realign_hap, new_A, np.uint8)
        self.all_mask_is_null = not bool(self.ptr_all.contents.realign_hap)
        self.mapping = arr(lib.hipstr_alleles_mapping(h), old_A, np.int32)
        self.new_n_alleles = arr(lib.hipstr_alleles_new_n_alleles(h), nl, np.int32)
        self.h2a = [arr(lib.hipstr_alleles_hap_to_allele(h, k), new_A, np.int32) for k in range(3)]
        self.added = arr(lib.hipstr_alleles_added(h), nl, np.uint8)

    def options(self):
        """per locus the three blocks' option strings (bytes)"""
        out = []; o = 0
        for l in range(len(self.new_n_alleles)):
            blocks = []
            for k in range(3):
                n = int(self.blk_nopts[3 * l + k])
                blocks.append([self.seq[self.opt_off[o + i]:self.opt_off[o + i + 1]] for i in range(n)]); o += n
            out.append(blocks)
        return out

    def arrays(self):
        """every output array, for comparisons between the two forms"""
        return dict(hap_off=self.hap_off, blk_nopts=self.blk_nopts, opt_off=self.opt_off, seq=np.frombuffer(self.seq, np.uint8), realign_hap=self.realign_hap,
                    mapping=self.mapping, new_n_alleles=self.new_n_alleles, h2a0=self.h2a[0], h2a1=self.h2a[1], h2a2=self.h2a[2], added=self.added)

    def free(self):
        if self.h:
            self.lib.hipstr_alleles_free(self.h); self.h = None; self.ptr = self.ptr_all = None

    def __del__(self):
        self.free()


def alleles_last(lib):
    """hipstr_debug_alleles_last as a dict"""
    _alleles_sigs(lib)
    v = (C.c_int64 * 8)()
    assert lib.hipstr_debug_alleles_last(v) == 0
    return dict(device_loci=int(v[0]), host_loci=int(v[1]), probes=int(v[2]), compares=int(v[3]), identity_loci=int(v[4]), chunks=int(v[5]))


def alleles_limits(lib):
    _alleles_sigs(lib)
    v = (C.c_int64 * 4)()
    assert lib.hipstr_debug_alleles_limits(v) == 0
    return dict(threads=int(v[0]), max_haps=int(v[1]), max_opts=int(v[2]), slots=int(v[3]))


def run_alleles_apply(lib, bptr, locus_on=None, keep=None, keep_blocks=7, add=None, host=False, raw=None):
    """hipstr_alleles_apply (host=True: _apply_host) -> Alleles.  bptr: the pooled batch (Batch.ptr).  keep: uint8 per old option or None;
    add: per locus three lists of bytes, or None.  raw: dict(add_off, add_seq_off, add_seq) handed over as given instead of `add` (the
    refusals' tests).  Raises RuntimeError with hipstr_last_error() on a refusal."""
    _alleles_sigs(lib)
    bp = _batch_ptr(bptr)
    nl = int(bp.contents.n_loci)
    u8 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.uint8))
    k = dict(locus_on=u8(locus_on), keep=u8(keep))
    if raw is not None:
        k["add_off"], k["add_seq_off"], k["add_seq"] = np.ascontiguousarray(raw["add_off"], np.int32), np.ascontiguousarray(raw["add_seq_off"], np.int32), raw["add_seq"] + b"\0"
    elif add is not None:
        assert len(add) == nl
        flat = [s for L in add for blk in L for s in blk]
        k["add_off"] = np.concatenate([[0], np.cumsum([len(blk) for L in add for blk in L])]).astype(np.int32)
        k["add_seq_off"] = np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int32)
        k["add_seq"] = b"".join(flat) + b"\0"
    rq = HipstrAllelesRequest(bp, _ptr(k["locus_on"], _u8p), _ptr(k["keep"], _u8p), int(keep_blocks), _ptr(k.get("add_off"), _i32p),
                              _ptr(k.get("add_seq_off"), _i32p), k.get("add_seq"))
    h = (lib.hipstr_alleles_apply_host if host else lib.hipstr_alleles_apply)(C.byref(rq))
    if not h:
        raise RuntimeError("hipstr_alleles_apply%s failed: %s" % ("_host" if host else "", lib.hipstr_last_error().decode()))
    return Alleles(lib, h, bp, (bptr, k, rq))


def run_alleles_step(lib, bptr, census, phase, max_total_haplotypes=0, host=False):
    """hipstr_alleles_step -> Alleles with .status, .n_added, .n_removed, .n_affected_blocks (int32 per locus) and .any_added.  census:
    run_census's dict (cand, new_n_haps, called, spanned are read).  phase: int32 array, updated in place unless the call is refused."""
    _alleles_sigs(lib)
    bp = _batch_ptr(bptr)
    nl = int(bp.contents.n_loci)
    assert isinstance(phase, np.ndarray) and phase.dtype == np.int32 and len(phase) == nl
    flat = [s for L in census["cand"] for s in L]
    k = dict(cand_off=np.concatenate([[0], np.cumsum([len(L) for L in census["cand"]])]).astype(np.int32),
             cand_seq_off=np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int32), cand_seq=b"".join(flat) + b"\0",
             new_n_haps=np.ascontiguousarray(np.asarray(census["new_n_haps"], np.int64)).reshape(-1),
             called=np.ascontiguousarray(np.asarray(census["called"], np.uint8)), spanned=np.ascontiguousarray(np.asarray(census["spanned"], np.uint8)))
    cen = HipstrCensusOut()
    cen.cand_off = _ptr(k["cand_off"], _i32p); cen.cand_seq_off = _ptr(k["cand_seq_off"], _i32p); cen.cand_seq = k["cand_seq"]
    cen.new_n_haps = k["new_n_haps"].ctypes.data_as(C.POINTER(C.c_int64)) if nl else None
    cen.called = _ptr(k["called"], _u8p); cen.spanned = _ptr(k["spanned"], _u8p)
    o = dict((nm, np.full(max(nl, 1), UNTOUCHED, np.int32)) for nm in ("status", "n_added", "n_removed", "n_affected_blocks"))
    so = HipstrAllelesStepOut(*[o[nm].ctypes.data_as(_i32p) for nm in ("status", "n_added", "n_removed", "n_affected_blocks")], -1)
    h = lib.hipstr_alleles_step(bp, C.byref(cen), phase.ctypes.data_as(_i32p), int(max_total_haplotypes), ALLELES_ON_HOST if host else 0, C.byref(so))
    if not h:
        e = RuntimeError("hipstr_alleles_step failed: %s" % lib.hipstr_last_error().decode())
        e.outputs = dict(o, any_added=int(so.any_added))
        raise e
    a = Alleles(lib, h, bp, (bptr, k, cen))
    a.status, a.n_added, a.n_removed, a.n_affected_blocks = [o[nm][:nl] for nm in ("status", "n_added", "n_removed", "n_affected_blocks")]
    a.any_added = int(so.any_added)
    return a


# ---- the resident traceback result (hipstr_hmm_trace_resident, hipstr_trace_dev_*): the constants are include/hipstr_hmm.h's HIPSTR_TRACE_F_*
TRACE_F_SCALARS, TRACE_F_HAP_ALN, TRACE_F_STR_SEQ, TRACE_F_FLANKS, TRACE_F_INDELS, TRACE_F_SNPS, TRACE_F_STITCH, TRACE_F_ALL = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x7f
# the arrays of every group: (name, kind, pool) — kind "f8" / "i4" per request, "off" an offset array, "i4p" / "chr" a pool array of pool `pool`
TRACE_GROUPS = {
    TRACE_F_SCALARS: [("ll", "f8", None), ("max_index", "i4", None), ("stutter_size", "i4", None), ("flank_ins", "i4", None), ("flank_del", "i4", None),
                      ("aln_start", "i4", None), ("aln_stop", "i4", None)],
    TRACE_F_HAP_ALN: [("hap_aln_off", "off", 0), ("hap_aln", "chr", 0)],
    TRACE_F_STR_SEQ: [("str_seq_off", "off", 1), ("str_seq", "chr", 1)],
    TRACE_F_FLANKS: [("flank_seq_off", "off", 2), ("flank_seq", "chr", 2)],
    TRACE_F_INDELS: [("indel_off", "off", 3), ("indel_pos", "i4p", 3), ("indel_size", "i4p", 3)],
    TRACE_F_SNPS: [("snp_off", "off", 4), ("snp_pos", "i4p", 4), ("snp_base", "chr", 4)],
    TRACE_F_STITCH: [("cigar_off", "off", 5), ("cigar_op", "chr", 5), ("cigar_len", "i4p", 5), ("aln_str_off", "off", 6), ("aln_str", "chr", 6)],
}
TRACE_SENTINEL = 0x5A        # what trace_dev_fetch fills every byte of every array with before the call


def _trace_dev_sigs(lib):
    _sig(lib.hipstr_hmm_trace_resident, C.c_int, [_BP, C.c_int32, _i32p, _i32p, _i32p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_void_p)])
    _sig(lib.hipstr_trace_dev_sizes, C.c_int, [C.c_void_p, _i32p, C.POINTER(C.c_int64)])
    _sig(lib.hipstr_trace_dev_fetch, C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(HipstrTraceOut)])
    _sig(lib.hipstr_trace_dev_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_trace_dev_from_host, C.c_int, [C.POINTER(HipstrTraceOut), C.c_int32, C.POINTER(C.c_void_p)])
    _sig(lib.hipstr_assign_trace_stats_dev, C.c_int, [_PBP, _i32p, C.c_void_p] + [_i32p] * 9)


class TraceDev:
    """A hipstr_trace_dev_t handle; close() frees it."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h

    def sizes(self):
        """(n_req, totals[7]) of hipstr_trace_dev_sizes."""
        n = np.zeros(1, np.int32); tot = np.zeros(7, np.int64)
        if self.lib.hipstr_trace_dev_sizes(self.h, n.ctypes.data_as(_i32p), tot.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
            raise RuntimeError("hipstr_trace_dev_sizes failed: " + self.lib.hipstr_last_error().decode())
        return int(n[0]), tot

    def close(self):
        if self.h:
            self.lib.hipstr_trace_dev_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_trace_resident(lib, bptr, req_read, req_allele, hap_to_ref=None, req_seed=None, flags=0):
    """hipstr_hmm_trace_resident -> TraceDev.  Raises with hipstr_last_error() when the call fails (the handle it left must then be NULL)."""
    _trace_dev_sigs(lib)
    _alleles_sigs(lib)
    rr = np.ascontiguousarray(np.asarray(req_read, np.int32)); aa = np.ascontiguousarray(np.asarray(req_allele, np.int32))
    ss = None if req_seed is None else np.ascontiguousarray(np.asarray(req_seed, np.int32))
    h2r = None if hap_to_ref is None else (C.c_char_p * len(hap_to_ref))(*hap_to_ref)
    h = C.c_void_p(0xdead)           # (the call has to clear it on failure)
    rc = lib.hipstr_hmm_trace_resident(bptr, len(rr), _ptr(rr, _i32p), _ptr(aa, _i32p), _ptr(ss, _i32p), h2r, int(flags), C.byref(h))
    if rc != 0:
        assert not h.value, "hipstr_hmm_trace_resident failed and left a handle"
        raise RuntimeError("hipstr_hmm_trace_resident failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    assert h.value
    return TraceDev(lib, h.value)


def trace_dev_fetch(lib, td, fields=TRACE_F_ALL, cap=None, null_others=False):
    """hipstr_trace_dev_fetch -> the dict of run_trace(..., unpack=False): numpy arrays and string buffers, every byte TRACE_SENTINEL before
    the call.  cap: out->cap_chars (default: the largest pool, so everything fits); the buffers always hold the largest pool.  null_others:
    the arrays of the groups not chosen are passed as NULL (they are still in the dict, untouched).  Raises when the call fails, with the dict
    as the exception's `keep`."""
    _trace_dev_sigs(lib)
    n, tot = td.sizes()
    room = max(int(tot.max()), 1)
    o = HipstrTraceOut(); keep = {}
    for bit, arrays in TRACE_GROUPS.items():
        for nm, kind, pool in arrays:
            if kind == "chr":
                a = C.create_string_buffer(bytes([TRACE_SENTINEL]) * room, room)
                ptr = C.cast(a, C.c_char_p)
            else:
                m = {"f8": n, "i4": n, "off": (2 * n if pool == 2 else n) + 1, "i4p": room}[kind]
                a = np.frombuffer(bytes([TRACE_SENTINEL]) * (max(m, 1) * (8 if kind == "f8" else 4)), np.float64 if kind == "f8" else np.int32).copy()
                ptr = a.ctypes.data_as(_f64p if kind == "f8" else _i32p)
            keep[nm] = a
            if (fields & bit) or not null_others:
                setattr(o, nm, ptr)
    o.cap_chars = int(room if cap is None else cap)
    rc = lib.hipstr_trace_dev_fetch(td.h, int(fields), C.byref(o))
    if rc != 0:
        e = RuntimeError("hipstr_trace_dev_fetch failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
        e.keep = keep
        raise e
    return keep


def trace_dev_from_host(lib, trace, n_req):
    """hipstr_debug_trace_dev_from_host -> TraceDev.  trace: dict of hipstr_trace_out_t's arrays (integers: sequences; pools: bytes or a string
    buffer); what is missing or None is an absent array."""
    _trace_dev_sigs(lib)
    t = HipstrTraceOut(); keep = []
    for arrays in TRACE_GROUPS.values():
        for nm, kind, pool in arrays:
            v = trace.get(nm)
            if v is None:
                continue
            if kind == "chr":
                setattr(t, nm, v if isinstance(v, bytes) else C.cast(v, C.c_char_p)); keep.append(v)
            else:
                a = np.ascontiguousarray(np.asarray(v, np.float64 if kind == "f8" else np.int32)); keep.append(a)
                setattr(t, nm, a.ctypes.data_as(_f64p if kind == "f8" else _i32p))
    h = C.c_void_p(0xdead)
    rc = lib.hipstr_debug_trace_dev_from_host(C.byref(t), int(n_req), C.byref(h))
    if rc != 0:
        assert not h.value
        raise RuntimeError("hipstr_debug_trace_dev_from_host failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    return TraceDev(lib, h.value)


# ---- the ragged gather of resident records and the trace cache built on it (hipstr_trace_dev_gather, hipstr_trace_cache_*)
class HipstrTraceCacheStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_hits", "n_misses", "n_inserted", "n_segments", "n_live", "n_dead")]


def _trace_cache_sigs(lib):
    _trace_dev_sigs(lib)
    vpp = C.POINTER(C.c_void_p)
    _sig(lib.hipstr_trace_dev_gather, C.c_int, [C.c_int32, vpp, C.c_int32, _i32p, _i32p, vpp])
    _sig(lib.hipstr_trace_cache_create, C.c_void_p, [C.c_int32, _i32p, _i32p])
    _sig(lib.hipstr_trace_cache_round, C.c_int, [C.c_void_p, _BP, C.c_int32, _i32p, _i32p, _i32p, C.POINTER(C.c_char_p), _u8p, vpp, C.POINTER(HipstrTraceCacheStats)])
    _sig(lib.hipstr_trace_cache_remap, C.c_int, [C.c_void_p, _i32p, _i32p])
    _sig(lib.hipstr_trace_cache_clear, C.c_int, [C.c_void_p, _u8p])
    _sig(lib.hipstr_trace_cache_compact, C.c_int, [C.c_void_p])
    _sig(lib.hipstr_trace_cache_entries, C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p, _i32p])
    _sig(lib.hipstr_trace_cache_view, C.c_int, [C.c_void_p, vpp])
    _sig(lib.hipstr_trace_cache_stats, C.c_int, [C.c_void_p, C.POINTER(HipstrTraceCacheStats)])
    _sig(lib.hipstr_trace_cache_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_trace_cache_plan, C.c_int, [C.c_int64] * 4 + [C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_trace_gather_last, C.c_int, [_f64p])


def trace_dev_gather(lib, sources, out_src, out_idx, n_src=None, n_out=None):
    """hipstr_trace_dev_gather -> TraceDev.  sources: TraceDev objects (None: a NULL source).  Raises with hipstr_last_error() when the call
    refuses (the handle it left must then be NULL).  n_src / n_out: counts other than the lists' lengths (the refusals)."""
    _trace_cache_sigs(lib)
    hs = (C.c_void_p * max(len(sources), 1))(*[None if s is None else s.h for s in sources])
    os_ = np.ascontiguousarray(np.asarray(out_src, np.int32)); oi = np.ascontiguousarray(np.asarray(out_idx, np.int32))
    h = C.c_void_p(0xdead)
    rc = lib.hipstr_trace_dev_gather(len(sources) if n_src is None else n_src, hs, len(os_) if n_out is None else n_out, _ptr(os_, _i32p), _ptr(oi, _i32p), C.byref(h))
    if rc != 0:
        assert not h.value, "hipstr_trace_dev_gather failed and left a handle"
        raise RuntimeError("hipstr_trace_dev_gather failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    assert h.value
    return TraceDev(lib, h.value)


def trace_gather_last(lib):
    """hipstr_debug_trace_gather_last of the calling thread as a dict."""
    _trace_cache_sigs(lib)
    o = np.zeros(4)
    assert lib.hipstr_debug_trace_gather_last(o.ctypes.data_as(_f64p)) == 0
    return dict(kernel_ms=float(o[0]), bytes_up=int(o[1]), bytes_home=int(o[2]), n_out=int(o[3]))


def trace_cache_plan(lib, n_out=0, n_live=0, n_dead=0, n_segments=0):
    """hipstr_debug_trace_cache_plan (host only) as a dict."""
    _trace_cache_sigs(lib)
    o = np.zeros(12, np.int64)
    if lib.hipstr_debug_trace_cache_plan(int(n_out), int(n_live), int(n_dead), int(n_segments), o.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise RuntimeError("hipstr_debug_trace_cache_plan failed: " + lib.hipstr_last_error().decode())
    keys = ("len_workgroups", "scan_steps", "scan_steps_flank", "copy_workgroups", "pieces", "compact", "min_dead", "max_segments", "len_threads", "wave",
            "totals_bytes", "pool_fits")
    return {k: int(v) for k, v in zip(keys, o)}


class TraceCache:
    """hipstr_trace_cache_*: SeqStutterGenotyper's trace_cache_ for a batch of loci (include/hipstr_hmm.h).  Every call raises with
    hipstr_last_error() when the library refuses it; `rc` is the last return code."""

    def __init__(self, lib, pool_off, n_alleles, n_loci=None):
        _trace_cache_sigs(lib)
        self.lib = lib; self.h = None; self.rc = 0
        po = None if pool_off is None else np.ascontiguousarray(np.asarray(pool_off, np.int32))
        na = None if n_alleles is None else np.ascontiguousarray(np.asarray(n_alleles, np.int32))
        self.h = lib.hipstr_trace_cache_create(len(na) if n_loci is None else n_loci, _ptr(po, _i32p), _ptr(na, _i32p))
        if not self.h:
            raise RuntimeError("hipstr_trace_cache_create failed: " + lib.hipstr_last_error().decode())

    def _check(self, rc, what):
        self.rc = rc
        if rc != 0:
            raise RuntimeError("%s failed rc=%d: %s" % (what, rc, self.lib.hipstr_last_error().decode()))

    @staticmethod
    def _stats(st):
        return {k: int(getattr(st, k)) for k, _ in HipstrTraceCacheStats._fields_}

    def round(self, bptr, req_read, req_allele, hap_to_ref=None, req_seed=None, locus_takes=None):
        """hipstr_trace_cache_round -> (TraceDev, stats dict)."""
        rr = np.ascontiguousarray(np.asarray(req_read, np.int32)); aa = np.ascontiguousarray(np.asarray(req_allele, np.int32))
        ss = None if req_seed is None else np.ascontiguousarray(np.asarray(req_seed, np.int32))
        lt = None if locus_takes is None else np.ascontiguousarray(np.asarray(locus_takes, np.uint8))
        h2r = None if hap_to_ref is None else (C.c_char_p * len(hap_to_ref))(*hap_to_ref)
        h = C.c_void_p(0xdead); st = HipstrTraceCacheStats()
        rc = self.lib.hipstr_trace_cache_round(self.h, bptr, len(rr), _ptr(rr, _i32p), _ptr(aa, _i32p), _ptr(ss, _i32p), h2r, _ptr(lt, _u8p), C.byref(h), C.byref(st))
        if rc != 0:
            assert not h.value, "hipstr_trace_cache_round failed and left a handle"
        self._check(rc, "hipstr_trace_cache_round")
        return TraceDev(self.lib, h.value), self._stats(st)

    def remap(self, new_n_alleles, allele_mapping):
        i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
        na = i32(new_n_alleles); am = i32(allele_mapping)
        self._check(self.lib.hipstr_trace_cache_remap(self.h, _ptr(na, _i32p), _ptr(am, _i32p)), "hipstr_trace_cache_remap")

    def clear(self, locus=None):
        m = None if locus is None else np.ascontiguousarray(np.asarray(locus, np.uint8))
        self._check(self.lib.hipstr_trace_cache_clear(self.h, _ptr(m, _u8p)), "hipstr_trace_cache_clear")

    def compact(self):
        self._check(self.lib.hipstr_trace_cache_compact(self.h), "hipstr_trace_cache_compact")

    def entries(self, cap=None):
        """(ent_read, ent_allele), sorted by (locus, pool, haplotype).  cap: the capacity handed to the call (default: what it needs)."""
        n = np.zeros(1, np.int32)
        if cap is None:
            rc = self.lib.hipstr_trace_cache_entries(self.h, 0, n.ctypes.data_as(_i32p), None, None)
            assert rc in (0, 3)
            cap = int(n[0])
        er = np.full(max(cap, 1), UNTOUCHED, np.int32); ea = np.full(max(cap, 1), UNTOUCHED, np.int32)
        rc = self.lib.hipstr_trace_cache_entries(self.h, int(cap), n.ctypes.data_as(_i32p), er.ctypes.data_as(_i32p), ea.ctypes.data_as(_i32p))
        self.n_entries = int(n[0])
        self._check(rc, "hipstr_trace_cache_entries")
        return er[:int(n[0])], ea[:int(n[0])]

    def view(self):
        h = C.c_void_p(0xdead)
        rc = self.lib.hipstr_trace_cache_view(self.h, C.byref(h))
        if rc != 0:
            assert not h.value
        self._check(rc, "hipstr_trace_cache_view")
        return TraceDev(self.lib, h.value)

    def stats(self):
        st = HipstrTraceCacheStats()
        self._check(self.lib.hipstr_trace_cache_stats(self.h, C.byref(st)), "hipstr_trace_cache_stats")
        return self._stats(st)

    def close(self):
        if self.h:
            self.lib.hipstr_trace_cache_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assign_trace_stats_dev(lib, pb, read_req, td, best_hap, hap_to_allele, allele_bp_diff, n_variants, region_start, region_stop):
    """hipstr_assign_trace_stats_dev -> (n_stutter[n_samp], n_flank_indel[n_samp], ml_bp[n_reads]); the shape of run_assign_trace_stats with a
    TraceDev in the trace's place."""
    _trace_dev_sigs(lib)
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))
    n_reads = int(pb.a["read_off"][-1]) if len(pb.a["read_off"]) else 0
    n_samp = int(pb.samp_off[-1])
    a = [i32(x) for x in (read_req, best_hap, hap_to_allele, allele_bp_diff, n_variants, region_start, region_stop)]
    ns = np.full(max(n_samp, 1), UNTOUCHED, np.int32); nf = np.full(max(n_samp, 1), UNTOUCHED, np.int32); ml = np.full(max(n_reads, 1), UNTOUCHED, np.int32)
    p = lambda x: x.ctypes.data_as(_i32p)
    rc = lib.hipstr_assign_trace_stats_dev(pb.ptr, p(a[0]), td.h, p(a[1]), p(a[2]), p(a[3]), p(a[4]), p(a[5]), p(a[6]), p(ns), p(nf), p(ml))
    if rc != 0:
        raise RuntimeError("hipstr_assign_trace_stats_dev failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    return ns[:n_samp], nf[:n_samp], ml[:n_reads]


# ---- the stutter model retrained from the tracebacks (hipstr_em_batch_from_traces, hipstr_em_train_dev)
class HipstrEmTraceRequest(C.Structure):
    _fields_ = [("pooled", C.POINTER(HipstrBatch)), ("seed", _i32p), ("read_req", _i32p), ("n_req", C.c_int32), ("req_read", _i32p),
                ("ref_allele", C.c_int32), ("max_iter", C.c_int32), ("min_ll_abs_change", C.c_double), ("min_ll_frac_change", C.c_double)]


class HipstrEmTraceOut(C.Structure):
    _fields_ = [("trained", _u8p), ("stutter", _f64p), ("n_iter", _i32p), ("final_ll", _f64p), ("em_read_off", _i32p), ("n_sizes", _i32p)]


class HipstrDebugEmInput(C.Structure):
    _fields_ = [("em_read_off", _i32p), ("num_bps", _i32p), ("sample_label", _i32p), ("obs", _i32p), ("log_p1", _f64p), ("log_p2", _f64p),
                ("size_off", _i32p), ("sizes", _i32p), ("log_freq", _f64p), ("route", _i32p)]


def _em_trace_sigs(lib):
    _sig(lib.hipstr_em_batch_from_traces, C.c_int, [_PBP, C.POINTER(HipstrEmTraceRequest), C.POINTER(HipstrTraceOut), _i32p, _i32p, _i32p, _f64p, _f64p])
    _sig(lib.hipstr_em_train_dev, C.c_int, [C.c_void_p, C.POINTER(HipstrEmTraceRequest), C.c_void_p, C.POINTER(HipstrEmTraceOut)])
    _sig(lib.hipstr_debug_em_input_plan, C.c_int, [C.c_int64] * 5 + [C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_em_input_fetch, C.c_int, [C.c_void_p, C.POINTER(HipstrEmTraceRequest), C.c_void_p, C.POINTER(HipstrDebugEmInput)])


def _em_trace_request(bptr, seed, read_req, req_read, ref_allele, max_iter, min_ll_abs_change, min_ll_frac_change):
    """(HipstrEmTraceRequest, what it points into)."""
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    keep = [i32(seed), i32(read_req), i32(req_read)]
    n_req = 0 if keep[2] is None else len(keep[2])
    pooled = None if bptr is None else (C.cast(bptr, C.POINTER(HipstrBatch)) if not hasattr(bptr, "_obj") else C.pointer(bptr._obj))
    rq = HipstrEmTraceRequest(pooled, _ptr(keep[0], _i32p), _ptr(keep[1], _i32p), n_req, _ptr(keep[2], _i32p), int(ref_allele), int(max_iter),
                              float(min_ll_abs_change), float(min_ll_frac_change))
    return rq, keep


def em_batch_from_traces(lib, pb, bptr, seed, read_req, req_read, trace, ref_allele=0, max_iter=100, min_ll_abs_change=0.01, min_ll_frac_change=0.001):
    """hipstr_em_batch_from_traces (host only) -> dict(read_off, sample_label, num_bps, log_p1, log_p2): the per-read arrays cut to the reads
    that entered.  pb: a PostBatch; bptr: the pooled batch; trace: dict with aln_start, aln_stop, stutter_size, str_seq_off (what is missing
    is passed as NULL).  Raises with hipstr_last_error() on a refusal; the exception's `outputs` are the arrays as the call left them
    (pre-filled with UNTOUCHED / NaN)."""
    _em_trace_sigs(lib)
    rq, keep = _em_trace_request(bptr, seed, read_req, req_read, ref_allele, max_iter, min_ll_abs_change, min_ll_frac_change)
    t = HipstrTraceOut()
    for nm in ("aln_start", "aln_stop", "stutter_size", "str_seq_off"):
        if trace is not None and trace.get(nm) is not None:
            a = np.ascontiguousarray(np.asarray(trace[nm], np.int32)); keep.append(a); setattr(t, nm, a.ctypes.data_as(_i32p))
    nl = int(pb.struct.n_loci); n = int(pb.a["read_off"][-1]) if nl else 0
    off = np.full(nl + 1, UNTOUCHED, np.int32); lab = np.full(max(n, 1), UNTOUCHED, np.int32); bps = np.full(max(n, 1), UNTOUCHED, np.int32)
    p1 = np.full(max(n, 1), np.nan); p2 = np.full(max(n, 1), np.nan)
    rc = lib.hipstr_em_batch_from_traces(pb.ptr, C.byref(rq), C.byref(t) if trace is not None else None, _ptr(off, _i32p), _ptr(lab, _i32p), _ptr(bps, _i32p),
                                         _ptr(p1, _f64p), _ptr(p2, _f64p))
    if rc != 0:
        e = RuntimeError("hipstr_em_batch_from_traces failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
        e.outputs = dict(read_off=off, sample_label=lab, num_bps=bps, log_p1=p1, log_p2=p2)
        raise e
    m = int(off[nl])
    return dict(read_off=off, sample_label=lab[:m], num_bps=bps[:m], log_p1=p1[:m], log_p2=p2[:m])


def em_train_dev(lib, pd, n_loci, bptr, seed, read_req, req_read, td, ref_allele=0, max_iter=100, min_ll_abs_change=0.01, min_ll_frac_change=0.001):
    """hipstr_em_train_dev -> (trained[n_loci] bool, stutter[n_loci, 6], n_iter, final_ll, em_read_off[n_loci+1], n_sizes[n_loci]) on a
    hipstr_post_dev_t handle and a TraceDev.  Raises with hipstr_last_error() on a refusal; the exception's `outputs` are the six arrays as
    the call left them (integers UNTOUCHED, doubles NaN, trained 0xAA)."""
    _em_trace_sigs(lib)
    rq, keep = _em_trace_request(bptr, seed, read_req, req_read, ref_allele, max_iter, min_ll_abs_change, min_ll_frac_change)
    nl = int(n_loci)
    trained = np.full(max(nl, 1), 0xAA, np.uint8); st = np.full(max(6 * nl, 6), np.nan); it = np.full(max(nl, 1), UNTOUCHED, np.int32)
    ll = np.full(max(nl, 1), np.nan); off = np.full(nl + 1, UNTOUCHED, np.int32); ns = np.full(max(nl, 1), UNTOUCHED, np.int32)
    o = HipstrEmTraceOut(_ptr(trained, _u8p), _ptr(st, _f64p), _ptr(it, _i32p), _ptr(ll, _f64p), _ptr(off, _i32p), _ptr(ns, _i32p))
    rc = lib.hipstr_em_train_dev(pd, C.byref(rq), None if td is None else td.h, C.byref(o))
    if rc != 0:
        e = RuntimeError("hipstr_em_train_dev failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
        e.outputs = dict(trained=trained, stutter=st, n_iter=it, final_ll=ll, em_read_off=off, n_sizes=ns)
        raise e
    return trained[:nl].astype(bool), st[:6 * nl].reshape(-1, 6), it[:nl], ll[:nl], off, ns[:nl]


def em_input_plan(lib, n_runs, run_reads, lo, hi, n_sizes):
    """hipstr_debug_em_input_plan (host only) as a dict: the decisions of hipstr_amd/csrc/em_input_layout.h and its compiled limits."""
    _em_trace_sigs(lib)
    out = np.zeros(12, np.int64)
    if lib.hipstr_debug_em_input_plan(int(n_runs), int(run_reads), int(lo), int(hi), int(n_sizes), out.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise RuntimeError("hipstr_debug_em_input_plan failed: " + lib.hipstr_last_error().decode())
    return dict(run_steps=int(out[0]), last_step=int(out[1]), run_workgroups=int(out[2]), scan_chunks=int(out[3]), scan_last_chunk=int(out[4]),
                device=bool(out[5]), bitmap_words=int(out[6]), device_priors=bool(out[7]),
                thresholds=dict(HS_EMI_THREADS=int(out[8]), HS_EMI_WAVE=int(out[9]), HS_EMI_SCAN_CHUNK=int(out[10]), HS_EMI_SPAN_LIMIT=int(out[11])))


def em_input_fetch(lib, pd, n_loci, n_reads, bptr, seed, read_req, req_read, td, ref_allele=0):
    """hipstr_debug_em_input_fetch -> dict(route ("device" / "host"), read_off, num_bps, sample_label, obs, log_p1, log_p2, size_off, sizes,
    log_freq): what hipstr_em_train_dev prepares before the EM loop."""
    _em_trace_sigs(lib)
    rq, keep = _em_trace_request(bptr, seed, read_req, req_read, ref_allele, 100, 0.01, 0.001)
    nl, n = int(n_loci), int(n_reads)
    off = np.zeros(nl + 1, np.int32); soff = np.zeros(nl + 1, np.int32); route = np.zeros(1, np.int32)
    ia = [np.zeros(max(n, 1), np.int32) for _ in range(3)]; fa = [np.zeros(max(n, 1)) for _ in range(2)]
    sizes = np.zeros(n + nl + 1, np.int32); freq = np.zeros(n + nl + 1)
    o = HipstrDebugEmInput(_ptr(off, _i32p), _ptr(ia[0], _i32p), _ptr(ia[1], _i32p), _ptr(ia[2], _i32p), _ptr(fa[0], _f64p), _ptr(fa[1], _f64p),
                           _ptr(soff, _i32p), _ptr(sizes, _i32p), _ptr(freq, _f64p), _ptr(route, _i32p))
    rc = lib.hipstr_debug_em_input_fetch(pd, C.byref(rq), td.h, C.byref(o))
    if rc != 0:
        raise RuntimeError("hipstr_debug_em_input_fetch failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    m = int(off[nl]); k = int(soff[nl])
    return dict(route="host" if route[0] else "device", read_off=off, num_bps=ia[0][:m], sample_label=ia[1][:m], obs=ia[2][:m], log_p1=fa[0][:m],
                log_p2=fa[1][:m], size_off=soff, sizes=sizes[:k], log_freq=freq[:k])


# ---- the flank reassembly (hipstr_flank_kmer_lengths, hipstr_flank_assemble, hipstr_flank_assemble_dev)
class HipstrFlankRequest(C.Structure):
    _fields_ = [("pooled", C.POINTER(HipstrBatch)), ("seed", _i32p), ("read_req", _i32p), ("n_req", C.c_int32), ("req_read", _i32p),
                ("pool_index", _i32p), ("sample_masked", _u8p), ("min_kmer", C.c_int32), ("max_kmer", C.c_int32), ("min_path_weight", C.c_int32),
                ("max_paths", C.c_int32), ("max_total_haplotypes", C.c_int32), ("max_flank_haplotypes", C.c_int32), ("min_flank_freq", C.c_double)]


class HipstrFlankOut(C.Structure):
    _fields_ = [("status", _i32p), ("new_n_haps", C.POINTER(C.c_int64)), ("opt_off", _i32p), ("opt_seq_off", _i32p), ("opt_seq", C.c_char_p),
                ("opt_n_samples", _i32p), ("sample_status", _u8p), ("realign_sample", _u8p), ("realign_pool", _u8p), ("copy_read", _u8p),
                ("task_k", _i32p), ("task_n_paths", _i32p), ("path_weight", _i32p), ("path_seq_off", _i32p), ("path_seq", C.c_char_p),
                ("cap_opts", C.c_int32), ("cap_opt_chars", C.c_int32), ("cap_paths", C.c_int32), ("cap_path_chars", C.c_int32)]


FLANK_FILL = 0xAA            # what run_flank fills the byte outputs with before the call
FLANK_FLAGS = dict(edges=0x01, nodes=0x02, recs=0x04, reads=0x08, len=0x10, byte=0x20, k=0x40, pool=0x80, peel=0x100, param=0x200, range=0x400)      # HS_FLK_F_*


def _flank_sigs(lib):
    _sig(lib.hipstr_flank_kmer_lengths, C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p])
    _sig(lib.hipstr_flank_assemble, C.c_int, [_PBP, C.POINTER(HipstrFlankRequest), C.POINTER(HipstrTraceOut), C.POINTER(HipstrFlankOut)])
    _sig(lib.hipstr_flank_assemble_dev, C.c_int, [C.c_void_p, C.POINTER(HipstrFlankRequest), C.c_void_p, C.POINTER(HipstrFlankOut)])
    _sig(lib.hipstr_debug_flank_plan, C.c_int, [_PBP, C.POINTER(HipstrFlankRequest), C.POINTER(HipstrTraceOut), C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_flank_last, C.c_int, [C.POINTER(C.c_int64), _i32p, _i32p, C.c_int64])


def flank_kmer_lengths(lib, bptr, min_kmer=0, max_kmer=0):
    """hipstr_flank_kmer_lengths -> int32 [n_loci, 2] (-1 = too repetitive)."""
    _flank_sigs(lib)
    b = _batch_struct(bptr)
    out = np.full(max(2 * int(b.n_loci), 1), UNTOUCHED, np.int32)
    if lib.hipstr_flank_kmer_lengths(C.byref(b), int(min_kmer), int(max_kmer), _ptr(out, _i32p)) != 0:
        raise RuntimeError("hipstr_flank_kmer_lengths failed: " + lib.hipstr_last_error().decode())
    return out[:2 * int(b.n_loci)].reshape(-1, 2)


def _flank_request(bptr, seed, read_req, req_read, pool_index, sample_masked, kw):
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    keep = [i32(seed), i32(read_req), i32(req_read), i32(pool_index), None if sample_masked is None else np.ascontiguousarray(np.asarray(sample_masked, np.uint8))]
    n_req = 0 if keep[2] is None else len(keep[2])
    pooled = None if bptr is None else (C.cast(bptr, C.POINTER(HipstrBatch)) if not hasattr(bptr, "_obj") else C.pointer(bptr._obj))
    rq = HipstrFlankRequest(pooled, _ptr(keep[0], _i32p), _ptr(keep[1], _i32p), kw.pop("n_req", n_req), _ptr(keep[2], _i32p), _ptr(keep[3], _i32p), _ptr(keep[4], _u8p),
                            int(kw.pop("min_kmer", 0)), int(kw.pop("max_kmer", 0)), int(kw.pop("min_path_weight", 0)), int(kw.pop("max_paths", 0)),
                            int(kw.pop("max_total_haplotypes", 1000)), int(kw.pop("max_flank_haplotypes", 4)), float(kw.pop("min_flank_freq", 0.15)))
    assert not kw, kw
    return rq, keep


def _flank_trace(trace, keep):
    if trace is None:
        return None
    t = HipstrTraceOut()
    if trace.get("flank_seq_off") is not None:
        a = np.ascontiguousarray(np.asarray(trace["flank_seq_off"], np.int32)); keep.append(a); t.flank_seq_off = a.ctypes.data_as(_i32p)
    if trace.get("flank_seq") is not None:
        v = trace["flank_seq"]; keep.append(v)
        t.flank_seq = v if isinstance(v, bytes) else C.cast(v, C.c_char_p)
    return t


def run_flank(lib, pb, bptr, seed, read_req, req_read, pool_index, trace=None, td=None, pd=None, sample_masked=None, caps=None, want_paths=True,
              null_out=None, **kw):
    """hipstr_flank_assemble (trace: dict with flank_seq_off / flank_seq) or hipstr_flank_assemble_dev (td: a TraceDev; pd: a hipstr_post_dev_t
    handle, or None = pb is uploaded and freed here) -> dict: "rc" (0 or 3), "status", "new_n_haps", "opts" (per locus, per flank: list of
    (bytes, supporting samples)), "sample_status", "realign_sample", "realign_pool", "copy_read", "task_k", "task_n_paths", "paths" (per task:
    list of (weight, bytes)), "raw" (every output array as the call left it: integers UNTOUCHED, bytes FLANK_FILL before the call) and, after
    rc 3, "need" (the four cap_* fields).  pb: the PostBatch (its sizes are read on both routes); bptr: the pooled batch.  caps: dict of the
    four capacities (default: sized by a first call).  null_out: name of an output array to pass as NULL.  Other keywords: the request's
    parameters.  Raises with hipstr_last_error() on any other failure; the exception's `raw` holds the arrays."""
    _flank_sigs(lib)
    rq, keep = _flank_request(bptr, seed, read_req, req_read, pool_index, sample_masked, dict(kw))
    t = _flank_trace(trace, keep)
    nl = int(pb.struct.n_loci)
    n_reads = int(pb.a["read_off"][-1]) if nl else 0
    n_samp = int(pb.samp_off[-1])
    b = _batch_struct(bptr) if bptr is not None else None
    n_pooled = int(np.ctypeslib.as_array(b.read_off, shape=(int(b.n_loci) + 1,))[-1]) if (b is not None and int(b.n_loci) > 0 and b.read_off) else 0
    own = td is not None and pd is None
    if own:
        pd = lib.hipstr_post_upload(pb.ptr, None)
        if not pd:
            raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())

    def call(c):
        k = dict(status=np.full(max(nl, 1), UNTOUCHED, np.int32), new_n_haps=np.full(max(nl, 1), UNTOUCHED, np.int64), opt_off=np.full(2 * nl + 1, UNTOUCHED, np.int32),
                 opt_seq_off=np.full(c["opts"] + 1, UNTOUCHED, np.int32), opt_n_samples=np.full(max(c["opts"], 1), UNTOUCHED, np.int32),
                 sample_status=np.full(max(n_samp, 1), FLANK_FILL, np.uint8), realign_sample=np.full(max(n_samp, 1), FLANK_FILL, np.uint8),
                 realign_pool=np.full(max(n_pooled, 1), FLANK_FILL, np.uint8), copy_read=np.full(max(n_reads, 1), FLANK_FILL, np.uint8),
                 task_k=np.full(max(2 * n_samp, 1), UNTOUCHED, np.int32), task_n_paths=np.full(max(2 * n_samp, 1), UNTOUCHED, np.int32),
                 path_weight=np.full(max(c["paths"], 1), UNTOUCHED, np.int32), path_seq_off=np.full(c["paths"] + 1, UNTOUCHED, np.int32))
        oseq = C.create_string_buffer(max(c["opt_chars"], 1)); pseq = C.create_string_buffer(max(c["path_chars"], 1))
        o = HipstrFlankOut()
        for nm, a in k.items():
            if nm == null_out or (not want_paths and nm in ("task_k", "task_n_paths", "path_weight", "path_seq_off")):
                continue
            setattr(o, nm, a.ctypes.data_as(dict(new_n_haps=C.POINTER(C.c_int64)).get(nm, _u8p if a.dtype == np.uint8 else _i32p)))
        if null_out != "opt_seq":
            o.opt_seq = C.cast(oseq, C.c_char_p)
        if want_paths:
            o.path_seq = C.cast(pseq, C.c_char_p)
        o.cap_opts, o.cap_opt_chars, o.cap_paths, o.cap_path_chars = c["opts"], c["opt_chars"], c["paths"], c["path_chars"]
        rc = (lib.hipstr_flank_assemble(pb.ptr, C.byref(rq), None if t is None else C.byref(t), C.byref(o)) if td is None else
              lib.hipstr_flank_assemble_dev(pd, C.byref(rq), td.h if hasattr(td, "h") else td, C.byref(o)))
        k["opt_seq"] = oseq.raw; k["path_seq"] = pseq.raw
        return rc, k, dict(opts=int(o.cap_opts), opt_chars=int(o.cap_opt_chars), paths=int(o.cap_paths), path_chars=int(o.cap_path_chars))

    try:
        if caps is None:
            rc, k, need = call(dict(opts=0, opt_chars=0, paths=0, path_chars=0))
            if rc == 3:
                rc, k, need = call(need)
        else:
            rc, k, need = call(dict(caps))
    finally:
        if own:
            lib.hipstr_post_free(pd)
    if rc not in (0, 3):
        e = RuntimeError("%s failed rc=%d: %s" % ("hipstr_flank_assemble" if td is None else "hipstr_flank_assemble_dev", rc, lib.hipstr_last_error().decode()))
        e.raw = k
        raise e
    out = dict(rc=rc, raw=k, need=need, opt_off=k["opt_off"])
    if rc != 0:
        return out
    out.update(status=k["status"][:nl], new_n_haps=k["new_n_haps"][:nl], sample_status=k["sample_status"][:n_samp], realign_sample=k["realign_sample"][:n_samp],
               realign_pool=k["realign_pool"][:n_pooled], copy_read=k["copy_read"][:n_reads])
    oo, so = k["opt_off"], k["opt_seq_off"]
    flat = [(k["opt_seq"][so[i]:so[i + 1]], int(k["opt_n_samples"][i])) for i in range(int(oo[2 * nl]))]
    out["opts"] = [[flat[oo[2 * l + f]:oo[2 * l + f + 1]] for f in range(2)] for l in range(nl)]
    if want_paths:
        out["task_k"] = k["task_k"][:2 * n_samp]; out["task_n_paths"] = k["task_n_paths"][:2 * n_samp]
        po = k["path_seq_off"]; paths = []; at = 0
        for tsk in range(2 * n_samp):
            m = int(k["task_n_paths"][tsk])
            paths.append([(int(k["path_weight"][i]), k["path_seq"][po[i]:po[i + 1]]) for i in range(at, at + m)])
            at += m
        out["paths"] = paths
    return out


def flank_plan(lib, pb, bptr, seed, read_req, req_read, pool_index, trace, sample_masked=None, **kw):
    """hipstr_debug_flank_plan (host only) as a dict; "tasks" rows are lists in the order of "fields"."""
    _flank_sigs(lib)
    rq, keep = _flank_request(bptr, seed, read_req, req_read, pool_index, sample_masked, dict(kw))
    t = _flank_trace(trace, keep)
    return _plan_json(lib, "hipstr_debug_flank_plan", lambda buf, cap: lib.hipstr_debug_flank_plan(pb.ptr, C.byref(rq), C.byref(t), buf, cap))


def flank_last(lib, n_tasks=0):
    """hipstr_debug_flank_last -> dict(tasks, skipped, host_tasks, fetched_strings, bytes_up, bytes_down, flags[n_tasks], sizes[n_tasks, 4])."""
    _flank_sigs(lib)
    out = np.zeros(8, np.int64); fl = np.zeros(max(n_tasks, 1), np.int32); sz = np.zeros(max(4 * n_tasks, 4), np.int32)
    if lib.hipstr_debug_flank_last(out.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(fl, _i32p), _ptr(sz, _i32p), int(n_tasks)) != 0:
        raise RuntimeError("hipstr_debug_flank_last failed: " + lib.hipstr_last_error().decode())
    return dict(tasks=int(out[0]), skipped=int(out[1]), host_tasks=int(out[2]), fetched_strings=bool(out[3]), bytes_up=int(out[4]), bytes_down=int(out[5]),
                flags=fl[:n_tasks], sizes=sz[:4 * n_tasks].reshape(-1, 4))


# ---- the record's numeric fields (hipstr_bias_pvalues, hipstr_record_fields and their host forms)
class HipstrRecordRequest(C.Structure):
    _fields_ = [("n_variants", _i32p), ("hap_to_allele", _i32p), ("sample_reported", _u8p), ("sample_masked", _u8p),
                ("n_aligned", _i32p), ("n_snp", _i32p), ("n_stutter", _i32p), ("n_flank_indel", _i32p),
                ("uniq_one", _i32p), ("uniq_two", _i32p), ("rv_uniq_one", _i32p), ("rv_uniq_two", _i32p), ("max_flank_indel_frac", C.c_float)]


class HipstrRecordOut(C.Structure):
    _fields_ = [("status", _i32p), ("gt", _i32p), ("ab", _f64p), ("dab", _i32p), ("fs", _f64p), ("n_skip", _i32p), ("n_filt", _i32p), ("an", _i32p),
                ("dp", _i32p), ("dsnp", _i32p), ("dstutter", _i32p), ("dflankindel", _i32p), ("allele_count", _i32p)]


RECORD_PASS, RECORD_NO_READS, RECORD_MASKED, RECORD_FLANK_INDEL_FRAC, RECORD_NOT_REPORTED = 0, 1, 2, 3, -1
RECORD_NOT_APPLICABLE = 1.01
RECORD_TABLE_READS = 5000
RECORD_COUNTS = ("n_aligned", "n_snp", "n_stutter", "n_flank_indel", "uniq_one", "uniq_two", "rv_uniq_one", "rv_uniq_two")
RECORD_NAMES = ("hipstr_bias_pvalues", "hipstr_bias_pvalues_host", "hipstr_record_fields", "hipstr_record_fields_host")


def _record_sigs(lib):
    pv = [C.c_int64, _i32p, _i32p, _i32p, _i32p, _f64p, _f64p]
    _sig(lib.hipstr_bias_pvalues, C.c_int, pv)
    _sig(lib.hipstr_bias_pvalues_host, C.c_int, pv)
    _sig(lib.hipstr_record_fields, C.c_int, [C.c_void_p, C.POINTER(HipstrRecordRequest), C.POINTER(HipstrRecordOut)])
    _sig(lib.hipstr_record_fields_host, C.c_int, [_PBP, _i32p, C.POINTER(HipstrRecordRequest), C.POINTER(HipstrRecordOut)])
    _sig(lib.hipstr_debug_record_last, C.c_int, [C.POINTER(C.c_int64)])


def bias_pvalues(lib, uniq_one, uniq_two, rv_uniq_one, rv_uniq_two, host=False, n=None):
    """hipstr_bias_pvalues (host=True: hipstr_bias_pvalues_host) -> (ab, fs); what the call leaves untouched holds NaN.  An argument may be
    None (a null pointer); n defaults to the length of uniq_one."""
    _record_sigs(lib)
    a = [None if x is None else np.ascontiguousarray(np.asarray(x, np.int32)) for x in (uniq_one, uniq_two, rv_uniq_one, rv_uniq_two)]
    if n is None:
        n = len(a[0])
    ab = np.full(max(n, 1), np.nan); fs = np.full(max(n, 1), np.nan)
    fn = lib.hipstr_bias_pvalues_host if host else lib.hipstr_bias_pvalues
    rc = fn(int(n), *[_ptr(x, _i32p) for x in a], _ptr(ab, _f64p), _ptr(fs, _f64p))
    if rc != 0:
        raise RuntimeError("hipstr_bias_pvalues%s failed rc=%d: %s" % ("_host" if host else "", rc, lib.hipstr_last_error().decode()))
    return ab[:max(n, 0)], fs[:max(n, 0)]


def run_record_fields(lib, pb, n_variants, hap_to_allele, counts, map_gt=None, pd=None, sample_reported=None, sample_masked=None,
                      max_flank_indel_frac=0.0, null_out=None):
    """hipstr_record_fields_host (map_gt given: the host form on the PostBatch pb) or hipstr_record_fields (pd: a hipstr_post_dev_t handle
    after hipstr_post_launch; None = pb is uploaded, launched and freed here) -> dict of the output arrays.  counts: dict of the eight
    per-sample arrays of RECORD_COUNTS (a missing one is passed as NULL).  Integers the call leaves untouched hold UNTOUCHED, doubles NaN.
    Raises with hipstr_last_error() when the call is refused; the exception's `raw` holds the arrays."""
    _record_sigs(lib)
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    u8 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.uint8))
    nl = int(pb.struct.n_loci)
    n_samp = int(pb.samp_off[-1])
    keep = dict(n_variants=i32(n_variants), hap_to_allele=i32(hap_to_allele), sample_reported=u8(sample_reported), sample_masked=u8(sample_masked))
    for nm in RECORD_COUNTS:
        keep[nm] = i32(counts.get(nm))
    rq = HipstrRecordRequest(*([_ptr(keep[f], t) for f, t in HipstrRecordRequest._fields_[:-1]] + [float(max_flank_indel_frac)]))
    nv = int(np.sum(keep["n_variants"])) if keep["n_variants"] is not None else 0
    k = dict(status=np.full(max(n_samp, 1), UNTOUCHED, np.int32), gt=np.full(max(2 * n_samp, 1), UNTOUCHED, np.int32), ab=np.full(max(n_samp, 1), np.nan),
             dab=np.full(max(n_samp, 1), UNTOUCHED, np.int32), fs=np.full(max(n_samp, 1), np.nan), allele_count=np.full(max(nv, 1), UNTOUCHED, np.int32))
    for nm in ("n_skip", "n_filt", "an", "dp", "dsnp", "dstutter", "dflankindel"):
        k[nm] = np.full(max(nl, 1), UNTOUCHED, np.int32)
    o = HipstrRecordOut(*[None if f == null_out else k[f].ctypes.data_as(t) for f, t in HipstrRecordOut._fields_])
    if map_gt is not None:
        mg = i32(np.asarray(map_gt).reshape(-1))
        rc = lib.hipstr_record_fields_host(pb.ptr, _ptr(mg, _i32p), C.byref(rq), C.byref(o))
        what = "hipstr_record_fields_host"
    else:
        what = "hipstr_record_fields"
        own = pd is None
        if own:
            pd = lib.hipstr_post_upload(pb.ptr, None)
            if not pd:
                raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())
        try:
            if own and lib.hipstr_post_launch(pd, None) != 0:
                raise RuntimeError("hipstr_post_launch failed: " + lib.hipstr_last_error().decode())
            rc = lib.hipstr_record_fields(pd, C.byref(rq), C.byref(o))
        finally:
            if own:
                lib.hipstr_post_free(pd)
    if rc != 0:
        e = RuntimeError("%s failed rc=%d: %s" % (what, rc, lib.hipstr_last_error().decode()))
        e.raw = k
        raise e
    out = {nm: k[nm][:n_samp] for nm in ("status", "ab", "dab", "fs")}
    out["gt"] = k["gt"][:2 * n_samp].reshape(-1, 2)
    out["allele_count"] = k["allele_count"][:nv]
    for nm in ("n_skip", "n_filt", "an", "dp", "dsnp", "dstutter", "dflankindel"):
        out[nm] = k[nm][:nl]
    return out


def record_last(lib):
    """hipstr_debug_record_last -> dict(lanes, host_lanes, bytes_up, bytes_down)."""
    _record_sigs(lib)
    out = (C.c_int64 * 4)()
    assert lib.hipstr_debug_record_last(out) == 0
    return dict(lanes=int(out[0]), host_lanes=int(out[1]), bytes_up=int(out[2]), bytes_down=int(out[3]))


# ---- the record's alleles (hipstr_record_alleles and its host form)
class HipstrRecordAllelesRequest(C.Structure):
    _fields_ = [("region_start", _i32p), ("region_stop", _i32p), ("win_off", _i32p), ("window", C.c_char_p)]


class HipstrRecordAllelesOut(C.Structure):
    _fields_ = [("status", _i32p), ("pos", _i32p), ("left_trim", _i32p), ("right_trim", _i32p), ("allele_off", _i32p), ("alleles", C.c_void_p),
                ("cap_alleles", C.c_int64), ("allele_bp_diff", _i32p), ("old_to_new", _i32p), ("new_to_old", _i32p),
                ("lflank_off", _i32p), ("lflanks", C.c_void_p), ("cap_lflanks", C.c_int64), ("rflank_off", _i32p), ("rflanks", C.c_void_p), ("cap_rflanks", C.c_int64)]


ALLELES_DUPLICATE, ALLELES_OUTSIDE_WINDOW, ALLELES_FLANK_ASSERT, ALLELES_DEVICE_OPTIONS, ALLELES_WIN_PAD = 1, 2, 4, 256, 40
RECORD_ALLELES_NAMES = ("hipstr_record_alleles", "hipstr_record_alleles_host")


def _record_alleles_sigs(lib):
    a = [_BP, C.POINTER(HipstrRecordAllelesRequest), C.POINTER(HipstrRecordAllelesOut)]
    _sig(lib.hipstr_record_alleles, C.c_int, a)
    _sig(lib.hipstr_record_alleles_host, C.c_int, a)
    _sig(lib.hipstr_debug_record_alleles_last, C.c_int, [C.POINTER(C.c_int64)])


def alleles_window(chrom, region_start, region_stop):
    """window[i] = chrom[region_start - 40 + i] for the bytes that exist up to region_stop + 40 (bytes; positions below 0 hold '.')."""
    w0 = region_start - ALLELES_WIN_PAD
    return b"." * max(0, -w0) + chrom[max(0, w0):max(0, region_stop + ALLELES_WIN_PAD)]


def run_record_alleles(lib, loci, host=False, flanks=True, caps=None, null=()):
    """hipstr_record_alleles (host=True: the _host form).  loci: dicts with region_start, region_stop, window (bytes) and blocks = three
    (start, end, [option bytes]) -> list of dicts per locus (status, pos, left_trim, right_trim, alleles, bp_diff, old_to_new, new_to_old,
    lflanks, rflanks).  caps: (alleles, lflanks, rflanks) capacities, default the header's bounds.  null: output fields to pass as NULL."""
    _record_alleles_sigs(lib)
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))
    nl = len(loci)
    starts = []; ends = []; nopts = []; off = [0]; seq = b""
    for L in loci:
        for st, en, opts in L["blocks"]:
            starts.append(st); ends.append(en); nopts.append(len(opts))
            for o in opts:
                seq += o; off.append(len(seq))
    keep = dict(blk_start=i32(starts), blk_end=i32(ends), blk_nopts=i32(nopts), opt_off=i32(off), seq=seq,
                region_start=i32([L["region_start"] for L in loci]), region_stop=i32([L["region_stop"] for L in loci]),
                win_off=i32(np.concatenate([[0], np.cumsum([len(L["window"]) for L in loci])])), window=b"".join(L["window"] for L in loci))
    b = HipstrBatch(); b.n_loci = nl
    for f in ("blk_start", "blk_end", "blk_nopts", "opt_off"):
        setattr(b, f, _ptr(keep[f], _i32p))
    b.seq = keep["seq"]
    rq = HipstrRecordAllelesRequest(_ptr(keep["region_start"], _i32p), _ptr(keep["region_stop"], _i32p), _ptr(keep["win_off"], _i32p), keep["window"])
    V = [len(L["blocks"][1][2]) for L in loci]; nv = sum(V)
    n0 = sum(len(L["blocks"][0][2]) for L in loci); n2 = sum(len(L["blocks"][2][2]) for L in loci)
    bound = lambda k: sum(sum(len(o) for o in L["blocks"][k][2]) + len(L["blocks"][k][2]) * len(L["blocks"][1][2][0]) for L in loci if L["blocks"][1][2])
    if caps is None:
        caps = (sum(v * (max([len(o) for o in L["blocks"][1][2]] + [0]) + len(L["window"]) + 1) for v, L in zip(V, loci)), bound(0), bound(2))
    k = dict(status=np.full(max(nl, 1), UNTOUCHED, np.int32), pos=np.full(max(nl, 1), UNTOUCHED, np.int32), left_trim=np.full(max(nl, 1), UNTOUCHED, np.int32),
             right_trim=np.full(max(nl, 1), UNTOUCHED, np.int32), allele_off=np.full(nv + 1, UNTOUCHED, np.int32), alleles=np.full(max(caps[0], 1), 0xEE, np.uint8),
             allele_bp_diff=np.full(max(nv, 1), UNTOUCHED, np.int32), old_to_new=np.full(max(nv, 1), UNTOUCHED, np.int32), new_to_old=np.full(max(nv, 1), UNTOUCHED, np.int32),
             lflank_off=np.full(n0 + 1, UNTOUCHED, np.int32), lflanks=np.full(max(caps[1], 1), 0xEE, np.uint8),
             rflank_off=np.full(n2 + 1, UNTOUCHED, np.int32), rflanks=np.full(max(caps[2], 1), 0xEE, np.uint8))
    o = HipstrRecordAllelesOut()
    for f, t in HipstrRecordAllelesOut._fields_:
        if f.startswith("cap_"):
            setattr(o, f, int(caps[("cap_alleles", "cap_lflanks", "cap_rflanks").index(f)]))
        elif f in null or (not flanks and f in ("lflank_off", "lflanks", "rflank_off", "rflanks")):
            setattr(o, f, None)
        else:
            setattr(o, f, k[f].ctypes.data if t is C.c_void_p else k[f].ctypes.data_as(t))
    fn = lib.hipstr_record_alleles_host if host else lib.hipstr_record_alleles
    rc = fn(C.byref(b), C.byref(rq), C.byref(o))
    if rc != 0:
        e = RuntimeError("hipstr_record_alleles%s failed rc=%d: %s" % ("_host" if host else "", rc, lib.hipstr_last_error().decode()))
        e.raw = k
        raise e
    out = []; v = 0; a0 = 0; a2 = 0
    cut = lambda pool, offs, i: pool[offs[i]:offs[i + 1]].tobytes()
    for l, L in enumerate(loci):
        d = dict(status=int(k["status"][l]), pos=int(k["pos"][l]), left_trim=int(k["left_trim"][l]), right_trim=int(k["right_trim"][l]),
                 alleles=[cut(k["alleles"], k["allele_off"], v + i) for i in range(V[l])], bp_diff=k["allele_bp_diff"][v:v + V[l]].tolist(),
                 old_to_new=k["old_to_new"][v:v + V[l]].tolist(), new_to_old=k["new_to_old"][v:v + V[l]].tolist())
        if flanks:
            m0, m2 = len(L["blocks"][0][2]), len(L["blocks"][2][2])
            d["lflanks"] = [cut(k["lflanks"], k["lflank_off"], a0 + i) for i in range(m0)]
            d["rflanks"] = [cut(k["rflanks"], k["rflank_off"], a2 + i) for i in range(m2)]
            a0 += m0; a2 += m2
        v += V[l]
        out.append(d)
    return out


def record_alleles_last(lib):
    """hipstr_debug_record_alleles_last -> dict(loci, host_loci, bytes_up, bytes_down)."""
    _record_alleles_sigs(lib)
    out = (C.c_int64 * 4)()
    assert lib.hipstr_debug_record_alleles_last(out) == 0
    return dict(loci=int(out[0]), host_loci=int(out[1]), bytes_up=int(out[2]), bytes_down=int(out[3]))


# ---- the genotype outputs in the record's allele order (hipstr_post_extract_vcf)
class HipstrGtVcfOrder(C.Structure):
    _fields_ = [("new_to_old", _i32p), ("old_to_new", _i32p), ("allele_bp_diff", _i32p), ("allele_count", _i32p), ("bp_diffs", _i32p), ("ac", _i32p)]


def gt_offsets(pb, n_variants):
    """(gl_off, pgl_off): [n_samp+1] starts of every sample's piece, as hipstr_gt_offsets gives them."""
    nl = pb.struct.n_loci
    hap = pb.a["haploid"] if pb.a["haploid"] is not None else np.zeros(nl, np.uint8)
    gl_off = [0]; pgl_off = [0]
    for l in range(nl):
        V = int(n_variants[l])
        for _ in range(int(pb.a["n_samples"][l])):
            gl_off.append(gl_off[-1] + (V if hap[l] else V * (V + 1) // 2)); pgl_off.append(pgl_off[-1] + (V if hap[l] else V * V))
    return np.asarray(gl_off, np.int64), np.asarray(pgl_off, np.int64)


def run_post_extract_flat(lib, pb, n_variants, hap_to_allele, order=None, calc_gls=True, calc_pls=True, calc_phased_gls=True, pd=None,
                          allele_bp_diff=None, allele_count=None, null=(), room_for_unrequested=True):
    """hipstr_post_extract (order None) or hipstr_post_extract_vcf (order = (new_to_old, old_to_new), each [sum V]) on a launched run pd
    (None: pb is uploaded, launched and freed here) -> dict of the FLAT output arrays (gl_off / pgl_off say where a sample's piece lies);
    what the call leaves untouched holds UNTOUCHED / NaN.  With an order also bp_diffs / ac when their inputs are given.  null: names of
    the order's fields to pass as NULL.  room_for_unrequested=False: an array that is not requested gets one element (the timing tools)."""
    _sig(lib.hipstr_post_extract, C.c_int, [C.c_void_p, C.POINTER(HipstrGtRequest), C.POINTER(HipstrGtOut)])
    _sig(lib.hipstr_post_extract_vcf, C.c_int, [C.c_void_p, C.POINTER(HipstrGtRequest), C.POINTER(HipstrGtVcfOrder), C.POINTER(HipstrGtOut)])
    i32 = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, np.int32))
    S = int(pb.samp_off[-1])
    nv = i32(n_variants); h2a = i32(hap_to_allele)
    rq = HipstrGtRequest(_ptr(nv, _i32p), _ptr(h2a, _i32p), int(calc_gls), int(calc_pls), int(calc_phased_gls))
    gl_off, pgl_off = gt_offsets(pb, nv)
    k = dict(best_hap=np.full(max(2 * S, 2), UNTOUCHED, np.int32), best_gt=np.full(max(2 * S, 2), UNTOUCHED, np.int32))
    for nm in ("log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff"):
        k[nm] = np.full(max(S, 1), np.nan)
    room = lambda want, n: max(int(n), 1) if (want or room_for_unrequested) else 1
    k["gls"] = np.full(room(calc_gls, gl_off[-1]), np.nan); k["pls"] = np.full(room(calc_pls, gl_off[-1]), UNTOUCHED, np.int32)
    k["phased_gls"] = np.full(room(calc_phased_gls, pgl_off[-1]), np.nan)
    o = HipstrGtOut(*[k[f].ctypes.data_as(t) for f, t in HipstrGtOut._fields_])
    tot_v = int(nv.sum())
    keep = None
    if order is not None:
        keep = dict(new_to_old=i32(order[0]), old_to_new=i32(order[1]), allele_bp_diff=i32(allele_bp_diff), allele_count=i32(allele_count),
                    bp_diffs=np.full(max(tot_v, 1), UNTOUCHED, np.int32), ac=np.full(max(tot_v, 1), UNTOUCHED, np.int32))
        od = HipstrGtVcfOrder(*[None if f in null else _ptr(keep[f], t) for f, t in HipstrGtVcfOrder._fields_])
    own = pd is None
    if own:
        pd = lib.hipstr_post_upload(pb.ptr, None)
        if not pd:
            raise RuntimeError("hipstr_post_upload failed: " + lib.hipstr_last_error().decode())
    try:
        if own and lib.hipstr_post_launch(pd, None) != 0:
            raise RuntimeError("hipstr_post_launch failed: " + lib.hipstr_last_error().decode())
        rc = lib.hipstr_post_extract(pd, C.byref(rq), C.byref(o)) if order is None else lib.hipstr_post_extract_vcf(pd, C.byref(rq), C.byref(od), C.byref(o))
    finally:
        if own:
            lib.hipstr_post_free(pd)
    if rc != 0:
        e = RuntimeError("hipstr_post_extract%s failed rc=%d: %s" % ("" if order is None else "_vcf", rc, lib.hipstr_last_error().decode()))
        e.raw = dict(k, **({} if keep is None else dict(bp_diffs=keep["bp_diffs"], ac=keep["ac"])))
        raise e
    out = dict(best_hap=k["best_hap"][:2 * S].reshape(-1, 2), best_gt=k["best_gt"][:2 * S].reshape(-1, 2), gl_off=gl_off, pgl_off=pgl_off)
    for nm in ("log_phased_post", "log_unphased_post", "hap_log_phased_post", "hap_log_unphased_post", "gl_diff"):
        out[nm] = k[nm][:S]
    out["gls"] = k["gls"][:int(gl_off[-1])]; out["pls"] = k["pls"][:int(gl_off[-1])]; out["phased_gls"] = k["phased_gls"][:int(pgl_off[-1])]
    if keep is not None:
        out["bp_diffs"] = keep["bp_diffs"][:tot_v]; out["ac"] = keep["ac"][:tot_v]
    return out


# ---- the record's per-read sizes and per-sample histograms (hipstr_cigar_bp_diffs, hipstr_sample_histograms, hipstr_em_batch_from_bp_diffs)
class HipstrCigarRequest(C.Structure):
    _fields_ = [("n_loci", C.c_int32), ("read_off", _i32p), ("read_start", _i32p), ("cigar_off", _i32p), ("cigar_op", _u8p), ("cigar_len", _i32p),
                ("region_start", _i32p), ("region_stop", _i32p), ("pad", _i32p)]


CIGAR_DEVICE_RUNS = 4096
HISTOGRAM_DEVICE_READS = 1024
NO_ML_BP = -2 ** 31
RECORD_READS_NAMES = ("hipstr_cigar_bp_diffs", "hipstr_cigar_bp_diffs_host", "hipstr_sample_histograms", "hipstr_sample_histograms_host",
                      "hipstr_em_batch_from_bp_diffs")


def _record_reads_sigs(lib):
    cg = [C.POINTER(HipstrCigarRequest), _u8p, _i32p]
    _sig(lib.hipstr_cigar_bp_diffs, C.c_int, cg)
    _sig(lib.hipstr_cigar_bp_diffs_host, C.c_int, cg)
    hs = [_PBP, _i32p, C.c_int32, _i32p, _i32p, _i32p]
    _sig(lib.hipstr_sample_histograms, C.c_int, hs)
    _sig(lib.hipstr_sample_histograms_host, C.c_int, hs)
    _sig(lib.hipstr_em_batch_from_bp_diffs, C.c_int, [_PBP, _u8p, _i32p, _i32p, _i32p, C.c_int32, _i32p, _i32p, _i32p, _f64p, _f64p, _u8p])
    _sig(lib.hipstr_debug_record_reads_last, C.c_int, [C.POINTER(C.c_int64)])


def cigar_request(loci):
    """loci: per locus (region_start, region_stop, pad, reads) with reads = [(start, [(op letter, length), ...]), ...] -> dict of the
    request's arrays."""
    read_off = [0]; start = []; coff = [0]; ops = []; lens = []
    for _, _, _, reads in loci:
        for s, runs in reads:
            start.append(s)
            ops += [ord(o) for o, _ in runs]; lens += [n for _, n in runs]
            coff.append(len(ops))
        read_off.append(len(start))
    i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int64).astype(np.int32))
    return dict(n_loci=len(loci), read_off=i32(read_off), read_start=i32(start), cigar_off=i32(coff), cigar_op=np.asarray(ops, np.uint8), cigar_len=i32(lens),
                region_start=i32([l[0] for l in loci]), region_stop=i32([l[1] for l in loci]), pad=i32([l[2] for l in loci]))


def run_cigar_bp_diffs(lib, rq, host=False, null=()):
    """hipstr_cigar_bp_diffs (host=True: the _host form) on a dict of cigar_request's arrays -> (got, bp_diff); what the call leaves untouched
    holds 0xEE / UNTOUCHED.  null: names of the request's arrays to pass as NULL, or "got" / "bp_diff"."""
    _record_reads_sigs(lib)
    n = int(rq["read_off"][-1])
    got = np.full(max(n, 1), 0xEE, np.uint8); bp = np.full(max(n, 1), UNTOUCHED, np.int32)
    st = HipstrCigarRequest(int(rq["n_loci"]), *[None if f in null else _ptr(rq[f], t) for f, t in HipstrCigarRequest._fields_[1:]])
    fn = lib.hipstr_cigar_bp_diffs_host if host else lib.hipstr_cigar_bp_diffs
    rc = fn(C.byref(st), None if "got" in null else _ptr(got, _u8p), None if "bp_diff" in null else _ptr(bp, _i32p))
    if rc != 0:
        e = RuntimeError("hipstr_cigar_bp_diffs%s failed rc=%d: %s" % ("_host" if host else "", rc, lib.hipstr_last_error().decode()))
        e.raw = (got, bp)
        raise e
    return got[:n], bp[:n]


def run_sample_histograms(lib, pb, value, skip, host=False):
    """hipstr_sample_histograms (host=True: the _host form) on the sample layout of the PostBatch pb -> (pair_off, hist_value, hist_count),
    the two pair arrays cut to pair_off[-1]; raw holds the whole buffers (UNTOUCHED where the call wrote nothing)."""
    _record_reads_sigs(lib)
    n = int(pb.struct.read_off[int(pb.struct.n_loci)]) if pb.struct.n_loci else 0
    ns = int(pb.samp_off[-1])
    v = None if value is None else np.ascontiguousarray(np.asarray(value, np.int32))
    po = np.full(ns + 1, UNTOUCHED, np.int32); hv = np.full(max(n, 1), UNTOUCHED, np.int32); hc = np.full(max(n, 1), UNTOUCHED, np.int32)
    fn = lib.hipstr_sample_histograms_host if host else lib.hipstr_sample_histograms
    rc = fn(pb.ptr, _ptr(v, _i32p), int(skip), _ptr(po, _i32p), _ptr(hv, _i32p), _ptr(hc, _i32p))
    if rc != 0:
        e = RuntimeError("hipstr_sample_histograms%s failed rc=%d: %s" % ("_host" if host else "", rc, lib.hipstr_last_error().decode()))
        e.raw = (po, hv, hc)
        raise e
    assert np.all(hv[po[-1]:] == UNTOUCHED) and np.all(hc[po[-1]:] == UNTOUCHED), "written behind the last pair"
    return po, hv[:po[-1]], hc[:po[-1]]


def em_batch_from_bp_diffs(lib, pb, got, bp_diff, region_start, region_stop, min_total_reads):
    """hipstr_em_batch_from_bp_diffs -> dict(read_off, sample_label, num_bps, log_p1, log_p2, too_few)."""
    _record_reads_sigs(lib)
    nl = int(pb.struct.n_loci)
    n = int(pb.struct.read_off[nl]) if nl else 0
    g = np.ascontiguousarray(np.asarray(got, np.uint8)); b = np.ascontiguousarray(np.asarray(bp_diff, np.int32))
    rs = np.ascontiguousarray(np.asarray(region_start, np.int32)); re_ = np.ascontiguousarray(np.asarray(region_stop, np.int32))
    ro = np.full(nl + 1, UNTOUCHED, np.int32); sl = np.full(max(n, 1), UNTOUCHED, np.int32); nb = np.full(max(n, 1), UNTOUCHED, np.int32)
    p1 = np.full(max(n, 1), np.nan); p2 = np.full(max(n, 1), np.nan); few = np.full(max(nl, 1), 0xEE, np.uint8)
    rc = lib.hipstr_em_batch_from_bp_diffs(pb.ptr, _ptr(g, _u8p), _ptr(b, _i32p), _ptr(rs, _i32p), _ptr(re_, _i32p), int(min_total_reads),
                                           _ptr(ro, _i32p), _ptr(sl, _i32p), _ptr(nb, _i32p), _ptr(p1, _f64p), _ptr(p2, _f64p), _ptr(few, _u8p))
    if rc != 0:
        raise RuntimeError("hipstr_em_batch_from_bp_diffs failed rc=%d: %s" % (rc, lib.hipstr_last_error().decode()))
    m = int(ro[-1])
    return dict(read_off=ro, sample_label=sl[:m], num_bps=nb[:m], log_p1=p1[:m], log_p2=p2[:m], too_few=few[:nl])


def record_reads_last(lib):
    """hipstr_debug_record_reads_last -> dict(items, host_items, bytes_up, bytes_down)."""
    _record_reads_sigs(lib)
    out = (C.c_int64 * 4)()
    assert lib.hipstr_debug_record_reads_last(out) == 0
    return dict(items=int(out[0]), host_items=int(out[1]), bytes_up=int(out[2]), bytes_down=int(out[3]))


class HipstrPoolOut(C.Structure):
    _fields_ = [("pool_index", _i32p), ("n_pools", _i32p), ("pool_off", _i32p), ("pool_rep", _i32p), ("pool_size", _i32p),
                ("pool_qual_off", _i32p), ("pool_quals", C.POINTER(C.c_char))]


POOL_ON_HOST = 1        # HIPSTR_POOL_ON_HOST
POOL_ROUTES = ("device", "host", "copy", "net", "radix")
POOL_LAST = ("device_loci", "host_loci", "collision_loci", "pools_copy", "pools_net", "pools_radix", "chunks", "reads_uploaded")
POOL_FILL = -7          # what run_pool fills the integer outputs with before the call (qualities: 0x5A)
POOL_FIELDS = ("pool_index", "n_pools", "pool_off", "pool_rep", "pool_size", "pool_qual_off", "pool_quals")


def _pool_sigs(lib):
    _sig(lib.hipstr_pool_reads, C.c_int, [_BP, C.POINTER(HipstrPoolOut)])
    _sig(lib.hipstr_pool_reads_host, C.c_int, [_BP, C.POINTER(HipstrPoolOut)])
    _sig(lib.hipstr_pool_batch, C.c_void_p, [_BP, C.c_uint32])
    _sig(lib.hipstr_pooled_batch_batch, _BP, [C.c_void_p])
    _sig(lib.hipstr_pooled_batch_pool_index, _i32p, [C.c_void_p])
    _sig(lib.hipstr_pooled_batch_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_pool_plan, C.c_int, [_BP, C.c_double, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_pool_last, C.c_int, [C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_pool_last_timing, C.c_int, [_f64p])


def _batch_struct(bptr):
    return bptr.contents if hasattr(bptr, "contents") else (bptr._obj if hasattr(bptr, "_obj") else bptr)


def run_pool(lib, bptr, host=False):
    """hipstr_pool_reads (host=True: hipstr_pool_reads_host) on a batch of un-pooled reads: a dict of the seven output arrays at their full
    size — what the call leaves untouched still holds POOL_FILL / 0x5A."""
    b = _batch_struct(bptr)
    nl = b.n_loci
    n = int(b.read_off[nl]) if nl else 0
    nb = int(b.base_off[n]) if n else 0
    a = dict(pool_index=np.full(n, POOL_FILL, np.int32), n_pools=np.full(nl, POOL_FILL, np.int32), pool_off=np.full(nl + 1, POOL_FILL, np.int32),
             pool_rep=np.full(n, POOL_FILL, np.int32), pool_size=np.full(n, POOL_FILL, np.int32), pool_qual_off=np.full(n + 1, POOL_FILL, np.int32),
             pool_quals=np.full(nb + 1, 0x5A, np.uint8))
    o = HipstrPoolOut(*[a[k].ctypes.data_as(_i32p) for k in POOL_FIELDS[:6]], a["pool_quals"].ctypes.data_as(C.POINTER(C.c_char)))
    rc = (lib.hipstr_pool_reads_host if host else lib.hipstr_pool_reads)(bptr, C.byref(o))
    if rc != 0:
        raise RuntimeError("hipstr_pool_reads%s failed: %s" % ("_host" if host else "", lib.hipstr_last_error().decode()))
    return a


def pool_plan(lib, bptr, ws_mib=0.0):
    """What hipstr_pool_reads would do with a batch (host only: hipstr_debug_pool_plan) as a dict."""
    return _plan_json(lib, "hipstr_debug_pool_plan", lambda buf, cap: lib.hipstr_debug_pool_plan(bptr, ws_mib, buf, cap))


def pool_last(lib):
    """hipstr_debug_pool_last as a dict keyed by POOL_LAST."""
    out = (C.c_int64 * 8)()
    assert lib.hipstr_debug_pool_last(out) == 0
    return dict(zip(POOL_LAST, [int(x) for x in out]))


def pool_last_timing(lib):
    out = (C.c_double * 4)()
    assert lib.hipstr_debug_pool_last_timing(out) == 0
    return dict(kernel_ms=out[0], bytes_up=out[1], bytes_down=out[2], stage_s=out[3])


def batch_arrays(ptr):
    """The arrays of a hipstr_batch_t the library returned (a pointer) as numpy copies (bytes arrays without their closing NUL)."""
    p = ptr.contents; nl = p.n_loci
    raw = lambda name, cnt: C.string_at(C.c_void_p.from_buffer(p, getattr(HipstrBatch, name).offset).value, cnt) if cnt else b""      # (a c_char_p field read as such stops at a NUL)
    i32 = lambda ptr, cnt: np.ctypeslib.as_array(ptr, shape=(cnt,)).copy() if cnt else np.zeros(0, np.int32)
    d = dict(blk_start=i32(p.blk_start, 3 * nl), blk_end=i32(p.blk_end, 3 * nl), blk_nopts=i32(p.blk_nopts, 3 * nl), period=i32(p.period, nl),
             stutter=np.ctypeslib.as_array(p.stutter, shape=(6 * nl,)).copy() if nl else np.zeros(0))
    nopt = int(d["blk_nopts"].sum())
    d["opt_off"] = i32(p.opt_off, nopt + 1); d["hap_off"] = i32(p.hap_off, nl + 1); d["read_off"] = i32(p.read_off, nl + 1)
    d["seq"] = np.frombuffer(raw("seq", int(d["opt_off"][-1])), np.uint8).copy()
    P = int(d["read_off"][-1])
    d["base_off"] = i32(p.base_off, P + 1); d["cigar_off"] = i32(p.cigar_off, P + 1); d["read_start"] = i32(p.read_start, P)
    nb, nc = int(d["base_off"][-1]), int(d["cigar_off"][-1])
    d["bases"] = np.frombuffer(raw("bases", nb), np.uint8).copy(); d["quals"] = np.frombuffer(raw("quals", nb), np.uint8).copy()
    d["cigar_op"] = np.frombuffer(raw("cigar_op", nc), np.uint8).copy(); d["cigar_len"] = i32(p.cigar_len, nc)
    A = int(d["hap_off"][-1])
    d["realign_hap"] = np.ctypeslib.as_array(p.realign_hap, shape=(A,)).copy() if p.realign_hap else np.zeros(0, np.uint8)
    d["realign_read"] = np.ctypeslib.as_array(p.realign_read, shape=(P,)).copy() if p.realign_read else np.zeros(0, np.uint8)
    return d


class PooledBatch:
    """hipstr_pool_batch: the pooled batch (ptr: a hipstr_batch_t for hipstr_hmm_upload) and the un-pooled reads' pool indices."""

    def __init__(self, lib, bptr, flags=0):
        self.lib = lib
        self.h = lib.hipstr_pool_batch(bptr, flags)
        if not self.h:
            raise RuntimeError("hipstr_pool_batch failed: " + lib.hipstr_last_error().decode())
        b = _batch_struct(bptr)
        self.n_unpooled = int(b.read_off[b.n_loci]) if b.n_loci else 0
        self.ptr = lib.hipstr_pooled_batch_batch(self.h)
        pi = lib.hipstr_pooled_batch_pool_index(self.h)
        self.pool_index = np.ctypeslib.as_array(pi, shape=(self.n_unpooled,)).copy() if self.n_unpooled else np.zeros(0, np.int32)

    def arrays(self):
        """The pooled batch's arrays as numpy copies (bytes arrays without their closing NUL)."""
        return batch_arrays(self.ptr)

    def close(self):
        if self.h:
            self.lib.hipstr_pooled_batch_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipstrHapgenRequest(C.Structure):
    _fields_ = [("region_start", _i32p), ("region_stop", _i32p), ("period", _i32p), ("chrom_len", C.POINTER(C.c_int64)), ("win_off", _i32p),
                ("window", C.POINTER(C.c_char)), ("n_samples", _i32p), ("sample_label", _i32p), ("read_stop", _i32p), ("use_read", _u8p), ("stutter", _f64p)]


class HipstrHapgenOut(C.Structure):
    _fields_ = [("status", _i32p), ("blk_start", _i32p), ("blk_end", _i32p), ("blk_nopts", _i32p), ("opt_off", _i32p), ("seq", C.POINTER(C.c_char)),
                ("n_spanning", _i32p), ("n_samples_spanning", _i32p), ("n_distinct", _i32p), ("left_trim", _i32p), ("right_trim", _i32p),
                ("min_aln_start", _i32p), ("max_aln_stop", _i32p), ("ext_off", _i32p), ("ext_len", _i32p), ("dist_len", _i32p), ("dist_rep", _i32p),
                ("dist_reads", _i32p), ("dist_strong", _i32p), ("dist_frac", _f64p)]


HAPGEN_ON_HOST = 1      # HIPSTR_HAPGEN_ON_HOST
HAPGEN_ROUTES = ("device", "host")
HAPGEN_LAST = ("device_loci", "host_loci", "collision_loci", "chunks", "reads_uploaded", "unused5", "unused6", "unused7")
HAPGEN_FILL = -7        # what run_hapgen fills the integer outputs with before the call (sequence bytes: 0x5A, dist_frac: -7.0)
HAPGEN_FIELDS = tuple(f for f, _ in HipstrHapgenOut._fields_)
HAPGEN_OPTIONAL = ("ext_off", "ext_len", "dist_len", "dist_rep", "dist_reads", "dist_strong", "dist_frac")
HAPGEN_STATUS = ("", "Haplotype blocks are too near to the chromosome ends", "No spanning alignments")


def _hapgen_sigs(lib):
    RQ, OUT = C.POINTER(HipstrHapgenRequest), C.POINTER(HipstrHapgenOut)
    _sig(lib.hipstr_hapgen, C.c_int, [_BP, RQ, OUT])
    _sig(lib.hipstr_hapgen_host, C.c_int, [_BP, RQ, OUT])
    _sig(lib.hipstr_hapgen_status_message, C.c_char_p, [C.c_int32])
    _sig(lib.hipstr_hapgen_batch, C.c_void_p, [_BP, RQ, C.c_uint32])
    _sig(lib.hipstr_hapgen_batch_batch, _BP, [C.c_void_p])
    _sig(lib.hipstr_hapgen_batch_locus, _i32p, [C.c_void_p])
    _sig(lib.hipstr_hapgen_batch_status, _i32p, [C.c_void_p])
    _sig(lib.hipstr_hapgen_batch_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_hapgen_plan, C.c_int, [_BP, RQ, C.c_double, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_hapgen_last, C.c_int, [C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_hapgen_last_timing, C.c_int, [_f64p])


class HapgenRequest:
    """A hipstr_hapgen_request_t over numpy arrays it keeps alive.  windows: one bytes object per locus; read_stop / use_read / stutter may be None."""

    def __init__(self, region_start, region_stop, period, chrom_len, windows, n_samples, sample_label, read_stop=None, use_read=None, stutter=None):
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, np.int32))
        win_off = np.concatenate([[0], np.cumsum([len(w) for w in windows])]).astype(np.int32)
        self.a = dict(region_start=i32(region_start), region_stop=i32(region_stop), period=i32(period),
                      chrom_len=np.ascontiguousarray(np.asarray(chrom_len, np.int64)), win_off=win_off,
                      window=np.frombuffer(b"".join(windows) + b"\0", np.uint8).copy(), n_samples=i32(n_samples),
                      sample_label=i32(sample_label if len(sample_label) else [0]), read_stop=None if read_stop is None else i32(read_stop),
                      use_read=None if use_read is None else np.ascontiguousarray(np.asarray(use_read, np.uint8)),
                      stutter=None if stutter is None else np.ascontiguousarray(np.asarray(stutter, np.float64)))
        a = self.a
        self.struct = HipstrHapgenRequest(_ptr(a["region_start"], _i32p), _ptr(a["region_stop"], _i32p), _ptr(a["period"], _i32p),
                                          a["chrom_len"].ctypes.data_as(C.POINTER(C.c_int64)), _ptr(a["win_off"], _i32p),
                                          a["window"].ctypes.data_as(C.POINTER(C.c_char)), _ptr(a["n_samples"], _i32p), _ptr(a["sample_label"], _i32p),
                                          _ptr(a["read_stop"], _i32p), _ptr(a["use_read"], _u8p), _ptr(a["stutter"], _f64p))

    @property
    def ptr(self):
        return C.byref(self.struct)


def hapgen_arrays(bptr, rq):
    """Room for every output of hipstr_hapgen on (bptr, rq), filled with HAPGEN_FILL / 0x5A / -7.0, and the struct that points into it."""
    b = _batch_struct(bptr)
    nl = b.n_loci
    n = int(b.read_off[nl]) if nl else 0
    nb = int(b.base_off[n]) if n else 0
    nw = int(rq.a["win_off"][-1]) if nl else 0
    size = dict(status=nl, blk_start=3 * nl, blk_end=3 * nl, blk_nopts=3 * nl, opt_off=3 * nl + n + 1, seq=nw + nb + 1)
    a = {}
    for k in HAPGEN_FIELDS:
        if k == "seq":
            a[k] = np.full(size[k], 0x5A, np.uint8)
        elif k == "dist_frac":
            a[k] = np.full(n + 1, float(HAPGEN_FILL), np.float64)
        else:
            a[k] = np.full(size.get(k, nl if k not in HAPGEN_OPTIONAL else n) + 1, HAPGEN_FILL, np.int32)
    return a


def hapgen_out_struct(a, skip=()):
    typ = dict(seq=C.POINTER(C.c_char), dist_frac=_f64p)
    return HipstrHapgenOut(*[None if k in skip else a[k].ctypes.data_as(typ.get(k, _i32p)) for k in HAPGEN_FIELDS])


def run_hapgen(lib, bptr, rq, host=False, skip=(), raw=False):
    """hipstr_hapgen (host=True: hipstr_hapgen_host): a dict of the outputs cut to what the call wrote (options: a list of lists of bytes per
    block).  skip: optional outputs passed as NULL.  raw=True: the arrays at their full size, what the call left untouched still HAPGEN_FILL."""
    a = hapgen_arrays(bptr, rq)
    o = hapgen_out_struct(a, skip)
    rc = (lib.hipstr_hapgen_host if host else lib.hipstr_hapgen)(bptr, rq.ptr, C.byref(o))
    if rc != 0:
        raise RuntimeError("hipstr_hapgen%s failed: %s" % ("_host" if host else "", lib.hipstr_last_error().decode()))
    if raw:
        return a
    b = _batch_struct(bptr)
    nl = b.n_loci
    n0 = int(b.read_off[0]) if nl else 0
    n = int(b.read_off[nl]) if nl else 0
    g = {k: a[k][:nl].copy() for k in ("status", "n_spanning", "n_samples_spanning", "n_distinct", "left_trim", "right_trim", "min_aln_start", "max_aln_stop")}
    for k in ("blk_start", "blk_end", "blk_nopts"):
        g[k] = a[k][:3 * nl].copy()
    nopt = int(g["blk_nopts"].sum())
    g["opt_off"] = a["opt_off"][:nopt + 1].copy()
    g["seq"] = a["seq"][:int(g["opt_off"][-1])].tobytes()
    nd = int(g["n_distinct"].sum())
    for k in HAPGEN_OPTIONAL:
        if k not in skip:
            g[k] = a[k][n0:n].copy() if k.startswith("ext") else a[k][:nd].copy()
    oo = g["opt_off"]
    g["options"] = [g["seq"][oo[i]:oo[i + 1]] for i in range(nopt)]
    g["untouched"] = all(np.all(a[k][m:] == HAPGEN_FILL) for k, m in (("status", nl), ("blk_nopts", 3 * nl), ("opt_off", nopt + 1))) and \
        bool(np.all(a["seq"][len(g["seq"]):] == 0x5A)) and all(k in skip or np.all(a[k][nd:] == HAPGEN_FILL) for k in HAPGEN_OPTIONAL if k.startswith("dist"))
    return g


def hapgen_plan(lib, bptr, rq, ws_mib=0.0):
    """What hipstr_hapgen would do with a request (host only: hipstr_debug_hapgen_plan) as a dict."""
    return _plan_json(lib, "hipstr_debug_hapgen_plan", lambda buf, cap: lib.hipstr_debug_hapgen_plan(bptr, rq.ptr, ws_mib, buf, cap))


def hapgen_last(lib):
    """hipstr_debug_hapgen_last as a dict keyed by HAPGEN_LAST."""
    out = (C.c_int64 * 8)()
    assert lib.hipstr_debug_hapgen_last(out) == 0
    return dict(zip(HAPGEN_LAST, [int(x) for x in out]))


def hapgen_last_timing(lib):
    out = (C.c_double * 4)()
    assert lib.hipstr_debug_hapgen_last_timing(out) == 0
    return dict(kernel_ms=out[0], bytes_up=out[1], bytes_down=out[2], stage_s=out[3])


class HapgenBatch:
    """hipstr_hapgen_batch: the un-pooled batch of the loci with status 0 (ptr: a hipstr_batch_t for hipstr_pool_batch), their original
    indices (locus) and the status of all loci."""

    def __init__(self, lib, bptr, rq, flags=0):
        self.lib = lib
        self.h = lib.hipstr_hapgen_batch(bptr, rq.ptr, flags)
        if not self.h:
            raise RuntimeError("hipstr_hapgen_batch failed: " + lib.hipstr_last_error().decode())
        nl = _batch_struct(bptr).n_loci
        self.ptr = lib.hipstr_hapgen_batch_batch(self.h)
        nk = self.ptr.contents.n_loci
        self.locus = np.ctypeslib.as_array(lib.hipstr_hapgen_batch_locus(self.h), shape=(nk,)).copy() if nk else np.zeros(0, np.int32)
        self.status = np.ctypeslib.as_array(lib.hipstr_hapgen_batch_status(self.h), shape=(nl,)).copy() if nl else np.zeros(0, np.int32)

    def arrays(self):
        return batch_arrays(self.ptr)

    def close(self):
        if self.h:
            self.lib.hipstr_hapgen_batch_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def census_plan(lib, n_req, n_reads):
    """hipstr_debug_census_plan (host only) as a dict: the route of a locus of n_req requests and n_reads un-pooled reads and the compiled
    limits of hipstr_amd/csrc/census_layout.h."""
    _sig(lib.hipstr_debug_census_plan, C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64)])
    out = np.zeros(10, np.int64)
    if lib.hipstr_debug_census_plan(int(n_req), int(n_reads), out.ctypes.data_as(C.POINTER(C.c_int64))) != 0:
        raise RuntimeError("hipstr_debug_census_plan failed: " + lib.hipstr_last_error().decode())
    return dict(route=CENSUS_ROUTES[int(out[0])], ws_ints=int(out[1]), lanes=int(out[2]), loci_per_workgroup=int(out[3]), global_ints=int(out[4]),
                thresholds=dict(HS_CENSUS_WAVE_REQS=int(out[5]), HS_CENSUS_WAVE_READS=int(out[6]), HS_CENSUS_LDS_INTS=int(out[7]),
                                HS_CENSUS_THREADS=int(out[8]), HS_CENSUS_REQ_INTS=int(out[9])))


TRACE_ASSEMBLE_DEVICE = 1      # HIPSTR_TRACE_ASSEMBLE_DEVICE


def run_trace(lib, prefix, bptr, req_read, req_allele, hap_to_ref=None, cap=1 << 16, timing=None, unpack=True, req_seed=None, flags=None):
    """Call <prefix>trace on a one-locus batch; returns a list of dicts (one per request) with python-typed fields.
    hap_to_ref: list of bytes (one per allele) or None.  The reference probe (prefix 'ref_') always stitches.
    flags: None, or the flags of <prefix>trace_ex (0 = host replay, TRACE_ASSEMBLE_DEVICE), which is then the entry point called."""
    n = len(req_read)
    o = HipstrTraceOut(); keep = {}
    def i32(name, m):
        a = np.zeros(m, np.int32); keep[name] = a; setattr(o, name, a.ctypes.data_as(_i32p))
    def chars(name):
        a = C.create_string_buffer(cap); keep[name] = a; setattr(o, name, C.cast(a, C.c_char_p))
    keep["ll"] = np.zeros(max(n, 1)); o.ll = keep["ll"].ctypes.data_as(_f64p)
    for nm, m in (("max_index", n), ("hap_aln_off", n + 1), ("stutter_size", n), ("str_seq_off", n + 1), ("flank_seq_off", 2 * n + 1),
                  ("flank_ins", n), ("flank_del", n), ("indel_off", n + 1), ("indel_pos", cap), ("indel_size", cap), ("snp_off", n + 1),
                  ("snp_pos", cap), ("aln_start", n), ("aln_stop", n), ("cigar_off", n + 1), ("cigar_len", cap), ("aln_str_off", n + 1)):
        i32(nm, max(m, 1))
    for nm in ("hap_aln", "str_seq", "flank_seq", "snp_base", "cigar_op", "aln_str"):
        chars(nm)
    o.cap_chars = cap
    rr = np.ascontiguousarray(np.asarray(req_read, np.int32)); aa = np.ascontiguousarray(np.asarray(req_allele, np.int32))
    fn = getattr(lib, prefix + ("trace_ex" if flags is not None else ("trace" if req_seed is None else "trace_seeded")))
    import time
    h2r = None
    if hap_to_ref is not None and prefix != "ref_":
        h2r = (C.c_char_p * len(hap_to_ref))(*hap_to_ref)       # (marshalling of this wrapper, not the call: outside the timed part)
    t_call = time.perf_counter()
    extra, extra_t = [], []
    if req_seed is not None:        # trace_optimal_aln's seed_base argument (HapAligner.h:93)
        ss = np.ascontiguousarray(np.asarray(req_seed, np.int32)); keep["req_seed"] = ss
        extra, extra_t = [ss.ctypes.data_as(_i32p)], [_i32p]
    if flags is not None:
        _sig(fn, C.c_int, [_BP, C.c_int32, _i32p, _i32p, _i32p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(HipstrTraceOut)])
        rc = fn(bptr, n, rr.ctypes.data_as(_i32p), aa.ctypes.data_as(_i32p), extra[0] if extra else None, h2r, int(flags), C.byref(o))
    elif prefix == "ref_":
        _sig(fn, C.c_int, [_BP, C.c_int32, _i32p, _i32p] + extra_t + [C.POINTER(HipstrTraceOut)])
        rc = fn(bptr, n, rr.ctypes.data_as(_i32p), aa.ctypes.data_as(_i32p), *(extra + [C.byref(o)]))
    else:
        _sig(fn, C.c_int, [_BP, C.c_int32, _i32p, _i32p] + extra_t + [C.POINTER(C.c_char_p), C.POINTER(HipstrTraceOut)])
        rc = fn(bptr, n, rr.ctypes.data_as(_i32p), aa.ctypes.data_as(_i32p), *(extra + [h2r, C.byref(o)]))
    if timing is not None:
        timing["call_s"] = timing.get("call_s", 0.0) + time.perf_counter() - t_call
    if rc != 0:
        why = ""
        if prefix == "hipstr_hmm_":
            _sig(lib.hipstr_last_error, C.c_char_p, [])
            why = ": " + lib.hipstr_last_error().decode()
        raise RuntimeError("%strace failed rc=%d%s" % (prefix, rc, why))
    if not unpack:
        return keep
    return unpack_trace(keep, n)


def unpack_trace(keep, n):
    """The arrays and pools of run_trace(..., unpack=False) as run_trace's list of dicts, one per request."""
    raws = {nm: keep[nm].raw for nm in ("hap_aln", "str_seq", "flank_seq", "snp_base", "cigar_op", "aln_str")}     # .raw copies: once per pool
    def piece(pool, off, i):
        return raws[pool][keep[off][i]:keep[off][i + 1]].decode()
    out = []
    for q in range(n):
        out.append(dict(
            ll=float(keep["ll"][q]), max_index=int(keep["max_index"][q]), hap_aln=piece("hap_aln", "hap_aln_off", q),
            stutter_size=int(keep["stutter_size"][q]), str_seq=piece("str_seq", "str_seq_off", q),
            flank_left=piece("flank_seq", "flank_seq_off", 2 * q), flank_right=piece("flank_seq", "flank_seq_off", 2 * q + 1),
            flank_ins=int(keep["flank_ins"][q]), flank_del=int(keep["flank_del"][q]),
            indels=[(int(keep["indel_pos"][i]), int(keep["indel_size"][i])) for i in range(keep["indel_off"][q], keep["indel_off"][q + 1])],
            snps=[(int(keep["snp_pos"][i]), raws["snp_base"][i:i + 1].decode()) for i in range(keep["snp_off"][q], keep["snp_off"][q + 1])],
            aln_start=int(keep["aln_start"][q]), aln_stop=int(keep["aln_stop"][q]),
            cigar="".join("%d%s" % (keep["cigar_len"][i], raws["cigar_op"][i:i + 1].decode()) for i in range(keep["cigar_off"][q], keep["cigar_off"][q + 1])),
            aln_str=piece("aln_str", "aln_str_off", q)))
    return out


def ref_hap_aln_info(ref, bptr, n_alleles, cap=1 << 20):
    """Haplotype::get_aln_info() of every allele (list of bytes) from the compiled reference."""
    ref.ref_hap_aln_info.restype = C.c_int
    ref.ref_hap_aln_info.argtypes = [_BP, C.c_char_p, C.c_int, _i32p]
    buf = C.create_string_buffer(cap); offs = np.zeros(n_alleles + 1, np.int32)
    rc = ref.ref_hap_aln_info(bptr, buf, cap, offs.ctypes.data_as(_i32p))
    if rc != 0:
        raise RuntimeError("ref_hap_aln_info rc=%d" % rc)
    raw = buf.raw
    return [raw[offs[k]:offs[k + 1] - 1] for k in range(n_alleles)]


def hap_aln_info(lib, prefix, bptr, cap=1 << 22):
    """<prefix>hap_aln_info: Haplotype::get_aln_info() of every haplotype of every locus of a batch (list of bytes)."""
    b = bptr.contents if hasattr(bptr, "contents") else (bptr._obj if hasattr(bptr, "_obj") else bptr)
    n = int(np.ctypeslib.as_array(b.hap_off, shape=(b.n_loci + 1,))[-1])
    fn = getattr(lib, prefix + "hap_aln_info")
    _sig(fn, C.c_int, [_BP, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)])
    buf = C.create_string_buffer(cap); offs = np.zeros(n + 1, np.int64)
    rc = fn(bptr, buf, cap, offs.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        why = ""
        if prefix == "hipstr_":
            _sig(lib.hipstr_last_error, C.c_char_p, [])
            why = ": " + lib.hipstr_last_error().decode()
        raise RuntimeError("%shap_aln_info failed rc=%d%s" % (prefix, rc, why))
    raw = buf.raw[:int(offs[n])]          # .raw copies the whole buffer: take it once
    return [raw[offs[k]:offs[k + 1] - 1] for k in range(n)]


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def gray_num_combs(nopts):
    return int(nopts[0]) * int(nopts[1]) * int(nopts[2])


class Batch:
    """Host-side flat batch: numpy arrays + the ctypes struct that points into them."""

    def __init__(self):
        self.blk_start, self.blk_end, self.blk_nopts, self.period, self.stutter = [], [], [], [], []
        self.opt_off, self.seq = [0], bytearray()
        self.hap_off, self.realign_hap = [0], []
        self.read_off, self.base_off, self.bases, self.quals = [0], [0], bytearray(), bytearray()
        self.read_start, self.cigar_off, self.cigar_op, self.cigar_len, self.realign_read = [], [0], bytearray(), [], []
        self._use_hap_mask = False
        self._use_read_mask = False
        self.struct = None

    def add_locus(self, blocks, period, stutter, reads, realign_hap=None):
        """blocks: 3 tuples (start, end, [option sequences]); reads: list of dicts
        {seq, qual, start, cigar:[(op,len)...], realign:bool}."""
        assert len(blocks) == 3
        nopts = []
        for (start, end, opts) in blocks:
            self.blk_start.append(start); self.blk_end.append(end); self.blk_nopts.append(len(opts))
            nopts.append(len(opts))
            for o in opts:
                self.seq += o.encode()
                self.opt_off.append(len(self.seq))
        A = gray_num_combs(nopts)
        self.period.append(period)
        self.stutter += list(stutter)
        self.hap_off.append(self.hap_off[-1] + A)
        if realign_hap is None:
            self.realign_hap += [1] * A
        else:
            assert len(realign_hap) == A
            self._use_hap_mask = True
            self.realign_hap += [1 if x else 0 for x in realign_hap]
        for rd in reads:
            assert len(rd["seq"]) == len(rd["qual"])
            self.bases += rd["seq"].encode(); self.quals += rd["qual"].encode()
            self.base_off.append(len(self.bases))
            self.read_start.append(rd["start"])
            for (op, n) in rd["cigar"]:
                self.cigar_op += op.encode(); self.cigar_len.append(n)
            self.cigar_off.append(len(self.cigar_op))
            flag = rd.get("realign", True)
            if not flag:
                self._use_read_mask = True
            self.realign_read.append(1 if flag else 0)
        self.read_off.append(self.read_off[-1] + len(reads))
        return A

    def finalize(self):
        i32 = lambda x: np.ascontiguousarray(np.array(x, dtype=np.int32))
        a = self.arrays = dict(
            blk_start=i32(self.blk_start), blk_end=i32(self.blk_end), blk_nopts=i32(self.blk_nopts), period=i32(self.period),
            stutter=np.ascontiguousarray(np.array(self.stutter, dtype=np.float64)), opt_off=i32(self.opt_off),
            seq=bytes(self.seq) + b"\0", hap_off=i32(self.hap_off),
            realign_hap=np.array(self.realign_hap, dtype=np.uint8) if self._use_hap_mask else None,
            read_off=i32(self.read_off), base_off=i32(self.base_off), bases=bytes(self.bases) + b"\0", quals=bytes(self.quals) + b"\0",
            read_start=i32(self.read_start), cigar_off=i32(self.cigar_off), cigar_op=bytes(self.cigar_op) + b"\0",
            cigar_len=i32(self.cigar_len if self.cigar_len else [0]),
            realign_read=np.array(self.realign_read, dtype=np.uint8) if self._use_read_mask else None,
        )
        s = HipstrBatch()
        s.n_loci = len(self.period)
        for name in ("blk_start", "blk_end", "blk_nopts", "period", "opt_off", "hap_off", "read_off", "base_off", "read_start",
                     "cigar_off", "cigar_len"):
            setattr(s, name, _ptr(a[name], _i32p))
        s.stutter = _ptr(a["stutter"], _f64p)
        s.seq, s.bases, s.quals, s.cigar_op = a["seq"], a["bases"], a["quals"], a["cigar_op"]
        s.realign_hap = _ptr(a["realign_hap"], _u8p)
        s.realign_read = _ptr(a["realign_read"], _u8p)
        s._keepalive = a     # byref(struct) keeps the struct alive; the struct keeps the arrays alive
        self.struct = s
        return self

    @property
    def ptr(self):
        return C.byref(self.struct)


def batch_dims(bptr):
    """(n_reads, n_out, out_off[n_loci+1]) of a hipstr_batch_t given as ctypes pointer/byref/struct."""
    b = bptr.contents if hasattr(bptr, "contents") else (bptr._obj if hasattr(bptr, "_obj") else bptr)
    n = b.n_loci
    read_off = np.ctypeslib.as_array(b.read_off, shape=(n + 1,))
    hap_off = np.ctypeslib.as_array(b.hap_off, shape=(n + 1,))
    P = np.diff(read_off).astype(np.int64)
    A = np.diff(hap_off).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(P * A)])
    return int(read_off[-1]), int(out_off[-1]), out_off


class PostBatch:
    def __init__(self, n_alleles, n_samples, read_off, sample_label, log_p1, log_p2, read_weight, log_aln_probs, haploid=None, log_prior=None):
        i32 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.int32))
        f64 = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        self.a = dict(n_alleles=i32(n_alleles), n_samples=i32(n_samples), read_off=i32(read_off), sample_label=i32(sample_label),
                      log_p1=f64(log_p1), log_p2=f64(log_p2), read_weight=i32(read_weight),
                      log_aln_probs=None if log_aln_probs is None else f64(log_aln_probs),
                      haploid=None if haploid is None else np.ascontiguousarray(np.asarray(haploid, dtype=np.uint8)),
                      log_prior=None if log_prior is None else f64(log_prior))
        s = HipstrPostBatch()
        s.n_loci = len(self.a["n_alleles"])
        for name in ("n_alleles", "n_samples", "read_off", "sample_label", "read_weight"):
            setattr(s, name, _ptr(self.a[name], _i32p))
        s.log_p1 = _ptr(self.a["log_p1"], _f64p); s.log_p2 = _ptr(self.a["log_p2"], _f64p)
        s.log_aln_probs = _ptr(self.a["log_aln_probs"], _f64p)
        s.haploid = _ptr(self.a["haploid"], _u8p)
        s.log_prior = _ptr(self.a["log_prior"], _f64p)
        s._keepalive = self.a
        self.struct = s
        A = self.a["n_alleles"].astype(np.int64); S = self.a["n_samples"].astype(np.int64)
        self.post_off = np.concatenate([[0], np.cumsum(S * A * A)])
        self.samp_off = np.concatenate([[0], np.cumsum(S)])

    @property
    def ptr(self):
        return C.byref(self.struct)


# ----------------------------------------------------------------------------- loaders
def _sig(fn, restype, argtypes):
    """The signature of an entry point, written once.  The wrappers bind on use, so they come here before every call: a signature that is
    already in place is left alone — ctypes converts the arguments of a call through fn's argtypes, and another host thread may be in
    that call (tests/test_threads_gpu.py)."""
    argtypes = tuple(argtypes)
    have = fn.argtypes
    if have is None or tuple(have) != argtypes:
        fn.argtypes = argtypes
    if fn.restype is not restype:
        fn.restype = restype


_BP = C.POINTER(HipstrBatch)
_PBP = C.POINTER(HipstrPostBatch)


def _common_align_sigs(lib, prefix):
    _sig(getattr(lib, prefix + "process_reads"), C.c_int, [_BP, _f64p, _i32p])
    _sig(getattr(lib, prefix + "posteriors"), C.c_int, [_PBP, _f64p, _f64p, _i32p, _f64p])


_scalar_probes = {
    "int_log": (C.c_double, [C.c_int]),
    "transition": (C.c_double, [C.c_int, C.c_int]),
    "base_quality": (C.c_double, [C.c_int, C.c_int]),
    "stutter_pmf": (C.c_double, [_f64p, C.c_int, C.c_int, C.c_int]),
    "fast_lse_vec": (C.c_double, [_f64p, C.c_int]),
    "fast_lse2": (C.c_double, [C.c_double, C.c_double]),
    "log_sum_exp": (C.c_double, [_f64p, C.c_int]),
}


_u32p = C.POINTER(C.c_uint32)
_i64p = C.POINTER(C.c_int64)
# the float log-sum-exp primitives in bulk (hipstr_amd/csrc/float_lse.h): the same three signatures in the product (hipstr_debug_*, device
# and _host), the oracle (oracle_*) and the compiled reference (ref_*), bound by the helpers below on first use
_float_lse_probes = {
    "float_fn": [C.c_int, C.c_uint32, C.c_int64, _u32p],
    "fast_lse2": [_f64p, _f64p, _f64p, C.c_int64],
    "fast_lse_vec": [_f64p, _i64p, _f64p, C.c_int64],
}
FLOAT_FN = {"fasterexp": 0, "fasterlog": 1, "fastexp": 2, "fastlog": 3, "lse2_term": 4, "div_pow2": 5, "div_log": 6, "rcp_pow2": 7, "rcp_log": 8}


def _float_lse_fn(lib, name):
    """Entry point `name` of `lib` with its signature set — bound where it is used, not by the loaders: load_oracle() / load_ref() / load_hmm()
    go on working with a library that was built before these entries existed."""
    fn = getattr(lib, name)
    kind = next(k for k in _float_lse_probes if k in name)
    _sig(fn, C.c_int, _float_lse_probes[kind])
    return fn


def float_fn(lib, name, which, bits_lo, count):
    """The result bits (uint32 array) of function `which` (a FLOAT_FN name or number) at the `count` float bit patterns from bits_lo, from
    entry point `name` of `lib` (hipstr_debug_float_fn[_host], oracle_float_fn, ref_float_fn)."""
    out = np.empty(int(count), np.uint32)
    rc = _float_lse_fn(lib, name)(FLOAT_FN.get(which, which), int(bits_lo), int(count), out.ctypes.data_as(_u32p))
    assert rc == 0, (name, which, hex(bits_lo), count, lib.hipstr_last_error() if name.startswith("hipstr_") else rc)
    return out


def fast_lse2(lib, name, a, b):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b, np.float64); out = np.empty_like(a)
    assert a.shape == b.shape and _float_lse_fn(lib, name)(a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p), a.size) == 0, name
    return out


def fast_lse_vec(lib, name, rows):
    """fast_log_sum_exp(vector) of every row of `rows` (a list of 1-d arrays) from entry point `name` of `lib`."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    v = np.ascontiguousarray(np.concatenate(rows), np.float64); out = np.empty(len(rows), np.float64)
    assert _float_lse_fn(lib, name)(v.ctypes.data_as(_f64p), off.ctypes.data_as(_i64p), out.ctypes.data_as(_f64p), len(rows)) == 0, name
    return out


def load_oracle():
    """oracle/libhipstr_oracle.so — the C restatement.  TEST INFRASTRUCTURE: callers must be
    tests/, __graft_entry__.smoke() or bench.py's cpu_baseline leg."""
    lib = C.CDLL(ORACLE_LIB)
    _common_align_sigs(lib, "oracle_")
    _sig(lib.oracle_calc_seed_bases, C.c_int, [_BP, _i32p])
    _sig(lib.oracle_allele_options, C.c_int, [_i32p, C.c_int, _i32p])
    _sig(lib.oracle_debug_row_h, C.c_int, [_BP, C.c_int, _i32p, _i32p, C.c_int])
    for name, (rt, at) in _scalar_probes.items():
        _sig(getattr(lib, "oracle_" + name), rt, at)
    _sig(lib.oracle_set_cr_math, None, [C.c_int])
    return lib


class oracle_cr_math:
    """with capi.oracle_cr_math(oracle): ... — the oracle's posterior / genotype-call / EM stages evaluate exp and log with the correctly
    rounded functions of hipstr_amd/csrc/cr_math.h (what the device kernels use) instead of the host libm: an operation-for-operation CPU
    restatement of the device path.  Only for those stages: the alignment path's model tables stay the host libm's in the library too."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.lib.oracle_set_cr_math(1)
        return self.lib

    def __exit__(self, *a):
        self.lib.oracle_set_cr_math(0)
        return False


def load_ref():
    """oracle/_ref/libhipstr_ref.so — the real reference sources compiled by oracle/Makefile.
    genotyper.cpp leaves FastaReader/htslib symbols undefined (only get_vcf_header uses them), so
    the library is opened with lazy binding.  TEST INFRASTRUCTURE, same rule as load_oracle."""
    libc = C.CDLL(None)
    libc.dlopen.restype = C.c_void_p
    libc.dlopen.argtypes = [C.c_char_p, C.c_int]
    handle = libc.dlopen(REF_LIB.encode(), os.RTLD_LAZY)
    if not handle:
        raise OSError("cannot dlopen " + REF_LIB)
    lib = C.CDLL(REF_LIB, handle=handle)
    _common_align_sigs(lib, "ref_")
    _sig(lib.ref_hap_sequences, C.c_int, [_BP, C.c_int, C.c_char_p, C.c_int, _i32p])
    _sig(lib.ref_log_thresh, C.c_double, [])
    _sig(lib.ref_log_one_half, C.c_double, [])
    for name, (rt, at) in _scalar_probes.items():
        _sig(getattr(lib, "ref_" + name), rt, at)
    return lib


def have_ref():
    return os.path.exists(REF_LIB)


def load_synth():
    lib = C.CDLL(SYNTH_LIB)
    _sig(lib.synth_create, C.c_void_p, [C.c_int32] * 7 + [C.c_uint64, C.c_double])
    _sig(lib.synth_create_at, C.c_void_p, [C.c_int32] * 8 + [C.c_uint64, C.c_double])
    _sig(lib.synth_batch, _BP, [C.c_void_p])
    _sig(lib.synth_src_allele, _i32p, [C.c_void_p])
    _sig(lib.synth_free, None, [C.c_void_p])
    return lib


class SynthBatch:
    """Seeded synthetic loci (hipstr_amd/synth/synth.cpp).  .ptr is a hipstr_batch_t*."""

    def __init__(self, n_loci, reads_per_locus, n_str_alleles, read_len=150, flank_len=60, str_bp=40, n_flank_opts=1,
                 seed=20260928, mask_rate=0.0, first_locus=0):
        self.lib = load_synth()
        self.h = self.lib.synth_create_at(first_locus, n_loci, reads_per_locus, n_str_alleles, read_len, flank_len, str_bp, n_flank_opts, seed, mask_rate)
        self.ptr = self.lib.synth_batch(self.h)
        self.n_reads, self.n_out, self.out_off = batch_dims(self.ptr)
        self.n_loci = n_loci

    def src_allele(self):
        return np.ctypeslib.as_array(self.lib.synth_src_allele(self.h), shape=(self.n_reads,)).copy()

    def close(self):
        if self.h:
            self.lib.synth_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_hmm():
    """The product: hipstr_amd/csrc/libhipstr_hmm.so (HIP/gfx950).  Raises if it is missing —
    there is deliberately no CPU fallback."""
    if not os.path.exists(HMM_LIB):
        raise RuntimeError("libhipstr_hmm.so is not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(HMM_LIB)
    _sig(lib.hipstr_batch_out_offsets, C.c_int, [_BP, C.POINTER(C.c_int64)])
    _sig(lib.hipstr_hmm_init, C.c_int, [C.c_int])
    _sig(lib.hipstr_hmm_shutdown, None, [])
    _sig(lib.hipstr_hmm_trim, C.c_int64, [])
    _sig(lib.hipstr_hmm_upload, C.c_void_p, [_BP])
    _sig(lib.hipstr_hmm_free, None, [C.c_void_p])
    _sig(lib.hipstr_hmm_align, C.c_int, [C.c_void_p, C.c_void_p])
    _sig(lib.hipstr_hmm_align_timed, C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)])
    _sig(lib.hipstr_hmm_fetch, C.c_int, [C.c_void_p, _f64p, _i32p])
    _sig(lib.hipstr_hmm_dev_aln_probs, C.c_void_p, [C.c_void_p])
    _sig(lib.hipstr_hmm_process_reads, C.c_int, [_BP, _f64p, _i32p])
    _sig(lib.hipstr_hmm_process_reads_seeded, C.c_int, [_BP, _i32p, _f64p, _i32p])
    _sig(lib.hipstr_hmm_upload_seeded, C.c_void_p, [_BP, _i32p])
    _sig(lib.hipstr_calc_seed_bases, C.c_int, [_BP, _i32p])
    _sig(lib.hipstr_post_offsets, C.c_int, [_PBP, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    _sig(lib.hipstr_post_run, C.c_int, [_PBP, C.c_void_p, _f64p, _f64p, _i32p, _f64p])
    _sig(lib.hipstr_post_upload, C.c_void_p, [_PBP, C.c_void_p])
    _sig(lib.hipstr_post_launch, C.c_int, [C.c_void_p, C.c_void_p])
    _sig(lib.hipstr_post_fetch, C.c_int, [C.c_void_p, _f64p, _f64p, _i32p, _f64p])
    _sig(lib.hipstr_post_free, None, [C.c_void_p])
    _sig(lib.hipstr_hmm_profile, C.c_int, [C.c_void_p, C.c_int])
    _sig(lib.hipstr_hmm_profile_read, C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.c_int])
    _sig(lib.hipstr_hmm_workload, C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_rows, C.c_int, [_BP, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int])
    _sig(lib.hipstr_debug_prepare, C.c_int, [_BP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)])
    _sig(lib.hipstr_debug_str_groups, C.c_int, [_BP, _i32p, _i32p, _i32p, C.c_int, _i32p, C.c_int, _i32p])
    _sig(lib.hipstr_debug_simple_table, C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)])
    _sig(lib.hipstr_last_error, C.c_char_p, [])
    _sig(lib.hipstr_debug_driver_allocs, C.c_int64, [])
    _sig(lib.hipstr_locus_costs, C.c_int, [_BP, _f64p])
    _sig(lib.hipstr_debug_cr_math, C.c_int, [C.c_int, _f64p, _f64p, C.c_int64])
    _sig(lib.hipstr_debug_cache_get, C.c_void_p, [C.c_int64])
    _sig(lib.hipstr_debug_cache_put, None, [C.c_void_p])
    _sig(lib.hipstr_debug_cache_poison, C.c_int64, [C.c_int])
    _sig(lib.hipstr_debug_cache_stats, C.c_int, [C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_allele_kinds, C.c_int, [C.c_void_p, C.POINTER(C.c_int64)])
    _sig(lib.hipstr_debug_stream_create, C.c_void_p, [])
    _sig(lib.hipstr_debug_stream_destroy, None, [C.c_void_p])
    _sig(lib.hipstr_debug_fetch_table, C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64])
    _sig(lib.hipstr_debug_launch_plan, C.c_int, [_BP, C.c_double, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_trace_plan, C.c_int, [_BP, C.c_int32, _i32p, _i32p, _i32p, C.c_double, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_trace_assemble_plan, C.c_int, [_BP, C.c_int32, _i32p, _i32p, _i32p, C.POINTER(C.c_char_p), C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_nw_plan, C.c_int, [C.POINTER(HipstrNwBatch), C.c_double, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_post_plan, C.c_int, [_PBP, C.c_char_p, C.c_int])
    _sig(lib.hipstr_debug_em_plan, C.c_int, [C.POINTER(HipstrEmBatch), C.c_char_p, C.c_int])
    _sig(lib.hipstr_rm_create, C.c_void_p, [C.POINTER(HipstrReadLayout), _f64p, _i32p])
    _sig(lib.hipstr_rm_scatter, C.c_int, [C.c_void_p, C.c_void_p, _u8p])
    _sig(lib.hipstr_rm_remap, C.c_int, [C.c_void_p, _i32p, _i32p])
    _sig(lib.hipstr_rm_dev_log_aln_probs, C.c_void_p, [C.c_void_p])
    _sig(lib.hipstr_rm_fetch, C.c_int, [C.c_void_p, _f64p, _i32p])
    _sig(lib.hipstr_rm_free, None, [C.c_void_p])
    _sig(lib.hipstr_debug_rm_plan, C.c_int, [C.c_int32, C.c_int64, C.POINTER(C.c_int64)])
    _trace_dev_sigs(lib)
    _trace_cache_sigs(lib)
    _sig(lib.hipstr_post_census_dev, C.c_int, [C.c_void_p, C.POINTER(HipstrCensusRequest), C.c_void_p, C.POINTER(HipstrCensusOut)])
    _em_trace_sigs(lib)
    _pool_sigs(lib)
    _hapgen_sigs(lib)
    return lib


def launch_plan(lib, bptr, ws_gib=0.0):
    """The launch plan hipstr_hmm_align would run for a batch (host only: hipstr_debug_launch_plan) as a dict; ws_gib > 0 sets the
    workspace budget per workspace."""
    import json
    n = lib.hipstr_debug_launch_plan(bptr, ws_gib, None, 0)
    if n < 0:
        raise RuntimeError("hipstr_debug_launch_plan failed: " + lib.hipstr_last_error().decode())
    buf = C.create_string_buffer(n + 1)
    assert lib.hipstr_debug_launch_plan(bptr, ws_gib, buf, n + 1) == n
    return json.loads(buf.value.decode())


def _plan_json(lib, what, call):
    """Two calls of a hipstr_debug_*_plan entry point: the length, then the JSON."""
    import json
    n = call(None, 0)
    if n < 0:
        raise RuntimeError("%s failed: %s" % (what, lib.hipstr_last_error().decode()))
    buf = C.create_string_buffer(n + 1)
    assert call(buf, n + 1) == n
    return json.loads(buf.value.decode())


def trace_plan(lib, bptr, req_read, req_allele, req_seed=None, ws_mib=0.0):
    """What hipstr_hmm_trace(_seeded) would launch for a request list (host only: hipstr_debug_trace_plan) as a dict; ws_mib > 0 sets the
    budget of decision matrices per chunk."""
    rr = np.ascontiguousarray(np.asarray(req_read, np.int32)); aa = np.ascontiguousarray(np.asarray(req_allele, np.int32))
    ss = None if req_seed is None else np.ascontiguousarray(np.asarray(req_seed, np.int32))
    return _plan_json(lib, "hipstr_debug_trace_plan", lambda buf, cap: lib.hipstr_debug_trace_plan(
        bptr, len(rr), rr.ctypes.data_as(_i32p), aa.ctypes.data_as(_i32p), _ptr(ss, _i32p), ws_mib, buf, cap))


def trace_assemble_plan(lib, bptr, req_read, req_allele, req_seed=None, hap_to_ref=None):
    """The slots and the staging route hipstr_hmm_trace_ex(TRACE_ASSEMBLE_DEVICE) gives every request of a list (host only:
    hipstr_debug_trace_assemble_plan) as a dict; "requests" rows are lists in the order of "fields"."""
    rr = np.ascontiguousarray(np.asarray(req_read, np.int32)); aa = np.ascontiguousarray(np.asarray(req_allele, np.int32))
    ss = None if req_seed is None else np.ascontiguousarray(np.asarray(req_seed, np.int32))
    h2r = None if hap_to_ref is None else (C.c_char_p * len(hap_to_ref))(*hap_to_ref)
    return _plan_json(lib, "hipstr_debug_trace_assemble_plan", lambda buf, cap: lib.hipstr_debug_trace_assemble_plan(
        bptr, len(rr), rr.ctypes.data_as(_i32p), aa.ctypes.data_as(_i32p), _ptr(ss, _i32p), h2r, buf, cap))


def nw_plan(lib, pairs, use_ref_end_penalty=False, ws_mib=0.0):
    """The chunks and fill kernels hipstr_nw_align would launch for [(ref, read), ...] (host only: hipstr_debug_nw_plan) as a dict."""
    refs = [r.encode() for r, _ in pairs]; reads = [q.encode() for _, q in pairs]
    ro = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    qo = np.concatenate([[0], np.cumsum([len(q) for q in reads])]).astype(np.int32)
    rb = b"".join(refs); qb = b"".join(reads)
    nb = HipstrNwBatch(len(pairs), ro.ctypes.data_as(_i32p), rb, qo.ctypes.data_as(_i32p), qb, int(use_ref_end_penalty))
    return _plan_json(lib, "hipstr_debug_nw_plan", lambda buf, cap: lib.hipstr_debug_nw_plan(C.byref(nb), ws_mib, buf, cap))


def post_plan(lib, pb):
    """The launch hipstr_post_launch would make for a PostBatch (host only: hipstr_debug_post_plan) as a dict."""
    return _plan_json(lib, "hipstr_debug_post_plan", lambda buf, cap: lib.hipstr_debug_post_plan(pb.ptr, buf, cap))


def _why(lib, prefix):
    """': <hipstr_last_error()>' for the MI355X library's entry points."""
    if not prefix.startswith("hipstr_"):
        return ""
    _sig(lib.hipstr_last_error, C.c_char_p, [])
    return ": " + lib.hipstr_last_error().decode()


def run_align(lib, prefix, bptr, fill=np.nan, seed_in=None):
    """Call <prefix>process_reads on a batch; returns (aln_probs, seeds) numpy arrays.
    Entries the callee leaves untouched keep `fill`.  seed_in: per-read seed bases chosen by the caller
    (<prefix>process_reads_seeded = HapAligner::process_read's seed_base argument; -2 = compute)."""
    n_reads, n_out, _ = batch_dims(bptr)
    probs = np.full(max(n_out, 1), fill, dtype=np.float64)
    seeds = np.full(max(n_reads, 1), -7, dtype=np.int32)
    if seed_in is not None:
        si = np.ascontiguousarray(np.asarray(seed_in, np.int32))
        fn = getattr(lib, prefix + "process_reads_seeded")
        _sig(fn, C.c_int, [_BP, _i32p, _f64p, _i32p])
        rc = fn(bptr, si.ctypes.data_as(_i32p), probs.ctypes.data_as(_f64p), seeds.ctypes.data_as(_i32p))
        if rc != 0:
            raise RuntimeError("%sprocess_reads_seeded failed rc=%d%s" % (prefix, rc, _why(lib, prefix)))
        return probs[:n_out], seeds[:n_reads]
    rc = getattr(lib, prefix + "process_reads")(bptr, probs.ctypes.data_as(_f64p), seeds.ctypes.data_as(_i32p))
    if rc != 0:
        raise RuntimeError("%sprocess_reads failed rc=%d%s" % (prefix, rc, _why(lib, prefix)))
    return probs[:n_out], seeds[:n_reads]


class HipstrStreamOpts(C.Structure):
    _fields_ = [("device", C.c_int32), ("slots", C.c_int32), ("batch_alignments", C.c_int64)]


class HipstrStreamStats(C.Structure):
    _fields_ = [("batches", C.c_int64), ("tickets", C.c_int64), ("alignment_slots", C.c_int64), ("host_seconds", C.c_double),
                ("wait_seconds", C.c_double), ("open_seconds", C.c_double), ("cpu_submit_seconds", C.c_double), ("cpu_prepare_seconds", C.c_double),
                ("cpu_upload_seconds", C.c_double), ("cpu_collect_seconds", C.c_double)]


class Stream:
    """hipstr_stream_*: loci in, results out in submission order (include/hipstr_hmm.h)."""

    def __init__(self, lib, device=0, slots=0, batch_alignments=0):
        self.lib = lib
        _sig(lib.hipstr_stream_open, C.c_void_p, [C.POINTER(HipstrStreamOpts)])
        _sig(lib.hipstr_stream_submit, C.c_int64, [C.c_void_p, _BP])
        _sig(lib.hipstr_stream_flush, C.c_int, [C.c_void_p])
        _sig(lib.hipstr_stream_submit_each, C.c_int, [C.c_void_p, _BP, C.POINTER(C.c_int64)])
        _sig(lib.hipstr_stream_collect, C.c_int, [C.c_void_p, C.c_int64, _f64p, C.c_int64, _i32p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
        _sig(lib.hipstr_stream_next_size, C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
        _sig(lib.hipstr_stream_next, C.c_int, [C.c_void_p, C.POINTER(C.c_int64), _f64p, C.c_int64, _i32p, C.c_int64])
        _sig(lib.hipstr_stream_stats, C.c_int, [C.c_void_p, C.POINTER(HipstrStreamStats)])
        _sig(lib.hipstr_stream_close, C.c_int, [C.c_void_p])
        o = HipstrStreamOpts(device, slots, batch_alignments)
        self.h = lib.hipstr_stream_open(C.byref(o))
        if not self.h:
            raise RuntimeError("hipstr_stream_open failed: " + lib.hipstr_last_error().decode())

    def submit(self, bptr):
        t = self.lib.hipstr_stream_submit(self.h, bptr)
        if t < 0:
            raise RuntimeError("hipstr_stream_submit failed: " + self.lib.hipstr_last_error().decode())
        return t

    def flush(self):
        assert self.lib.hipstr_stream_flush(self.h) == 0

    def submit_each(self, bptr):
        """Every locus of the batch as its own submission; returns the first ticket."""
        t = C.c_int64(-1)
        if self.lib.hipstr_stream_submit_each(self.h, bptr, C.byref(t)) != 0:
            raise RuntimeError("hipstr_stream_submit_each failed: " + self.lib.hipstr_last_error().decode())
        return t.value

    def collect(self, n_tickets, probs, seeds):
        """The next n_tickets submissions in order, back to back into probs / seeds; returns (doubles, seeds) written."""
        a = C.c_int64(); b = C.c_int64()
        if self.lib.hipstr_stream_collect(self.h, n_tickets, probs.ctypes.data_as(_f64p), probs.size, seeds.ctypes.data_as(_i32p), seeds.size,
                                          C.byref(a), C.byref(b)) != 0:
            raise RuntimeError("hipstr_stream_collect failed: " + self.lib.hipstr_last_error().decode())
        return a.value, b.value

    def next(self, fill=np.nan, into=None):
        """(ticket, aln_probs, seeds) of the next submission in order, or None when nothing is outstanding."""
        t = C.c_int64(); n_out = C.c_int64(); n_reads = C.c_int64()
        if self.lib.hipstr_stream_next_size(self.h, C.byref(t), C.byref(n_out), C.byref(n_reads)) == 2:
            return None
        if into is None:
            probs = np.full(max(n_out.value, 1), fill); seeds = np.full(max(n_reads.value, 1), -7, np.int32)
        else:
            probs, seeds = into
        rc = self.lib.hipstr_stream_next(self.h, C.byref(t), probs.ctypes.data_as(_f64p), probs.size, seeds.ctypes.data_as(_i32p), seeds.size)
        if rc != 0:
            raise RuntimeError("hipstr_stream_next failed: " + self.lib.hipstr_last_error().decode())
        return t.value, probs[:n_out.value], seeds[:n_reads.value]

    def stats(self):
        st = HipstrStreamStats()
        assert self.lib.hipstr_stream_stats(self.h, C.byref(st)) == 0
        return {k: getattr(st, k) for k, _ in HipstrStreamStats._fields_}

    def close(self):
        if self.h:
            self.lib.hipstr_stream_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_posteriors(lib, prefix, pb):
    S = int(pb.samp_off[-1])
    post = np.zeros(max(int(pb.post_off[-1]), 1)); tot = np.zeros(max(S, 1)); gt = np.zeros(max(2 * S, 2), dtype=np.int32)
    ltot = np.zeros(max(pb.struct.n_loci, 1))
    fn = getattr(lib, prefix + "posteriors")
    rc = fn(pb.ptr, post.ctypes.data_as(_f64p), tot.ctypes.data_as(_f64p), gt.ctypes.data_as(_i32p), ltot.ctypes.data_as(_f64p))
    if rc != 0:
        raise RuntimeError("%sposteriors failed rc=%d" % (prefix, rc))
    return post[:int(pb.post_off[-1])], tot[:S], gt[:2 * S].reshape(-1, 2), ltot[:pb.struct.n_loci]
