"""Fabricated inputs for hipstr_em_batch_from_traces / hipstr_em_train_dev (tests/test_em_from_traces_host.py, _gpu.py) and the numpy
restatement of SeqStutterGenotyper::recompute_stutter_models' walk (seq_stutter_genotyper.cpp:1555-1566) they are compared with.

A case is a list of loci; a locus is dict(period, haploid (optional), runs): `runs` holds, per sample, the list of its reads, each one of
  ("in", size)      a traced read whose trace spans block 1: it enters with num_bps = size
  ("share", size)   the same, on the request of the locus' previous traced read (two reads sharing one request: `size` must be that read's)
  ("seed", size)    a spanning trace, but seed < 0 (traced_alns[r] == NULL)
  ("noreq",)        seed >= 0 but read_req == -1
  ("start", size)   aln_start == blk_start: does not span (the comparison is strict)
  ("stop", size)    aln_stop == blk_end: does not span
  ("nostr",)        spans, but its request has stutter_size == HIPSTR_NO_STR_DATA
A request's str_seq has STR_LEN bytes and its stutter_size is size - STR_LEN, so any size — negative ones too — can be made."""
import ctypes as C

import numpy as np

from hipstr_amd import capi

STR_LEN = 8
BLK_START, BLK_END = 100, 140
NO_STR_DATA = -100000


class Case:
    pass


def build(loci, seed=1, n_alleles=2):
    rng = np.random.default_rng(seed)
    c = Case()
    nl = len(loci)
    c.n_loci = nl
    c.period = [L["period"] for L in loci]
    c.haploid = [1 if L.get("haploid") else 0 for L in loci]
    c.n_samples = [len(L["runs"]) for L in loci]
    read_off, label, seeds, read_req = [0], [], [], []
    req_read, a_start, a_stop, stut, pooled_off = [], [], [], [], [0]
    for L in loci:
        last = -1
        for s, run in enumerate(L["runs"]):
            for rd in run:
                kind = rd[0]
                label.append(s)
                seeds.append(-1 if kind == "seed" else int(rng.integers(0, 50)))
                if kind == "noreq":
                    read_req.append(-1)
                    continue
                if kind == "share":
                    assert last >= 0
                    read_req.append(last)
                    continue
                k = len(req_read)
                req_read.append(k)                      # one pooled read per request
                a_start.append(BLK_START if kind == "start" else BLK_START - 1 - int(rng.integers(0, 20)))
                a_stop.append(BLK_END if kind == "stop" else BLK_END + 1 + int(rng.integers(0, 20)))
                stut.append(NO_STR_DATA if kind == "nostr" else int(rd[1]) - STR_LEN)
                read_req.append(k); last = k
        read_off.append(len(label))
        pooled_off.append(len(req_read))
    n = len(label); nq = len(req_read)
    c.n_reads, c.n_req = n, nq
    c.read_off = np.asarray(read_off, np.int32); c.sample_label = np.asarray(label, np.int32)
    c.seed = np.asarray(seeds, np.int32); c.read_req = np.asarray(read_req, np.int32); c.req_read = np.asarray(req_read, np.int32)
    # phasing likelihoods: a third of the reads without phasing information (log_p1 == log_p2)
    c.log_p1 = np.where(rng.random(n) < 0.33, np.log(0.5), np.log(rng.uniform(0.05, 0.95, n)))
    c.log_p2 = np.where(c.log_p1 == np.log(0.5), np.log(0.5), np.log1p(-np.exp(c.log_p1)))
    c.trace = dict(ll=np.zeros(nq), max_index=np.zeros(nq, np.int32), stutter_size=np.asarray(stut, np.int32), flank_ins=np.zeros(nq, np.int32),
                   flank_del=np.zeros(nq, np.int32), aln_start=np.asarray(a_start, np.int32), aln_stop=np.asarray(a_stop, np.int32),
                   str_seq_off=(STR_LEN * np.arange(nq + 1)).astype(np.int32), str_seq=b"A" * (STR_LEN * nq))
    c.pb = capi.PostBatch([n_alleles] * nl, c.n_samples, c.read_off, c.sample_label, c.log_p1, c.log_p2, np.ones(n, np.int32),
                          -rng.uniform(1, 30, n * n_alleles), haploid=c.haploid)
    c.pooled = pooled(nl, [BLK_START] * nl, [BLK_END] * nl, c.period, pooled_off)
    return c


def pooled(nl, blk_start, blk_end, period, read_off):
    """A hipstr_batch_t with the fields the EM's trace request reads: block 1's bounds, the periods, the pooled reads of every locus."""
    s = capi.HipstrBatch()
    bs = np.zeros(3 * nl, np.int32); be = np.zeros(3 * nl, np.int32)
    bs[1::3] = blk_start; be[1::3] = blk_end
    keep = dict(bs=bs, be=be, period=np.ascontiguousarray(np.asarray(period, np.int32)), read_off=np.ascontiguousarray(np.asarray(read_off, np.int32)))
    s.n_loci = nl
    s.blk_start = keep["bs"].ctypes.data_as(capi._i32p); s.blk_end = keep["be"].ctypes.data_as(capi._i32p)
    s.period = keep["period"].ctypes.data_as(capi._i32p); s.read_off = keep["read_off"].ctypes.data_as(capi._i32p)
    s._keepalive = keep
    return s


def restate(c, trace=None):
    """seq_stutter_genotyper.cpp:1555-1566 in numpy: the batch of the reads that enter, in order."""
    t = c.trace if trace is None else trace
    off, lab, bps, p1, p2 = [0], [], [], [], []
    bs = np.ctypeslib.as_array(c.pooled.blk_start, shape=(3 * c.n_loci,)) if c.n_loci else []
    be = np.ctypeslib.as_array(c.pooled.blk_end, shape=(3 * c.n_loci,)) if c.n_loci else []
    for l in range(c.n_loci):
        for r in range(c.read_off[l], c.read_off[l + 1]):
            q = c.read_req[r]
            if c.seed[r] < 0 or q < 0:
                continue                                                   # traced_alns[r] == NULL
            if t["aln_start"][q] < bs[3 * l + 1] and t["aln_stop"][q] > be[3 * l + 1]:      # :1558-1559
                bps.append(int(t["str_seq_off"][q + 1] - t["str_seq_off"][q]) + int(t["stutter_size"][q]))
                lab.append(c.sample_label[r]); p1.append(c.log_p1[r]); p2.append(c.log_p2[r])
        off.append(len(bps))
    return dict(read_off=np.asarray(off, np.int32), sample_label=np.asarray(lab, np.int32), num_bps=np.asarray(bps, np.int32),
                log_p1=np.asarray(p1, np.float64), log_p2=np.asarray(p2, np.float64))


def em_kw(c, batch, **kw):
    """run_em's keyword arguments for the batch of a case."""
    return dict(period=c.period, n_samples=c.n_samples, read_off=batch["read_off"], sample_label=batch["sample_label"], num_bps=batch["num_bps"],
                log_p1=batch["log_p1"], log_p2=batch["log_p2"], haploid=c.haploid, **kw)


def host_batch(lib, c, trace=None, **kw):
    return capi.em_batch_from_traces(lib, c.pb, C.pointer(c.pooled), c.seed, c.read_req, c.req_read, c.trace if trace is None else trace, **kw)


def same_batch(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("read_off", "sample_label", "num_bps", "log_p1", "log_p2"))
