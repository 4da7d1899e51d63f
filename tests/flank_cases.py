"""Fabricated inputs for the flank reassembly (hipstr_flank_kmer_lengths, hipstr_flank_assemble, hipstr_flank_assemble_dev) and a python
restatement of the aggregation of SeqStutterGenotyper::assemble_flanks (seq_stutter_genotyper.cpp:99-201) on per-task records.

A batch is a list of loci; a locus is dict(name, ref=(left, right), samples=[dict(reads=[...], masked=False)], nopts=(1, 1, 1), num_combs=None);
a read is dict(l=left flank string, r=right flank string, seed=True, req=True, pool=None).  Every read has a pooled read and a request of its
own unless `pool` names a pool of the locus it shares with others (their strings are then the first member's).

The per-task records (k, paths in pop order, weights) of the REFERENCE's DebruijnGraph for these batches are the goldens
tests/golden/flank_<batch>.npz (tests/golden/make_golden_flank.py; written through `genotype_flow --debruijn-cases`): one "case" of the text
format per (locus, flank) holding every sample's strings, masked samples included (the masks are the aggregation's business)."""
import ctypes as C
import os

import numpy as np

from hipstr_amd import capi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OK, INDEL, CYCLIC, LOW_FREQ = 0, 1, 2, 3
T_CYCLIC, T_SKIPPED = -1, -2
DEFAULTS = dict(min_kmer=10, max_kmer=15, min_path_weight=2, max_paths=10, max_total_haplotypes=1000, max_flank_haplotypes=4, min_flank_freq=0.15)


def rand_seq(rng, n, alphabet="ACGT"):
    """n bases without a repeated 8-mer (so that a flank is acyclic at k = 10 unless a case builds a repeat on purpose)."""
    while True:
        s = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n))
        if len({s[i:i + 8] for i in range(n - 7)}) == n - 7:
            return s


def sub(s, pos, base=None):
    b = base or {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}[s[pos]]
    assert b != s[pos]
    return s[:pos] + b + s[pos + 1:]


def rd(l, r, **kw):
    return dict(dict(l=l, r=r, seed=True, req=True, pool=None), **kw)


def unit_loci():
    """The unit cases: the smallest shapes at which the stage can go wrong.  Flank strings are 20-40 bases (the 16-path case: an 80-base
    reference flank and 31-base strings), at most 16 strings per sample except in the 101-string case."""
    rng = np.random.default_rng(7)
    T = rand_seq(rng, 24)                                      # the trivial other flank
    loci = []

    def locus(name, ref, samples, side=0, **kw):
        """samples: per sample a list of strings of the flank under test (or dict(strings=, masked=, other=)); the other flank's reads carry T."""
        ss = []
        for s in samples:
            d = s if isinstance(s, dict) else dict(strings=s)
            other = d.get("other")
            reads = [rd(x, (other[i] if other else T)) if side == 0 else rd((other[i] if other else T), x) for i, x in enumerate(d["strings"])]
            ss.append(dict(reads=reads, masked=d.get("masked", False)))
        loci.append(dict(dict(name=name, ref=(ref, T) if side == 0 else (T, ref), samples=ss, nopts=(1, 1, 1), num_combs=None), **kw))

    R = rand_seq(rng, 32)
    snp = sub(R, 16)
    locus("no_reads_and_short_strings", R, [[], [R[:8], R[3:13], ""], [R]])
    locus("snp_two_reads", R, [[R] * 3 + [snp] * 2], side=1)
    locus("snp_one_read_pruned", R, [[R] * 3 + [snp]])
    locus("threshold_three", R, [[R] * 99 + [snp] * 2, [R] * 97 + [snp] * 3, [R] * 47 + [snp] * 2], side=1)      # 102, 101 and 50 strings with the flank itself
    locus("alt_source", R, [[R] * 3 + [sub(R, 4)] * 3])
    locus("alt_sink", R, [[R] * 3 + [sub(R, 27)] * 3], side=1)
    locus("alt_source_with_incident_edge", R, [[R] * 3 + ["G" + sub(R, 4)] * 3])
    locus("source_with_incident_edge", R, [[R] * 2 + ["T" + R[:11]] * 2], side=1)                                 # the string is too short to enter at k = 12
    a = 8
    locus("cycle_at_10_not_at_12", R, [[R] * 2 + [R[:a] + R[a:a + 11] * 2 + R[a + 11:]] * 2])
    locus("cycle_at_every_k", R, [[R] * 2 + [R[:a] + R[a:a + 20] * 2 + R[a + 20:]] * 2, [R] * 2], side=1)
    ins = R[:16] + "T" + R[16:]
    dele = R[:16] + R[17:]
    locus("indels", R, [[R] * 3 + [ins] * 3, [R] * 3 + [dele] * 3, [R] * 4])
    locus("indel_then_equal_length", R, [[ins] * 3 + [sub(R, 20)] * 3, [sub(R, 12)] * 3 + [R[:20] + "G" + R[20:]] * 3, [R] * 2], side=1)
    W = rand_seq(rng, 80)
    sites = (15, 31, 47, 63)
    locus("sixteen_paths", W, [[sub(W, p)[p - 15:p + 16] for p in sites for _ in range(2)]])
    withn = sub(R, 15, "N")
    locus("strings_with_n", R, [[R] * 3 + [withn] * 3, [R[:10] + "NN" + R[12:]] * 2], side=1)
    locus("ref_len_10", R[:10], [[R[:10]] * 2])
    locus("ref_len_11", R[:11], [[R[:11]] * 2, []], side=1)
    locus("ref_len_0", "", [["", R[:12]]])
    locus("masked_sample", R, [dict(strings=[R] * 3 + [snp] * 2, masked=True), [R] * 3 + [snp] * 2], side=1)
    R2 = rand_seq(rng, 28)
    low = [dict(strings=[R] * 5, other=[R2] * 5) for _ in range(10)]
    low[3] = dict(strings=[R] * 3 + [snp] * 2, other=[R2] * 3 + [sub(R2, 14)] * 2)                               # its right flank would be low frequency too: skipped
    for i in (5, 6):
        low[i] = dict(strings=[R] * 5, other=[R2] * 3 + [sub(R2, 9)] * 2)                                       # 2 of 10 samples: frequent enough
    loci.append(dict(name="low_frequency_then_skipped", ref=(R, R2), nopts=(1, 1, 1), num_combs=None,
                     samples=[dict(reads=[rd(x, y) for x, y in zip(d["strings"], d["other"])], masked=False) for d in low]))
    locus("five_alternatives", R, [[R] * 3 + [sub(R, 10 + 2 * i)] * 2 for i in range(5)])
    locus("four_alternatives", R, [[R] * 3 + [sub(R, 10 + 2 * i)] * 2 for i in range(4)], side=1)
    locus("too_many_haplotypes", R, [[R] * 3 + [snp] * 2, [R] * 3 + [sub(R, 12)] * 2], num_combs=400)
    locus("two_left_options", R, [[R] * 3], nopts=(2, 3, 1), num_combs=6)
    shared = [dict(reads=[rd(R, T)] * 2 + [rd(snp, T)] * 2 + [rd(R, T, pool="both")], masked=False),
              dict(reads=[rd(R, T, pool="both"), rd(R, T), rd(R, T, seed=False), rd(snp, T, req=False)], masked=False)]
    loci.append(dict(name="shared_pool", ref=(R, T), samples=shared, nopts=(1, 1, 1), num_combs=None))
    return loci


def random_loci(seed=2024, n_loci=25, n_samples=4):
    """Seeded random small tasks (2 * n_loci * n_samples of them): reference flanks of 20-40 bases, 0-16 strings per sample cut from mutated
    copies (substitutions with N among them, 1-base indels, tandem copies of 11-18 bases that close cycles below their length); every fifth
    flank carries a repeat of 10-13 bases, so that its first k is above 10."""
    rng = np.random.default_rng(seed)
    below = lambda n: int(rng.integers(0, n))
    loci = []
    for l in range(n_loci):
        refs = []
        for f in range(2):
            ref = rand_seq(rng, 20 + below(21))
            if (2 * l + f) % 5 == 1:
                n = 10 + below(4); b = below(len(ref) - n + 1)
                ref += ref[b:b + n]
            refs.append(ref)
        samples = []
        for s in range(n_samples):
            strings = []
            for f in range(2):
                alleles = [refs[f]]
                for _ in range(below(4)):
                    m = refs[f]
                    for _ in range(1 + below(3)):
                        p = below(len(m)); kind = below(10)
                        if kind < 6:
                            m = m[:p] + "ACGTN"[below(5)] + m[p + 1:]
                        elif kind < 8:
                            m = m[:p] + m[p + 1:]
                        elif kind < 9:
                            m = m[:p] + "ACGT"[below(4)] + m[p:]
                        else:
                            n = 11 + below(8); b = below(max(1, len(m) - n))
                            m = m[:b] + m[b:b + n] + m[b:]
                    alleles.append(m)
                out = []
                for _ in range(16):
                    a = alleles[below(len(alleles))]
                    b = 0 if below(3) else below(len(a))
                    e = len(a) if below(3) else b + below(len(a) - b + 1)
                    out.append(a[b:e])
                strings.append(out)
            n = below(17)
            samples.append(dict(reads=[rd(strings[0][i], strings[1][i], seed=below(12) > 0, req=below(12) > 0) for i in range(n)], masked=False))
        loci.append(dict(name="random%d" % l, ref=tuple(refs), samples=samples, nopts=(1, 1, 1), num_combs=None))
    return loci


BATCHES = {"unit": unit_loci, "random": random_loci}


class Case:
    pass


def build(loci, **params):
    """The arrays of a batch: PostBatch, pooled hipstr_batch_t, per-read and per-request tables, the trace's flank arrays."""
    c = Case()
    c.loci = loci
    c.params = dict(params)
    nl = c.n_loci = len(loci)
    c.n_samples = [len(L["samples"]) for L in loci]
    read_off, label, seed, read_req, pool_index, masked = [0], [], [], [], [], []
    req_read, pooled_off, fl, nopts, opt_seqs, hap_off = [], [0], [], [], [], [0]
    for L in loci:
        pools = {}
        n_pools = 0
        for s, S in enumerate(L["samples"]):
            masked.append(1 if S.get("masked") else 0)
            for r in S["reads"]:
                label.append(s)
                seed.append(3 if r["seed"] else -1)
                if r["pool"] is not None and r["pool"] in pools:
                    pi, q = pools[r["pool"]]
                else:
                    pi = n_pools; n_pools += 1
                    q = len(req_read); req_read.append(pooled_off[-1] + pi); fl.append((r["l"], r["r"]))
                    if r["pool"] is not None:
                        pools[r["pool"]] = (pi, q)
                pool_index.append(pi)
                read_req.append(q if r["req"] else -1)
        read_off.append(len(label)); pooled_off.append(pooled_off[-1] + n_pools)
        no = L.get("nopts", (1, 1, 1))
        nopts += list(no)
        for blk in range(3):
            for o in range(no[blk]):
                opt_seqs.append(L["ref"][0] if (blk == 0 and o == 0) else L["ref"][1] if (blk == 2 and o == 0) else "ACACACAC" + "AC" * o)
        hap_off.append(hap_off[-1] + (L.get("num_combs") or no[0] * no[1] * no[2]))
    n = c.n_reads = len(label)
    c.n_req = len(req_read)
    c.read_off = np.asarray(read_off, np.int32); c.sample_label = np.asarray(label, np.int32)
    c.seed = np.asarray(seed, np.int32); c.read_req = np.asarray(read_req, np.int32); c.req_read = np.asarray(req_read, np.int32)
    c.pool_index = np.asarray(pool_index, np.int32); c.sample_masked = np.asarray(masked, np.uint8)
    c.pooled_off = np.asarray(pooled_off, np.int32)
    flat = [x for pair in fl for x in pair]
    c.trace = dict(flank_seq_off=np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int32) if flat else np.zeros(1, np.int32),
                   flank_seq="".join(flat).encode() + b"?")
    A = np.diff(hap_off).astype(np.int32) if nl else np.zeros(0, np.int32)
    c.pb = capi.PostBatch(A, c.n_samples, c.read_off, c.sample_label, np.zeros(n), np.zeros(n), np.ones(n, np.int32), np.zeros(int((np.diff(c.read_off) * A).sum())) if nl else np.zeros(0))
    s = capi.HipstrBatch()
    keep = dict(nopts=np.asarray(nopts, np.int32), opt_off=np.concatenate([[0], np.cumsum([len(x) for x in opt_seqs])]).astype(np.int32),
                seq="".join(opt_seqs).encode() + b"?", hap_off=np.asarray(hap_off, np.int32), read_off=c.pooled_off)
    s.n_loci = nl
    s.blk_nopts = keep["nopts"].ctypes.data_as(capi._i32p); s.opt_off = keep["opt_off"].ctypes.data_as(capi._i32p); s.seq = keep["seq"]
    s.hap_off = keep["hap_off"].ctypes.data_as(capi._i32p); s.read_off = keep["read_off"].ctypes.data_as(capi._i32p)
    s._keepalive = keep
    c.pooled = s
    c.hap_off = keep["hap_off"]; c.nopts = keep["nopts"]
    c.samp_off = np.concatenate([[0], np.cumsum(c.n_samples)]).astype(np.int64)
    return c


def args(c, **kw):
    """run_flank's / flank_plan's arguments for a case (without the trace or the handle)."""
    a = dict(pb=c.pb, bptr=C.pointer(c.pooled), seed=c.seed, read_req=c.read_req, req_read=c.req_read, pool_index=c.pool_index,
             sample_masked=c.sample_masked if c.sample_masked.any() else None)
    a.update(c.params); a.update(kw)
    return a


def task_strings(c, l, flank, s):
    """What the task's DebruijnGraph is fed: the non-empty flank strings of the sample's reads that have a trace, in read order."""
    off, seq = c.trace["flank_seq_off"], c.trace["flank_seq"]
    out = []
    for r in range(c.read_off[l], c.read_off[l + 1]):
        if c.sample_label[r] != s or c.seed[r] < 0 or c.read_req[r] < 0:
            continue
        q = int(c.read_req[r])
        x = seq[off[2 * q + flank]:off[2 * q + flank + 1]].decode()
        if x:
            out.append(x)
    return out


def case_text(c):
    """The text the reference-driven generator (and tests/cpp/flank_host_test.cpp) reads: a case per (locus, flank)."""
    p = dict(DEFAULTS, **c.params)
    lines = []
    for l, L in enumerate(c.loci):
        for f in range(2):
            lines.append("case %s.%d %d %d %d %d %d" % (L["name"], f, p["min_kmer"], p["max_kmer"], p["min_path_weight"], p["max_paths"], c.n_samples[l]))
            lines.append("ref %s" % (L["ref"][f] or "-"))
            for s in range(c.n_samples[l]):
                ss = task_strings(c, l, f, s)
                lines.append("sample %d" % len(ss))
                lines += ss
    return "\n".join(lines) + "\n"


def parse_records(text):
    """The generator's output -> {case name: dict(kmer, tasks=[dict(k, paths=[(weight, bytes)])])}."""
    out = {}
    cur = None
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cur = out[w[1]] = dict(kmer=int(w[3]), tasks=[])
        elif w[0] == "task":
            assert int(w[1]) == len(cur["tasks"])
            cur["tasks"].append(dict(k=int(w[3]), n=int(w[5]), paths=[]))
        elif w[0] == "path":
            cur["tasks"][-1]["paths"].append((int(w[1]), w[2].encode()))
    for v in out.values():
        assert all(t["n"] == len(t["paths"]) for t in v["tasks"])
    return out


def golden(name):
    """(case text, reference records) of tests/golden/flank_<name>.npz."""
    z = np.load(os.path.join(GOLD, "flank_%s.npz" % name))
    return z["cases"].tobytes().decode(), parse_records(z["records"].tobytes().decode())


def expect(c, records):
    """assemble_flanks' aggregation (:46-201) restated on the reference's per-task records -> what run_flank returns for the batch."""
    p = dict(DEFAULTS, **c.params)
    nl = c.n_loci
    n_samp = int(c.samp_off[-1])
    status = np.zeros(nl, np.int32); new_n = np.zeros(nl, np.int64); st = np.zeros(n_samp, np.uint8); realign = np.zeros(n_samp, np.uint8)
    opts = [[[], []] for _ in range(nl)]
    task_k = np.full(2 * n_samp, T_SKIPPED, np.int32); paths = [[] for _ in range(2 * n_samp)]
    for l, L in enumerate(c.loci):
        S = c.n_samples[l]; so = int(c.samp_off[l])
        total = int(c.hap_off[l + 1] - c.hap_off[l])
        ls = [OK] * S; lr = [0] * S; lo = [[], []]
        for f in range(2):
            rec = records["%s.%d" % (L["name"], f)]
            ref = L["ref"][f].encode()
            total //= int(c.nopts[3 * l + (0 if f == 0 else 2)])
            new_n[l] = total
            if rec["kmer"] < 0:
                status[l] = 1
                break
            index = {}
            for s in range(S):
                t = 2 * so + f * S + s
                if c.sample_masked[so + s] or ls[s] != OK:
                    task_k[t] = T_SKIPPED; paths[t] = []
                    continue
                tk = rec["tasks"][s]
                task_k[t] = tk["k"]; paths[t] = list(tk["paths"])
                if tk["k"] < 0:
                    ls[s] = CYCLIC
                    continue
                if len(tk["paths"]) <= 1:
                    continue
                depth = sum(w for w, _ in tk["paths"])
                for w, seq in tk["paths"]:
                    if seq == ref or not (w * 1.0 / depth > 0.25):
                        continue
                    if len(seq) != len(ref):
                        ls[s] = INDEL; lr[s] = 0
                    else:
                        index.setdefault(seq, []).append(s); lr[s] = 1
            for seq in sorted(index):
                if len(index[seq]) < p["min_flank_freq"] * S:
                    for s in index[seq]:
                        if ls[s] == OK:
                            ls[s] = LOW_FREQ; lr[s] = 0
                    del index[seq]
            if index:
                if len(index) > p["max_flank_haplotypes"]:
                    status[l] = 2
                    break
                lo[f] = [(seq, len(index[seq])) for seq in sorted(index)]
                total *= 1 + len(index)
                new_n[l] = total
        else:
            if total > p["max_total_haplotypes"]:
                status[l] = 3
        if status[l] == 0:
            st[so:so + S] = ls; realign[so:so + S] = lr; opts[l] = lo
    copy_read = np.zeros(c.n_reads, np.uint8); realign_pool = np.zeros(int(c.pooled_off[-1]), np.uint8)
    for l in range(nl):
        for r in range(c.read_off[l], c.read_off[l + 1]):
            flag = realign[int(c.samp_off[l]) + int(c.sample_label[r])]
            copy_read[r] = flag
            if flag:
                realign_pool[int(c.pooled_off[l]) + int(c.pool_index[r])] = 1
    return dict(status=status, new_n_haps=new_n, sample_status=st, realign_sample=realign, opts=opts, copy_read=copy_read, realign_pool=realign_pool,
                task_k=task_k, paths=paths)


def assert_matches(c, got, want, what):
    """run_flank's result against expect()'s: the statuses and the masks everywhere; everything else for the loci with status 0 (for the
    others only the status is promised)."""
    assert got["rc"] == 0, what
    assert np.array_equal(got["status"], want["status"]), "%s: status %s != %s" % (what, got["status"], want["status"])
    for k in ("copy_read", "realign_pool"):
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)
    for l, L in enumerate(c.loci):
        if want["status"][l] != 0:
            continue
        w = "%s, locus %s" % (what, L["name"])
        so, S = int(c.samp_off[l]), c.n_samples[l]
        assert got["new_n_haps"][l] == want["new_n_haps"][l], "%s: new_n_haps %d != %d" % (w, got["new_n_haps"][l], want["new_n_haps"][l])
        assert got["opts"][l] == want["opts"][l], "%s: options %s != %s" % (w, got["opts"][l], want["opts"][l])
        for k in ("sample_status", "realign_sample"):
            assert np.array_equal(got[k][so:so + S], want[k][so:so + S]), "%s: %s %s != %s" % (w, k, got[k][so:so + S], want[k][so:so + S])
        if "task_k" in got:
            assert np.array_equal(got["task_k"][2 * so:2 * (so + S)], want["task_k"][2 * so:2 * (so + S)]), "%s: task_k" % w
            for t in range(2 * so, 2 * (so + S)):
                assert got["paths"][t] == want["paths"][t], "%s: paths of task %d: %s != %s" % (w, t, got["paths"][t], want["paths"][t])


def same_bytes(a, b, what):
    """Two run_flank results (both entry points): every output array equal byte for byte."""
    assert a["rc"] == b["rc"], what
    for k in a["raw"]:
        x, y = a["raw"][k], b["raw"][k]
        assert (x == y) if isinstance(x, bytes) else np.array_equal(x, y), "%s: %s differs" % (what, k)
    assert a["need"] == b["need"], what
