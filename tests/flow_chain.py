"""Helper (not a test module): the rounds of SeqStutterGenotyper::genotype() driven from Python over a BATCH of loci, on the entry points of
INTEGRATION.md §2a, against the reference's own final state (tests/golden/flow_<case>.txt.gz, written by the compiled reference through
integration/genotype_flow.cpp) from the reference's own inputs (tests/golden/flowin_<case>.txt.gz, the same driver's --dump-inputs).

  genotype()                      reference src/seq_stutter_genotyper.cpp:603-671     -> genotype_pass
  id_and_align_to_stutter_alleles :570-601                                            -> State.step, phase ADD
  get_unused_alleles' call sites  :649, :658 (the marks: :229-315)                    -> State.step, phases UNCALLED / UNSPANNED
  add_and_remove_alleles          :324-415                                            -> State.apply
  recompute_stutter_models        :1542-1581                                          -> run (the EM round and the second pass)

All loci go through the rounds as ONE batch: a locus leaves the add loop when its census has no candidate, then takes its two removal
checks, then idles (identity mapping, nothing realigned, no read copied) until the last locus is done.  What the recipe leaves to the caller
is restated here: the new blocks, Gray-code enumeration of the haplotypes, allele_mapping / realign_to_haplotype by haplotype string, the
trace cache.  The stages themselves belong to a backend: HostBackend (the oracle and the numpy restatements of the stage tests, which live
in this module: host_scatter / host_remap, assign_restate, census_restate) or DeviceBackend (exactly the calls of §2a).

All cases run with --no-flanks: assemble_flanks (:40-217) is De Bruijn assembly on the host and is out of scope.

Regenerate the fixtures (CPU only, needs oracle/_ref/libflow_ref.so from `make -C oracle flow`): python tests/flow_chain.py --regen"""
import gzip
import math
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from hipstr_amd import capi  # noqa: E402
import util  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
UNALIGNED = -100000.0                  # seq_stutter_genotyper.cpp:374
NO_STR = -100000                       # HIPSTR_NO_STR_DATA
FILL = -3.25                           # what the host arrays hold where process_reads leaves them untouched
LOG_ONE_HALF = math.log(0.5)           # mathops.cpp: LOG_ONE_HALF = log(0.5)
TOLERANCE = 1e-10                      # mathops.cpp:10
CENSUS_FILL = capi.CENSUS_FILL
MAX_TOTAL_HAPLOTYPES = 1000            # genotype(1000, 4, 0.15, ...) in integration/genotype_flow.cpp

# case -> arguments of integration/genotype_flow.cpp; what the rounds do is asserted from the fixtures (tests/test_flow_chain.py)
CASES = {
    "s4p3_noflank": ["--seed", "4", "--period", "3", "--no-flanks"],
    "s1p1_noflank": ["--seed", "1", "--period", "1", "--no-flanks"],
    "s1p3_noflank": ["--seed", "1", "--period", "3", "--no-flanks"],
    "s3p2_noflank": ["--seed", "3", "--period", "2", "--no-flanks"],
    "s12p4_noflank": ["--seed", "12", "--period", "4", "--no-flanks"],
    "s1p2_noflank": ["--seed", "1", "--period", "2", "--no-flanks"],
    "s11p3_noflank": ["--seed", "11", "--period", "3", "--no-flanks"],
    "s10p4_noflank": ["--seed", "10", "--period", "4", "--no-flanks"],
    "s12p6_noflank": ["--seed", "12", "--period", "6", "--no-flanks"],
    "s2p2_24samples_noflank": ["--seed", "2", "--period", "2", "--samples", "24", "--reads", "12", "--no-flanks"],
    "s3p5_24samples_noflank": ["--seed", "3", "--period", "5", "--samples", "24", "--reads", "12", "--no-flanks"],
    "s5p2_recompute_noflank": ["--seed", "5", "--period", "2", "--samples", "30", "--recompute", "--no-flanks"],
}


# ====================================================================================================== restatements of the stage tests
def host_scatter(M, seeds, A, read_off, pool_index, mates, copy, pool_ll, pool_seeds, pool_read_off, realign_hap):
    """seq_stutter_genotyper.cpp:530-564 on flat arrays, locus by locus (M and seeds are changed in place).  pool_ll / pool_seeds: what
    process_reads wrote for the pooled batch (P x A per locus); realign_hap: per locus a boolean array or None = all."""
    mo = po = 0
    for l in range(len(A)):
        a = int(A[l]); r0, r1 = int(read_off[l]), int(read_off[l + 1]); P = int(pool_read_off[l + 1] - pool_read_off[l])
        Ml = M[mo:mo + (r1 - r0) * a].reshape(r1 - r0, a); Pl = pool_ll[po:po + P * a].reshape(P, a)
        re_ = np.ones(a, bool) if realign_hap[l] is None else np.asarray(realign_hap[l], bool)
        for i in range(r0, r1):                                   # :532-543
            if not copy[i]:
                continue
            seeds[i] = pool_seeds[pool_read_off[l] + pool_index[i]]
            Ml[i - r0, re_] = Pl[pool_index[i], re_]
        for i in range(r0, r1):                                   # :551-564
            if not mates[i] or not copy[i]:
                continue
            total = Ml[i - r0 - 1, re_] + Ml[i - r0, re_]
            Ml[i - r0 - 1, re_] = total; Ml[i - r0, re_] = total
        mo += (r1 - r0) * a; po += P * a


def host_remap(M, A, read_off, new_A, mapping):
    """seq_stutter_genotyper.cpp:371-386 per locus -> the new flat matrix."""
    out = []; mo = jo = 0
    for l in range(len(A)):
        a, na, R = int(A[l]), int(new_A[l]), int(read_off[l + 1] - read_off[l])
        old = M[mo:mo + R * a].reshape(R, a); new = np.full((R, na), UNALIGNED)
        for j in range(a):
            if mapping[jo + j] != -1:
                new[:, mapping[jo + j]] = old[:, j]
        out.append(new.ravel()); mo += R * a; jo += a
    return np.concatenate(out) if out else np.zeros(0)


def _lse2(a, b, exp, log):            # mathops.cpp:52-57
    if a > b:
        return a + log(1 + exp(b - a))
    return b + log(1 + exp(a - b))


def _lse_vec(v, exp, log, pairwise=False):      # mathops.cpp:64-70
    mx = max(v)
    if pairwise:                      # NOT the reference: a tree sum, to show that the order of the additions matters
        t = [exp(x - mx) for x in v]
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return mx + log(t[0])
    total = 0.0
    for x in v:
        total += exp(x - mx)
    return mx + log(total)


def assign_restate(pb, LL, map_gt, seed, reverse=None, pool_index=None, pool_off=None, rule=capi.ASSIGN_VCF, tol=0.0, exp=math.exp, log=math.log,
                   pairwise=False):
    """seq_stutter_genotyper.cpp:1079-1157 + :1355-1356 (+ :823-825 for rule == ASSIGN_RETRACE) over a PostBatch; the shape of capi.run_assign."""
    a = pb.a
    nl = len(a["n_alleles"]); n = int(a["read_off"][-1]); ns = int(pb.samp_off[-1])
    tol = tol if tol != 0 else 0.1                                     # STRAND_TOLERANCE, seq_stutter_genotyper.h:157
    p1 = [float(x) for x in a["log_p1"]]; p2 = [float(x) for x in a["log_p2"]]
    LL = [float(x) for x in LL]
    o = dict(best_hap=np.full(n, -1, np.int32), read_strand=np.full(n, -1, np.int32), log_phase_one=np.full(n, np.nan), read_req=np.full(n, -1, np.int32),
             phase1_reads=np.zeros(ns), phase2_reads=np.zeros(ns))
    for k in capi.ASSIGN_COUNTERS:
        o[k] = np.zeros(ns, np.int32)
    phases = [[] for _ in range(ns)]
    cache = {}; req_read = []; req_allele = []
    ptr = 0
    for l in range(nl):
        A = int(a["n_alleles"][l]); haploid = a["haploid"] is not None and bool(a["haploid"][l])
        for r in range(int(a["read_off"][l]), int(a["read_off"][l + 1])):
            row = LL[ptr:ptr + A]; ptr += A
            if seed[r] < 0:                                            # :1080
                continue
            s = int(pb.samp_off[l]) + int(a["sample_label"][r])        # :1085
            ha, hb = int(map_gt[s][0]), int(map_gt[s][1])              # :1088-1089
            if ha < 0 or hb < 0:                                       # no MAP pair (every diplotype -inf): the reference would index haplotype -1
                continue                                               # here (in Python: silently the LAST allele); the library skips the sample's reads
            x1 = LOG_ONE_HALF + p1[r] + row[ha]; x2 = LOG_ONE_HALF + p2[r] + row[hb]
            total = _lse2(x1, x2, exp, log)                            # :1090
            lpo = LOG_ONE_HALF + p1[r] + row[ha] - total               # :1091
            phases[s].append(lpo); o["log_phase_one"][r] = lpo
            strand = 0                                                 # :1095
            if (not haploid) and ((ha != hb) or (abs(p1[r] - p2[r]) > TOLERANCE)):      # :1096
                v1 = p1[r] + row[ha]; v2 = p2[r] + row[hb]             # :1097
                if abs(v1 - v2) > tol:                                 # :1098
                    strand = 0 if v1 > v2 else 1                       # :1099
                    rv = reverse is not None and bool(reverse[r])
                    if strand == 0:                                    # :1100-1107
                        o["uniq_one"][s] += 1; o["rv_uniq_one"][s] += 1 if rv else 0
                    else:
                        o["uniq_two"][s] += 1; o["rv_uniq_two"][s] += 1 if rv else 0
            if rule == capi.ASSIGN_RETRACE:
                best = ha if x1 > x2 else hb                           # :825
            else:
                best = ha if strand == 0 else hb                       # :1113
            o["best_hap"][r] = best; o["read_strand"][r] = strand
            if pool_index is not None:                                 # :1115-1122 / :828-835: the cache fills in order of first occurrence
                key = (l, int(pool_index[r]), best)
                if key not in cache:
                    cache[key] = len(req_read); req_read.append(int(pool_off[l]) + int(pool_index[r])); req_allele.append(best)
                o["read_req"][r] = cache[key]
            o["n_aligned"][s] += 1                                     # :1135
            if abs(p1[r] - p2[r]) > TOLERANCE:                         # :1138-1144
                o["n_snp"][s] += 1
                if p1[r] > p2[r]:
                    o["n_strand_one"][s] += 1
                else:
                    o["n_strand_two"][s] += 1
    for s in range(ns):                                                # :1355-1356
        ph1 = 0 if o["n_aligned"][s] == 0 else exp(_lse_vec(phases[s], exp, log, pairwise))
        o["phase1_reads"][s] = ph1; o["phase2_reads"][s] = int(o["n_aligned"][s]) - ph1
    o["n_req"] = len(req_read); o["req_read"] = np.array(req_read, np.int32); o["req_allele"] = np.array(req_allele, np.int32)
    return o


def gray_h2a(nopts):
    """A haps_to_alleles-shaped map per block for a reflected mixed-radix Gray code with block 0 fastest."""
    A = nopts[0] * nopts[1] * nopts[2]; out = [[], [], []]
    for i in range(A):
        q = i
        for k in range(3):
            d = q % nopts[k]; q //= nopts[k]
            out[k].append(nopts[k] - 1 - d if q % 2 else d)
    return out


class Locus:
    """blocks: 3 x (start, end, [options]); samples: per sample the list of reads (log_p1, log_p2, LL row, seed, request within the locus or -1);
    reqs: list of (pool within the locus, aln_start, aln_stop, stutter_size, str_seq bytes)."""

    def __init__(self, blocks, samples, reqs, n_pooled=None, haploid=0, h2a=None):
        self.blocks, self.samples, self.reqs, self.haploid = blocks, samples, reqs, haploid
        self.nopts = [len(b[2]) for b in blocks]
        self.A = self.nopts[0] * self.nopts[1] * self.nopts[2]
        self.n_pooled = n_pooled if n_pooled is not None else (max([r[0] for r in reqs]) + 1 if reqs else 0)
        self.h2a = h2a if h2a is not None else gray_h2a(self.nopts)


class Case:
    pass


def census_restate(c, map_gt, h2a=None, uncallable=None, min_reads=2, min_frac=0.15, LL=None, trace=None, read_req=None, req_read=None, seed=None):
    """seq_stutter_genotyper.cpp:843-879 (+ :582-584) and :229-315 over a Case; the shape of capi.run_census."""
    a = c.pb.a
    h2a = c.h2a if h2a is None else h2a
    LL = [float(x) for x in (c.LL if LL is None else LL)]
    tr = c.trace if trace is None else trace
    read_req = c.read_req if read_req is None else read_req; req_read = c.req_read if req_read is None else req_read; seed = c.seed if seed is None else seed
    raw = bytes(tr["str_seq"]) if isinstance(tr["str_seq"], bytes) else tr["str_seq"].raw
    soff = [int(x) for x in tr["str_seq_off"]]
    strs = [raw[soff[q]:soff[q + 1]] for q in range(len(req_read))]
    start, stop, stut = [list(map(int, tr[k][:len(req_read)])) for k in ("aln_start", "aln_stop", "stutter_size")]
    req_locus = [int(np.searchsorted(c.pool_off, r, side="right")) - 1 for r in req_read]
    p1 = [float(x) for x in a["log_p1"]]; p2 = [float(x) for x in a["log_p2"]]
    ns = int(c.pb.samp_off[-1]); n_opts = sum(sum(L.nopts) for L in c.loci)
    o = dict(cand=[], cand_req=[], new_n_haps=[], n_spanning=np.zeros(ns, np.int32), n_span_stutter=np.zeros(ns, np.int32),
             called=np.full(n_opts, CENSUS_FILL, np.uint8), spanned=np.full(n_opts, CENSUS_FILL, np.uint8))
    ptr = 0; hap0 = 0; opt0 = 0
    for l, L in enumerate(c.loci):
        A = L.A; S = len(L.samples); s0 = int(c.pb.samp_off[l]); haploid = bool(L.haploid)
        bs, be = L.blocks[1][0], L.blocks[1][1]
        r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1])
        lab = [int(x) for x in a["sample_label"][r0:r1]]
        # ---- get_stutter_candidate_alleles
        counts = [0] * S; sc = [dict() for _ in range(S)]
        for r in range(r0, r1):
            q = int(read_req[r])
            if seed[r] < 0 or q < 0:                                   # traced_alns[read_index] == NULL, :853
                continue
            if start[q] < bs:                                          # :856
                if stop[q] > be:                                       # :857
                    if stut[q] != 0:                                   # :858
                        sc[lab[r - r0]][strs[q]] = sc[lab[r - r0]].get(strs[q], 0) + 1
                        o["n_span_stutter"][s0 + lab[r - r0]] += 1
                    counts[lab[r - r0]] += 1                           # :860
        cand = set()
        for s in range(S):
            for k, v in sc[s].items():
                if v >= min_reads and 1.0 * v / counts[s] >= min_frac:         # :869
                    if k not in [x.encode() for x in L.blocks[1][2]]:          # :870
                        cand.add(k)
        cand = sorted(cand, key=lambda s: (len(s), s))                 # :582 orderByLengthAndSequence
        o["cand"].append(cand)
        mine = [q for q in range(len(req_read)) if req_locus[q] == l]
        o["cand_req"] += [min(q for q in mine if strs[q] == k) for k in cand]
        o["new_n_haps"].append(A // L.nopts[1] * (L.nopts[1] + len(cand)))     # :583-584
        o["n_spanning"][s0:s0 + S] = counts
        # ---- get_unused_alleles
        aligned = [False] * S                                          # :244-247
        for r in range(r0, r1):
            if seed[r] >= 0:
                aligned[lab[r - r0]] = True
        for k in range(3):
            ob = opt0 + sum(L.nopts[:k])
            if h2a[k] is None:
                continue
            m = [int(x) for x in h2a[k][hap0:hap0 + A]]
            called = [0] * L.nopts[k]; spanned = [0] * L.nopts[k]
            if k == 1:                                                 # :266-291
                for r in range(r0, r1):
                    row = LL[ptr + (r - r0) * A:ptr + (r - r0 + 1) * A]
                    q = int(read_req[r])
                    if seed[r] < 0 or q < 0:
                        continue
                    if start[q] < bs and stop[q] > be and stut[q] == 0:
                        ha, hb = int(map_gt[s0 + lab[r - r0]][0]), int(map_gt[s0 + lab[r - r0]][1])
                        if ha < 0 or hb < 0:
                            continue
                        best = ha
                        if (not haploid) and ha != hb:
                            v1 = p1[r] + row[ha]; v2 = p2[r] + row[hb]
                            if abs(v1 - v2) > TOLERANCE:
                                best = ha if v1 > v2 else hb
                        spanned[m[best]] = 1
                o["spanned"][ob:ob + L.nopts[k]] = spanned
            for s in range(S):                                         # :294-301
                ha, hb = int(map_gt[s0 + s][0]), int(map_gt[s0 + s][1])
                if aligned[s] and not (uncallable is not None and uncallable[s0 + s]) and ha >= 0 and hb >= 0:
                    called[m[ha]] = 1; called[m[hb]] = 1
            o["called"][ob:ob + L.nopts[k]] = called
        ptr += (r1 - r0) * A; hap0 += A; opt0 += sum(L.nopts)
    o["cand_off"] = np.concatenate([[0], np.cumsum([len(x) for x in o["cand"]])]).astype(np.int32)
    o["cand_req"] = np.array(o["cand_req"], np.int32); o["new_n_haps"] = np.array(o["new_n_haps"], np.int64)
    return o


# ====================================================================================================== fixtures
def _read_gz(kind, name):
    with gzip.open(os.path.join(GOLD, "%s_%s.txt.gz" % (kind, name)), "rt") as f:
        return f.read()


def gold(name):
    """The reference's dump of the case: its final state."""
    return _read_gz("flow", name)


def _f64_of_hex(words):
    return np.array([int(x, 16) for x in words], np.uint64).view(np.float64)


class Inputs:
    """tests/golden/flowin_<case>.txt.gz: what the reference's constructor left for genotype()."""

    def __init__(self, name):
        self.name = name; self.recompute = "--recompute" in CASES[name]
        self.blocks = []; self.reads = []; self.sample = []; self.second_mate = []; self.strand = []; p1 = []; p2 = []
        for line in _read_gz("flowin", name).splitlines():
            w = line.split(" ")
            if w[0] == "region":
                self.region = (w[1], int(w[2]), int(w[3]), int(w[4]), w[5])
            elif w[0] == "initialized":
                assert w[1] == "1"
            elif w[0] == "num_samples":
                self.n_samples = int(w[1])
            elif w[0] == "num_reads":
                self.n_reads = int(w[1])
            elif w[0] == "block":
                assert int(w[1]) == len(self.blocks) and int(w[4]) == len(w) - 5
                self.blocks.append((int(w[2]), int(w[3]), w[5:]))
            elif w[0] == "repeat_block":
                self.rep_block, self.period = int(w[1]), int(w[2])
            elif w[0] == "stutter_model":
                self.stutter = _f64_of_hex(w[2:])
            elif w[0] == "read":
                assert int(w[1]) == len(self.reads)
                self.sample.append(int(w[2])); self.second_mate.append(int(w[3])); self.strand.append(int(w[4]))
                cigar = [(op, int(n)) for n, op in re.findall(r"(\d+)([A-Z=])", w[6])]
                self.reads.append(dict(seq=w[7], qual=w[8], start=int(w[5]), cigar=cigar))
                p1.append(w[9]); p2.append(w[10])
        self.log_p1 = _f64_of_hex(p1); self.log_p2 = _f64_of_hex(p2)
        assert len(self.reads) == self.n_reads and len(self.blocks) == 3 and self.rep_block == 1 and len(self.stutter) == 6
        assert self.sample == sorted(self.sample)                      # reads grouped by ascending sample (genotyper.h:105-113)


def what_the_rounds_do(name):
    """From the fixtures alone — the initial blocks of flowin_*, the final blocks and the `log` lines of flow_* — what genotype() did to the
    repeat block: dict(period, first, last, added, uncalled, unspanned), the three counts summed over both passes of a --recompute case."""
    inp = Inputs(name); first = len(inp.blocks[1][2])
    last = None; n = dict(added=0, uncalled=0, unspanned=0)
    for line in gold(name).splitlines():
        w = line.split(" ")
        if w[0] == "block" and w[1] == "1":
            last = int(w[4])
        if w[0] != "log":
            continue
        m = re.search(r"Identified (\d+) additional candidate alleles from stutter artifacts", line)
        if m:
            n["added"] += int(m.group(1))
        m = re.search(r"after removing (\d+) (uncalled alleles|alleles with no spanning reads)", line)
        if m:
            n["uncalled" if m.group(2) == "uncalled alleles" else "unspanned"] += int(m.group(1))
    assert first + n["added"] - n["uncalled"] - n["unspanned"] == last, name          # the log lines account for every option that came or went
    return dict(n, period=inp.period, first=first, last=last)


# ====================================================================================================== the caller's bookkeeping
ADD, UNCALLED, UNSPANNED, DONE = range(4)


def order_by_length_and_sequence(seqs):
    return sorted(seqs, key=lambda s: (len(s), s))                     # stringops.cpp:35-39


def hap_options(oracle, nopts):
    """[A, 3]: the option of every block in haplotype k, in the order Haplotype::next visits them (Gray code, Haplotype.cpp)."""
    n = np.ascontiguousarray(nopts, np.int32); A = capi.gray_num_combs(nopts)
    out = np.zeros((A, 3), np.int32); o = np.zeros(3, np.int32)
    for k in range(A):
        assert oracle.oracle_allele_options(n.ctypes.data_as(capi._i32p), k, o.ctypes.data_as(capi._i32p)) == 0
        out[k] = o
    return out


class State:
    """One locus between the rounds: its blocks, its phase in genotype(), its trace cache."""

    def __init__(self, inp, oracle):
        self.inp, self.oracle = inp, oracle
        self.blocks = [(s, e, list(o)) for s, e, o in inp.blocks]
        self.stutter = inp.stutter.copy()
        self.phase = ADD
        self.cache = {}                                                # trace_cache_: (pool, haplotype) -> (trace handle, request)

    @property
    def nopts(self):
        return [len(b[2]) for b in self.blocks]

    @property
    def A(self):
        return capi.gray_num_combs(self.nopts)

    def options(self):
        return hap_options(self.oracle, self.nopts)

    def hap_seqs(self):
        return ["".join(self.blocks[b][2][o[b]] for b in range(3)) for o in self.options()]

    def apply(self, remove, add):
        """add_and_remove_alleles (:324-415) without the alignment: the new blocks, then -> (allele_mapping, realign_to_haplotype)."""
        old = self.hap_seqs()
        index = {s: i for i, s in enumerate(old)}                      # :331-336 (a later haplotype with the same string wins)
        blocks = []
        for b, (s, e, opts) in enumerate(self.blocks):
            assert 0 not in remove[b]
            keep = [o for i, o in enumerate(opts) if i not in set(remove[b])]              # HapBlock::remove_alleles
            blocks.append((s, e, keep + list(add[b])))                                     # :345-350 add_alternate, in the order given
        self.blocks = blocks
        new = self.hap_seqs()
        mapping = [-1] * len(old); realign = []
        for j, s in enumerate(new):                                    # :358-367
            if s in index:
                realign.append(False); mapping[index[s]] = j
            else:
                realign.append(True)
        assert new[0] == old[0]                                        # :369
        self.cache = {(p, mapping[h]): v for (p, h), v in self.cache.items() if mapping[h] != -1}      # :401-409
        return mapping, realign

    def step(self, cand, called, spanned, new_n_haps):
        """What genotype() does with one census of this locus -> (allele_mapping, realign_to_haplotype, added)."""
        nopts = self.nopts; A = self.A
        none = [[], [], []]
        if self.phase == ADD:                                          # id_and_align_to_stutter_alleles :573-599
            cand = order_by_length_and_sequence([c.decode() for c in cand])                # :582
            assert int(new_n_haps) == A // nopts[1] * (nopts[1] + len(cand))               # :583-584
            if cand:
                assert new_n_haps <= MAX_TOTAL_HAPLOTYPES              # :591 (no case aborts)
                m, r = self.apply(none, [[], cand, []])
                return m, r, True
            self.phase = UNCALLED
        if self.phase == UNCALLED:                                     # :647-654 takes `called`
            self.phase = UNSPANNED
            rem = [[o for o in range(1, nopts[b]) if not called[b][o]] if nopts[b] > 1 else [] for b in range(3)]      # :255, :305-311
            if any(rem):
                m, r = self.apply(rem, none)
                return m, r, False
        if self.phase == UNSPANNED:                                    # :657-663 takes `spanned`
            self.phase = DONE
            assert nopts[0] == 1 and nopts[2] == 1                     # --no-flanks: only the repeat block has alternatives
            rem = [[], [o for o in range(1, nopts[1]) if not spanned[1][o]] if nopts[1] > 1 else [], []]
            if any(rem):
                m, r = self.apply(rem, none)
                return m, r, False
        return list(range(A)), [False] * A, False


def build_batch(states, reads, masks=None):
    b = capi.Batch()
    for l, s in enumerate(states):
        b.add_locus(s.blocks, s.inp.period, list(s.stutter), reads[l], realign_hap=None if masks is None else masks[l])
    return b.finalize()


def layout_of(states):
    k = Case()
    k.read_off = np.concatenate([[0], np.cumsum([s.inp.n_reads for s in states])]).astype(np.int32)
    k.n = int(k.read_off[-1])
    k.mates = np.array([m for s in states for m in s.inp.second_mate], np.uint8)
    k.n_samples = np.array([s.inp.n_samples for s in states], np.int32)
    k.samp_off = np.concatenate([[0], np.cumsum(k.n_samples)]).astype(np.int32)
    k.sample = np.array([x for s in states for x in s.inp.sample], np.int32)
    k.log_p1 = np.concatenate([s.inp.log_p1 for s in states]); k.log_p2 = np.concatenate([s.inp.log_p2 for s in states])
    return k


def post_kw(states, k):
    return dict(n_alleles=[s.A for s in states], n_samples=k.n_samples, read_off=k.read_off, sample_label=k.sample, log_p1=k.log_p1, log_p2=k.log_p2,
                read_weight=1 - k.mates.astype(np.int32))              # read_weights_: 0 for a second mate (:500)


def genotype_pass(states, be, oracle, recs):
    """genotype() (:603-671, --no-flanks) for a batch of loci.  Leaves the backend with the final posteriors launched."""
    k = layout_of(states); nl = len(states)
    for s in states:
        s.phase = ADD
    unpooled = build_batch(states, [s.inp.reads for s in states])
    pool = be.pool(unpooled, states)                                   # pooler_.pool (:632)
    k.pool_index, k.pool_off, pool_reads = pool["pool_index"], pool["pool_off"], pool["reads"]
    be.create([s.A for s in states], k)
    pooled = pool.get("batch") or build_batch(states, pool_reads)
    be.align_scatter(pooled, None, [None] * nl)                        # calc_hap_aln_probs (:636-638)
    seeds = be.seeds()
    if recs is not None:                                               # (the first record of a pass: the matrix after the first scatter, with be.diag)
        recs.append(dict(matrix_after_scatter=be.matrix()) if be.diag else {})
    while True:
        be.posteriors(post_kw(states, k))                              # calc_log_sample_posteriors (:639, :414)
        if all(s.phase == DONE for s in states):
            break
        asg = be.assign(seeds, k)                                      # retrace_alignments' picks (:805-841)
        tr = be.trace(pooled, asg, states)
        opts = [s.options() for s in states]
        h2a = [np.concatenate([o[:, b] for o in opts]).astype(np.int32) for b in range(3)]         # haps_to_alleles (:219-227)
        cen = be.census(pooled, seeds, asg, tr, h2a, states, k)
        rec = dict(read_off=k.read_off.copy(), n_alleles=np.array([s.A for s in states], np.int32), cand=cen["cand"], called=cen["called"].copy(),
                   spanned=cen["spanned"].copy(), new_n_haps=np.asarray(cen["new_n_haps"]).copy(),
                   n_req=int(asg["n_req"]), req_read=asg["req_read"].copy(), req_allele=asg["req_allele"].copy(), read_req=asg["read_req"].copy())
        mapping, masks, copy, new_A = [], [], np.zeros(k.n, np.uint8), []
        ob = 0; any_new = False
        for l, s in enumerate(states):
            if s.phase != DONE:                                        # this locus' retrace_alignments ran: the cache takes what it did not have
                for q in np.nonzero((asg["req_read"] >= k.pool_off[l]) & (asg["req_read"] < k.pool_off[l + 1]))[0]:
                    s.cache.setdefault((int(asg["req_read"][q] - k.pool_off[l]), int(asg["req_allele"][q])), (tr, int(q)))
            no = s.nopts; marks = [[cen[w][ob + sum(no[:b]):ob + sum(no[:b + 1])] for b in range(3)] for w in ("called", "spanned")]
            ob += sum(no)
            m, r, added = s.step(cen["cand"][l], marks[0], marks[1], cen["new_n_haps"][l])
            mapping += m; masks.append(np.array(r, np.uint8)); new_A.append(len(r))
            if added:                                                  # calc_hap_aln_probs only where a sequence was added (:397-398), every read copied
                copy[k.read_off[l]:k.read_off[l + 1]] = 1; any_new = True
        rec.update(mapping=np.array(mapping, np.int32), new_n_alleles=np.array(new_A, np.int32))
        be.end_posteriors()
        be.remap(new_A, mapping)
        if recs is not None and be.diag:
            rec["matrix_after_remap"] = be.matrix()
        if any_new:
            pooled = build_batch(states, pool_reads, masks)
            be.align_scatter(pooled, copy, masks)
        else:
            pooled = build_batch(states, pool_reads)
        if recs is not None:
            if be.diag:
                rec["matrix_after_scatter"] = be.matrix()
            recs.append(rec)
    return k, pooled, seeds


def fill_after_remap(rec):
    """seq_stutter_genotyper.cpp:374 on a round's record (taken with be.diag) -> (new columns, True iff in the matrix fetched after the remap
    every new column holds -100000 in every row and no kept column does)."""
    M = rec["matrix_after_remap"]; mo = jo = 0; n_new = 0; ok = True
    for l, (a, na) in enumerate(zip(rec["n_alleles"], rec["new_n_alleles"])):
        R = int(rec["read_off"][l + 1] - rec["read_off"][l])
        Ml = M[mo:mo + R * na].reshape(R, na)
        new = ~np.isin(np.arange(na), rec["mapping"][jo:jo + a])
        ok = ok and bool(np.all(Ml[:, new] == UNALIGNED)) and not np.any(Ml[:, ~new] == UNALIGNED)
        n_new += int(new.sum()); mo += R * na; jo += a
    assert mo == len(M)
    return n_new, ok


def dump_of(s, k, l, fin, stutter_model=None):
    """The lines of integration/genotype_flow.cpp's dump that the chain produces, in its format."""
    inp = s.inp; A = s.A; r0, r1 = int(k.read_off[l]), int(k.read_off[l + 1]); P = int(k.pool_off[l + 1] - k.pool_off[l])
    out = ["num_reads %d" % inp.n_reads, "num_samples %d" % inp.n_samples, "num_pools %d" % P, "num_alleles %d" % A]
    for b, (st, en, opts) in enumerate(s.blocks):
        out.append("block %d %d %d %d %s" % (b, st, en, len(opts), " ".join(opts)))
    ints = lambda key, v: "%s %d %s" % (key, len(v), " ".join(str(int(x)) for x in v))
    out += [ints("pool_index", k.pool_index[r0:r1]), ints("second_mate", k.mates[r0:r1]), ints("seed_positions", fin["seeds"][r0:r1])]
    out += ["pool_qual %d %s" % (i, rd["qual"]) for i, rd in enumerate(fin["pool_reads"][l])]
    ll = fin["ll"][fin["ll_off"][l]:fin["ll_off"][l + 1]]
    out.append("log_aln_probs %d %s" % (len(ll), " ".join("%016x" % int(x) for x in np.ascontiguousarray(ll).view(np.uint64))))
    S = inp.n_samples; s0 = int(k.samp_off[l])
    post = fin["post"][fin["post_off"][l]:fin["post_off"][l + 1]]
    out.append("log_sample_posteriors %d %s" % (len(post), " ".join("%.17g" % x for x in post)))
    out.append("sample_total_LLs %d %s" % (S, " ".join("%.17g" % x for x in fin["tot"][s0:s0 + S])))
    out.append("map_haplotypes %d %s" % (S, " ".join("%d|%d" % (a, b) for a, b in fin["gt"][s0:s0 + S])))
    for (p, h) in sorted(s.cache):
        tr, q = s.cache[(p, h)]; t = fin["traces"][tr][q]
        nostr = t["stutter_size"] == NO_STR
        out.append("trace %d %d %s %d %s %d %d %s" % (p, h, t["hap_aln"], t["stutter_size"], t["cigar"], t["aln_start"], t["aln_stop"], "-" if nostr else t["str_seq"]))
    if stutter_model is not None:
        out.append("stutter_model 6 %s" % " ".join("%.17g" % x for x in stutter_model))
    return "\n".join(out) + "\n"


def finish(states, k, be):
    fin = be.final()
    A = np.array([s.A for s in states], np.int64); R = np.diff(k.read_off).astype(np.int64)
    fin["ll_off"] = np.concatenate([[0], np.cumsum(R * A)]); fin["post_off"] = np.concatenate([[0], np.cumsum(k.n_samples.astype(np.int64) * A * A)])
    return fin


def run(names, be, oracle, recs=None):
    """Every case of `names` as one batch through genotype() [and, for the --recompute cases, recompute_stutter_models()] -> {name: dump}.
    recs: a list that receives one dict per round (the per-round intermediates; with be.diag also the matrix after each remap and scatter)."""
    states = [State(Inputs(n), oracle) for n in names]
    k, pooled, seeds = genotype_pass(states, be, oracle, recs)
    again = [l for l, s in enumerate(states) if s.inp.recompute]
    em = None
    if again:                                                          # recompute_stutter_models :1545-1577, on the whole batch
        asg = be.assign(seeds, k)
        tr = be.trace(pooled, asg, states)
        em = be.em(pooled, seeds, asg, tr, k)
        if recs is not None:
            recs.append(dict(em_trained=em[0].copy(), em_stutter=em[1].copy(), n_req=int(asg["n_req"]), req_read=asg["req_read"].copy(),
                             req_allele=asg["req_allele"].copy(), read_req=asg["read_req"].copy()))
    fin = finish(states, k, be)
    out = {s.inp.name: dump_of(s, k, l, fin) for l, s in enumerate(states) if l not in again}
    if again:
        sub = [states[l] for l in again]
        for l, s in zip(again, sub):
            assert em[0][l], "EM did not train"                        # :1571-1574
            s.stutter = em[1][l].copy()                                # :1577 set_stutter_model
            s.cache = {}                                               # :1579
        k2, _, _ = genotype_pass(sub, be, oracle, recs)                # :1580
        fin = finish(sub, k2, be)
        out.update({s.inp.name: dump_of(s, k2, i, fin, stutter_model=s.stutter) for i, s in enumerate(sub)})
    return out


def against_gold(got, name):
    """test_genotype_flow._compare — its bars, unchanged — on the lines the chain produces: everything of the reference's dump but
    genotype_ok / recompute_ok (the chain has no such flags) and the genotyper's log lines."""
    import test_genotype_flow as tgf
    want = "".join(l + "\n" for l in gold(name).splitlines() if l.split(" ")[0] not in ("genotype_ok", "recompute_ok", "log"))
    tgf._compare(got, want, loose_ll=Inputs(name).recompute)


# ====================================================================================================== backends
def _pool_reads_of(states, pool_off, rep, quals_of):
    out = []
    ro = np.concatenate([[0], np.cumsum([s.inp.n_reads for s in states])])
    for l, s in enumerate(states):
        rows = []
        for p in range(int(pool_off[l]), int(pool_off[l + 1])):
            rd = dict(s.inp.reads[int(rep[p]) - int(ro[l])]); rd["qual"] = quals_of(p)
            rows.append(rd)
        out.append(rows)
    return out


class HostBackend:
    """hipstr_pool_reads_host, the oracle's process_reads / posteriors / trace / em_train and the restatements above.  No device."""
    diag = True

    def __init__(self, hmm_host, oracle):
        self.hmm, self.ora = hmm_host, oracle
        self.traces = []

    def pool(self, unpooled, states):
        a = capi.run_pool(self.hmm, unpooled.ptr, host=True)           # hipstr_pool_reads_host
        raw = a["pool_quals"].tobytes(); qo = a["pool_qual_off"]
        self._reads = _pool_reads_of(states, a["pool_off"], a["pool_rep"], lambda p: raw[qo[p]:qo[p + 1]].decode())
        return dict(pool_index=a["pool_index"], pool_off=a["pool_off"], reads=self._reads)

    def create(self, A, k):
        self.k = k; self.A = np.array(A, np.int32)
        self.M = np.full(int((np.diff(k.read_off) * self.A).sum()), UNALIGNED); self.seed = np.full(k.n, -1, np.int32)

    def align_scatter(self, pooled, copy, masks):
        k = self.k
        ll, sd = capi.run_align(self.ora, "oracle_", pooled.ptr, fill=FILL)
        host_scatter(self.M, self.seed, self.A, k.read_off, k.pool_index, k.mates, np.ones(k.n, bool) if copy is None else copy, ll, sd, k.pool_off,
                     [None if m is None else m.astype(bool) for m in masks])

    def seeds(self):
        return self.seed.copy()

    def matrix(self):
        return self.M.copy()

    def posteriors(self, kw):
        self.pb = capi.PostBatch(log_aln_probs=self.M.copy(), **kw)
        self.post, self.tot, self.gt, _ = capi.run_posteriors(self.ora, "oracle_", self.pb)

    def end_posteriors(self):
        pass

    def assign(self, seeds, k):
        return assign_restate(self.pb, self.M, self.gt, seeds, pool_index=k.pool_index, pool_off=k.pool_off, rule=capi.ASSIGN_RETRACE)

    def trace(self, pooled, asg, states):
        """oracle_trace takes one locus per call."""
        k = self.k; recs = []
        d = util.batch_to_dict(pooled)
        h2r = capi.hap_aln_info(self.ora, "oracle_", pooled.ptr)
        ho = d["hap_off"]
        for l in range(len(states)):
            qs = np.nonzero((asg["req_read"] >= k.pool_off[l]) & (asg["req_read"] < k.pool_off[l + 1]))[0]
            assert len(qs) == 0 or np.array_equal(qs, np.arange(qs[0], qs[0] + len(qs)))
            if len(qs) == 0:
                continue
            one = build_batch([states[l]], [self._reads[l]])
            recs += capi.run_trace(self.ora, "oracle_", one.ptr, asg["req_read"][qs] - k.pool_off[l], asg["req_allele"][qs],
                                   hap_to_ref=h2r[ho[l]:ho[l + 1]], cap=1 << 18)
        assert len(recs) == asg["n_req"]
        self.traces.append(recs)
        return len(self.traces) - 1

    def _trace_dict(self, tr):
        recs = self.traces[tr]
        return capi.census_trace(np.array([t["aln_start"] for t in recs], np.int32), np.array([t["aln_stop"] for t in recs], np.int32),
                                 np.array([t["stutter_size"] for t in recs], np.int32), [t["str_seq"].encode() for t in recs])

    def census(self, pooled, seeds, asg, tr, h2a, states, k):
        c = Case(); c.pb = self.pb; c.pool_off = k.pool_off; c.h2a = h2a
        c.loci = [Locus(s.blocks, [None] * s.inp.n_samples, [], n_pooled=int(k.pool_off[l + 1] - k.pool_off[l])) for l, s in enumerate(states)]
        return census_restate(c, self.gt, LL=self.M, trace=self._trace_dict(tr), read_req=asg["read_req"], req_read=asg["req_read"], seed=seeds)

    def em(self, pooled, seeds, asg, tr, k):
        eb = capi.em_batch_from_traces(self.hmm, self.pb, pooled.ptr, seeds, asg["read_req"], asg["req_read"], self._trace_dict(tr))
        d = util.batch_to_dict(pooled)
        trained, st, _, _ = capi.run_em(self.ora, "oracle_", d["period"], k.n_samples, eb["read_off"], eb["sample_label"], eb["num_bps"], eb["log_p1"], eb["log_p2"])
        return trained, st

    def remap(self, new_A, mapping):
        self.M = host_remap(self.M, self.A, self.k.read_off, new_A, mapping); self.A = np.array(new_A, np.int32)

    def final(self):
        return dict(ll=self.M.copy(), seeds=self.seed.copy(), post=self.post, tot=self.tot, gt=self.gt, traces=self.traces, pool_reads=self._reads)


class DeviceBackend:
    """Exactly the calls of INTEGRATION.md §2a, in that order, nothing synchronised or fetched between them but what the recipe names: the
    seeds once after the first scatter, the assign request list, the census outputs, the EM result.  diag: also fetch the matrix after each
    remap and scatter (a second, diagnostic pass)."""

    def __init__(self, hmm, pool_flags=0, diag=False):
        self.hmm, self.flags, self.diag = hmm, pool_flags, diag
        self.tds = []; self.rm = None; self.pd = None; self.pbatch = None; self.keep = []

    def pool(self, unpooled, states):
        self.close_round()
        if self.pbatch is not None:
            self.pbatch.close()
        self.pbatch = capi.PooledBatch(self.hmm, unpooled.ptr, self.flags)                 # hipstr_pool_batch
        d = self.pbatch.arrays()
        reads = []
        for l in range(len(d["read_off"]) - 1):
            rows = []
            for p in range(int(d["read_off"][l]), int(d["read_off"][l + 1])):
                b0, b1 = int(d["base_off"][p]), int(d["base_off"][p + 1]); c0, c1 = int(d["cigar_off"][p]), int(d["cigar_off"][p + 1])
                rows.append(dict(seq=bytes(d["bases"][b0:b1]).decode(), qual=bytes(d["quals"][b0:b1]).decode(), start=int(d["read_start"][p]),
                                 cigar=[(chr(o), int(n)) for o, n in zip(d["cigar_op"][c0:c1], d["cigar_len"][c0:c1])]))
            reads.append(rows)
        self._reads = reads

        class First:                                                   # the round-1 batch is the library's own pooled batch
            ptr = self.pbatch.ptr
        return dict(pool_index=self.pbatch.pool_index, pool_off=d["read_off"].astype(np.int32), reads=reads, batch=First)

    def create(self, A, k):
        self.k = k
        if self.rm is not None:
            self.rm.close()
        self.rm = capi.ReadMatrix(self.hmm, A, k.read_off, k.pool_index, k.mates)          # hipstr_rm_create: -100000 everywhere, seeds -1

    def align_scatter(self, pooled, copy, masks):
        dev = self.hmm.hipstr_hmm_upload(pooled.ptr)
        assert dev, self.hmm.hipstr_last_error().decode()
        try:
            assert self.hmm.hipstr_hmm_align(dev, None) == 0, self.hmm.hipstr_last_error().decode()
            self.rm.scatter(dev, copy)
        finally:
            self.hmm.hipstr_hmm_free(dev)

    def seeds(self):
        s = np.zeros(max(self.k.n, 1), np.int32)
        assert self.hmm.hipstr_rm_fetch(self.rm.h, None, s.ctypes.data_as(capi._i32p)) == 0, self.hmm.hipstr_last_error().decode()
        return s[:self.k.n]

    def matrix(self):
        return self.rm.fetch()[0].copy()

    def posteriors(self, kw):
        self.pb = capi.PostBatch(log_aln_probs=None, **kw)
        self.pd = self.hmm.hipstr_post_upload(self.pb.ptr, self.rm.dev_ll)
        assert self.pd, self.hmm.hipstr_last_error().decode()
        assert self.hmm.hipstr_post_launch(self.pd, None) == 0, self.hmm.hipstr_last_error().decode()

    def end_posteriors(self):
        if self.pd:
            self.hmm.hipstr_post_free(self.pd); self.pd = None

    def close_round(self):
        self.end_posteriors()

    def assign(self, seeds, k):
        out = capi.run_assign(self.hmm, self.pd, seeds, pool_index=k.pool_index, pool_off=k.pool_off, rule=capi.ASSIGN_RETRACE, n_reads=k.n,
                              n_samp=int(k.samp_off[-1]))
        assert out["rc"] == 0
        return out

    def trace(self, pooled, asg, states):
        h2r = capi.hap_aln_info(self.hmm, "hipstr_", pooled.ptr)
        self.tds.append(capi.run_trace_resident(self.hmm, pooled.ptr, asg["req_read"], asg["req_allele"], hap_to_ref=h2r, flags=0))
        return len(self.tds) - 1

    def census(self, pooled, seeds, asg, tr, h2a, states, k):
        out = capi.run_census(self.hmm, self.pd, pooled.ptr, seeds, asg["read_req"], asg["req_read"], None, hap_to_allele=h2a, n_samp=int(k.samp_off[-1]),
                              td=self.tds[tr])
        assert out["rc"] == 0
        return out

    def em(self, pooled, seeds, asg, tr, k):
        out = capi.em_train_dev(self.hmm, self.pd, len(k.n_samples), pooled.ptr, seeds, asg["read_req"], asg["req_read"], self.tds[tr])
        return out[0], out[1]

    def remap(self, new_A, mapping):
        self.rm.remap(new_A, mapping)

    def final(self):
        """The only fetches of the chain: the matrix and the seeds, the posteriors, every resident trace result."""
        k = self.k; ll, seeds = self.rm.fetch()
        S = int(k.samp_off[-1]); nl = len(k.n_samples)
        A = self.rm.n_alleles.astype(np.int64)
        post = np.zeros(max(int((k.n_samples.astype(np.int64) * A * A).sum()), 1)); tot = np.zeros(max(S, 1)); gt = np.zeros(max(2 * S, 2), np.int32); lt = np.zeros(max(nl, 1))
        assert self.hmm.hipstr_post_fetch(self.pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p),
                                          lt.ctypes.data_as(capi._f64p)) == 0, self.hmm.hipstr_last_error().decode()
        traces = []
        for td in self.tds:
            if td is None:
                traces.append(None); continue
            n = td.sizes()[0]
            traces.append(capi.unpack_trace(capi.trace_dev_fetch(self.hmm, td), n))
            td.close()
        self.tds = [None] * len(self.tds)
        self.end_posteriors()
        return dict(ll=ll.copy(), seeds=seeds.copy(), post=post, tot=tot[:S], gt=gt[:2 * S].reshape(-1, 2), traces=traces, pool_reads=self._reads)

    def close(self):
        self.end_posteriors()
        for td in self.tds:
            if td is not None:
                td.close()
        self.tds = []
        if self.rm is not None:
            self.rm.close(); self.rm = None
        if self.pbatch is not None:
            self.pbatch.close(); self.pbatch = None


# ====================================================================================================== fixtures from the reference
if __name__ == "__main__" and "--regen" in sys.argv:
    import tempfile
    refdir = os.path.join(ROOT, "oracle", "_ref")
    for name, args in CASES.items():
        with tempfile.TemporaryDirectory() as t:
            out, inp = os.path.join(t, "flow.txt"), os.path.join(t, "in.txt")
            r = subprocess.run([os.path.join(refdir, "flow_launcher"), os.path.join(refdir, "libflow_ref.so")] + args + ["--out", out, "--dump-inputs", inp],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            assert r.returncode == 0, r.stdout
            for kind, path in (("flow", out), ("flowin", inp)):
                dst = os.path.join(GOLD, "%s_%s.txt.gz" % (kind, name))
                txt = open(path).read()
                if kind == "flow" and os.path.exists(dst) and gold(name) == txt:
                    continue                                           # a committed reference dump keeps its bytes
                with gzip.GzipFile(dst, "wb", mtime=0) as f:
                    f.write(txt.encode())
                print(name, kind, len(txt), "bytes ->", os.path.getsize(dst))
