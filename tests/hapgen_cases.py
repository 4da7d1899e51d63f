"""Fabricated inputs for the haplotype generator (hipstr_hapgen, hipstr_hapgen_host, hipstr_hapgen_batch) and a python restatement of
HaplotypeGenerator::add_haplotype_block / gen_candidate_seqs / extract_sequence / trim / fuse_haplotype_blocks (HaplotypeGenerator.cpp:12-366)
with the bounds loop of build_haplotype (seq_stutter_genotyper.cpp:428-432), written on strings and dicts as the reference is.

A batch is a list of loci; a locus is dict(name, chrom (the whole chromosome, a few hundred bases), region_start, region_stop, period,
n_samples, reads); a read is dict(start, stop, cigar=[(op, n)], seq, sample, use).  The window the library gets is
chrom[region_start - 40 : region_stop + 40] (empty where region_start < 40: such a locus fails the chromosome-end check first).

The three blocks and the status of the REFERENCE's own HaplotypeGenerator for these batches are the goldens tests/golden/hapgen_<batch>.npz
(tests/golden/make_golden_hapgen.py; written through `genotype_flow --hapgen-cases`).  The reference exposes no more than that; the
restatement must reproduce those blocks on every golden case and is then the yardstick for ext_*, dist_* and the per-locus counts.

A case the reference itself cannot finish is not in a golden batch; none had to be dropped: the reference accepts the alternative "" (a
deletion of the whole padded region) as any other."""
import os
import struct

import numpy as np

from hipstr_amd import capi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
LEFT_PAD = RIGHT_PAD = 5
REF_FLANK_LEN = 35
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A", "N": "A"}
STUTTER = [0.9, 0.05, 0.05, 0.7, 0.005, 0.005]


# ====================================================================================================== builders
def rand_seq(rng, n):
    return "".join("ACGT"[int(i)] for i in rng.integers(0, 4, n))


def chrom_with_repeat(rng, start, motif, copies, tail=200):
    """A chromosome with one repeat at `start`, flanks that do not continue it -> (chrom, region_start, region_stop)."""
    left, right = rand_seq(rng, start), rand_seq(rng, tail)
    if left[-1] == motif[-1]:
        left = left[:-1] + OTHER[left[-1]]
    if right[0] == motif[0]:
        right = OTHER[right[0]] + right[1:]
    return left + motif * copies + right, start, start + len(motif) * copies


def read(chrom, start, cigar, sample=0, use=True, stop=None, ins=None, lower=False, inclusive=False, n_at=None):
    """A read laid over chrom from `start` with the given CIGAR: '=' copies, 'X' substitutes, 'I' takes bases from `ins` (a string used up
    from its front; default 'T's alternating with 'G's), 'D' skips.  stop: as given, else start + the =, X and D runs (inclusive: one less)."""
    seq, pos, k = [], start, 0
    ins = ins if ins is not None else "TG" * 64
    for op, n in cigar:
        if op == "=":
            seq.append(chrom[pos:pos + n]); pos += n
        elif op == "X":
            seq.append("".join(OTHER[c] for c in chrom[pos:pos + n])); pos += n
        elif op == "I":
            seq.append(ins[k:k + n]); k += n
        else:
            pos += n
    s = "".join(seq)
    if n_at is not None:
        s = s[:n_at] + "N" + s[n_at + 1:]
    if lower:
        s = s.lower()
    end = pos - 1 if inclusive else pos
    return dict(start=start, stop=end if stop is None else stop, cigar=list(cigar), seq=s, sample=sample, use=use)


def locus(name, chrom, region_start, region_stop, period, n_samples, reads):
    return dict(name=name, chrom=chrom, region_start=region_start, region_stop=region_stop, period=period, n_samples=n_samples, reads=reads)


def padded_read(chrom, rs, re, edits, start=None, end=None, **kw):
    """A read over [start, end) whose only differences from the reference are `edits` inside the padded region [rs, re]: a list of
    ("X", i) / ("D", i, n) / ("I", i, n) at padded index i (ascending, not overlapping)."""
    start = rs - 30 if start is None else start
    end = re + 30 if end is None else end
    cigar, pos = [], start
    def push(op, n):
        if n <= 0:
            return
        if cigar and cigar[-1][0] == op:
            cigar[-1] = (op, cigar[-1][1] + n)
        else:
            cigar.append((op, n))
    for e in edits:
        at = rs + e[1]
        push("=", at - pos); pos = at
        if e[0] == "X":
            push("X", 1); pos += 1
        elif e[0] == "D":
            push("D", e[2]); pos += e[2]
        else:
            push("I", e[2])
    push("=", end - pos)
    return read(chrom, start, cigar, **kw)


def unit_extract():
    """One sample, 1-4 reads per locus: the span test's two edges under both stop conventions, insertions at and around the region's edges,
    deletions over them, the empty allele, X runs, lower case and N, and a read that is not flagged but bounds the flanks."""
    rng = np.random.default_rng(11)
    chrom, a, b = chrom_with_repeat(rng, 150, "ACGT", 5)
    rs, re = a - LEFT_PAD, b + RIGHT_PAD
    wide = lambda **kw: read(chrom, 100, [("=", 120)], **kw)
    x_at = lambda start, n, at=a + 6: [("=", at - start), ("X", 1), ("=", n - (at - start) - 1)]      # one substitution inside the repeat
    loci = []
    add = lambda name, reads: loci.append(locus(name, chrom, a, b, 4, 1, reads))
    add("start_at_edge_rejected", [wide(), read(chrom, rs, x_at(rs, 80))])
    add("start_one_before_edge", [wide(), read(chrom, rs - 1, x_at(rs - 1, 80))])
    add("stop_at_edge_rejected_exclusive", [wide(), read(chrom, 120, x_at(120, re - 120))])
    add("stop_one_beyond_exclusive", [wide(), read(chrom, 120, x_at(120, re + 1 - 120))])
    add("stop_at_edge_rejected_inclusive", [wide(inclusive=True), read(chrom, 120, x_at(120, re + 1 - 120), inclusive=True)])
    add("stop_one_beyond_inclusive", [wide(inclusive=True), read(chrom, 120, x_at(120, re + 2 - 120), inclusive=True)])
    add("insertion_where_the_region_begins", [wide(), read(chrom, 120, [("=", rs - 120), ("I", 3), ("=", 80)])])
    add("insertion_at_the_last_position", [wide(), read(chrom, 120, [("=", re - 120), ("I", 2), ("=", 30)])])
    add("two_insertions_at_the_last_position", [wide(), read(chrom, 120, [("=", re - 120), ("I", 2), ("I", 1), ("=", 30)])])
    add("insertion_before_the_region", [wide(), read(chrom, 120, [("=", rs - 1 - 120), ("I", 3), ("=", 80)])])
    add("insertion_after_the_region", [wide(), read(chrom, 120, [("=", re + 1 - 120), ("I", 3), ("=", 30)])])
    add("deletion_over_the_left_edge", [wide(), read(chrom, 120, [("=", rs - 2 - 120), ("D", 4), ("=", 80)])])
    add("deletion_over_the_right_edge", [wide(), read(chrom, 120, [("=", re - 2 - 120), ("D", 4), ("=", 30)])])
    add("deletion_of_the_whole_padded_region", [wide(), wide(), read(chrom, 120, [("=", rs - 3 - 120), ("D", re - rs + 6), ("=", 30)])] * 1)
    add("x_runs", [wide(), read(chrom, 120, [("=", a + 2 - 120), ("X", 3), ("=", 4), ("X", 2), ("=", 60)])])
    add("lower_case_and_n", [wide(), read(chrom, 120, [("=", 100)], lower=True), read(chrom, 118, x_at(118, 100), lower=True),
                             read(chrom, 119, [("=", 100)], n_at=a + 3 - 119), read(chrom, 119, [("=", 100)], n_at=a + 3 - 119, lower=True)])
    add("unflagged_read_bounds_the_flanks", [read(chrom, 125, [("=", 80)]), read(chrom, 126, x_at(126, 80)), read(chrom, 100, [("=", 130)], use=False)])
    add("unflagged_read_is_not_counted", [wide(), read(chrom, 120, x_at(120, 100), use=False)])
    return loci


def _sample_reads(chrom, rs, re, allele, sample, k):
    """A read of `sample` carrying allele number `allele` (0 = the reference) in the padded region; k spreads the starts."""
    edits = [] if allele == 0 else [("X", 6 + allele)] if allele < 6 else [("D", 8, allele - 4)]
    return padded_read(chrom, rs, re, edits, start=rs - 20 - (k % 7), sample=sample)


def counts_locus(name, rng, per_sample, n_samples=None, interleave=False, reverse=False, extra=()):
    """per_sample: per sample a dict allele -> reads (0 = reference).  interleave: the samples' reads take turns; reverse: the last sample's
    reads come first."""
    chrom, a, b = chrom_with_repeat(rng, 150, "ACGT", 5)
    rs, re = a - LEFT_PAD, b + RIGHT_PAD
    by_sample = []
    for s, d in enumerate(per_sample):
        by_sample.append([_sample_reads(chrom, rs, re, al, s, k) for al, c in sorted(d.items()) for k in range(c)])
    if interleave:
        reads, k = [], 0
        while any(by_sample):
            if by_sample[k % len(by_sample)]:
                reads.append(by_sample[k % len(by_sample)].pop(0))
            k += 1
    else:
        reads = [r for rr in (reversed(by_sample) if reverse else by_sample) for r in rr]
    reads += list(extra(chrom, rs, re)) if extra else []
    return locus(name, chrom, a, b, 4, n_samples or len(per_sample), reads)


def unit_thresholds():
    rng = np.random.default_rng(12)
    loci = []
    add = lambda name, per_sample, **kw: loci.append(counts_locus(name, rng, per_sample, **kw))
    # strong in a sample: c >= 2 and c >= 0.2 n.  The other samples keep the reads' and the samples' shares of allele 1 at or under 5 %.
    add("strong_2_of_10", [{0: 8, 1: 2}, {0: 11}, {0: 11}, {0: 11}])
    add("not_strong_2_of_11", [{0: 9, 1: 2}, {0: 10}, {0: 10}, {0: 10}])
    add("not_strong_1_of_1", [{1: 1}, {0: 10}, {0: 10}])
    # read_counts against 0.05 tot_reads, sample_counts against 0.05 tot_samples: equal is out (strict >), one more is in
    add("reads_exactly_5_percent", [{0: 9, 1: 1}, {0: 9, 1: 1}, {0: 10}, {0: 10}])
    add("reads_one_more", [{0: 9, 1: 1}, {0: 9, 1: 1}, {0: 9, 1: 1}, {0: 10}])
    add("reads_exactly_5_percent_eight_samples", [{0: 4, 1: 1}, {0: 4, 1: 1}] + [{0: 5}] * 6)
    add("fraction_exactly_5_percent", [{0: 4, 1: 1}, {0: 10}, {0: 10}, {0: 10}])
    add("fraction_one_more", [{0: 3, 1: 1}, {0: 10}, {0: 10}, {0: 10}])
    add("fraction_and_reads_exact_together", [{0: 4, 1: 1}, {0: 5}, {0: 5}, {0: 5}])
    # samples
    nonspanning = lambda chrom, rs, re: [read(chrom, rs + 2, [("=", 60)], sample=1), read(chrom, rs - 60, [("=", 50)], sample=1)]
    add("sample_without_spanning_reads", [{0: 3, 1: 2}, {}, {0: 4}], extra=nonspanning)
    add("sample_index_without_any_read", [{0: 3, 1: 2}, {}, {0: 4}], n_samples=5)
    add("three_samples_interleaved", [{0: 4, 1: 2}, {0: 3, 2: 3}, {1: 2, 2: 2, 3: 1}], interleave=True)
    # the reference string: strong, weak only, absent
    add("reference_strong", [{0: 5, 1: 3}])
    add("reference_weak_only", [{0: 1, 1: 30, 2: 29}, {1: 30}])
    add("reference_absent", [{1: 3, 2: 3}])
    # denominators 3, 7, 9, 11: the double sum depends on the order; ascending sample index whatever the order of the reads
    add("four_denominators", [{0: 2, 1: 1}, {0: 5, 1: 2}, {0: 8, 1: 1}, {0: 8, 1: 3}])
    add("four_denominators_reads_reversed", [{0: 2, 1: 1}, {0: 5, 1: 2}, {0: 8, 1: 1}, {0: 8, 1: 3}], reverse=True)
    add("four_denominators_other_samples", [{0: 8, 1: 3}, {0: 8, 1: 1}, {0: 5, 1: 2}, {0: 2, 1: 1}], interleave=True)
    add("four_denominators_third_order", [{0: 8, 1: 1}, {0: 8, 1: 3}, {0: 2, 1: 1}, {0: 5, 1: 2}])
    return loci


def trim_locus(name, rng, period, copies, alts, n_ref=3):
    motif = {1: "A", 2: "AC", 3: "ACG", 4: "ACGT", 5: "ACGTT", 6: "ACGTTG"}[period]
    chrom, a, b = chrom_with_repeat(rng, 150, motif, copies)
    rs, re = a - LEFT_PAD, b + RIGHT_PAD
    reads = [padded_read(chrom, rs, re, [], start=rs - 20 - k) for k in range(n_ref)]
    for edits in alts:
        reads += [padded_read(chrom, rs, re, edits, start=rs - 25 - k) for k in range(3)]
    return locus(name, chrom, a, b, period, 1, reads)


def unit_trim():
    rng = np.random.default_rng(13)
    loci = []
    add = lambda name, period, copies, alts, **kw: loci.append(trim_locus(name, rng, period, copies, alts, **kw))
    L = lambda period, copies: period * copies + 10                    # length of the padded reference
    add("no_trim_short_reference", 6, 1, [[("X", 8)]])                 # 16 <= 18
    add("no_trim_short_alternative", 6, 4, [[("D", 6, 18)]])           # 34 - 18 = 16 <= 18
    add("min_len_one_over", 6, 4, [[("D", 6, 15)]])                    # 19: one base may go
    add("prefix_2_suffix_5", 4, 6, [[("X", 2)]])
    add("prefix_5_suffix_1", 4, 6, [[("X", L(4, 6) - 2)]])
    add("prefix_0_suffix_0", 4, 6, [[("X", 0), ("X", L(4, 6) - 1)]])
    add("balancing_steps_on_both_sides", 6, 5, [[("D", 8, 16)]])       # min_len 24, ideal 18, both sides 5: four steps back
    add("balancing_one_step", 6, 5, [[("D", 8, 13)]])                  # min_len 27: 27 - 10 = 17 < 18
    add("balancing_exact", 6, 5, [[("D", 8, 12)]])                     # min_len 28: 28 - 10 = 18
    add("left_arm", 6, 5, [[("D", 8, 9), ("X", L(6, 5) - 3)]])         # min_len 31, left 5, right 2
    add("left_arm_capped", 6, 5, [[("D", 8, 16), ("X", L(6, 5) - 3)]])   # min_len 24: left min(5, 24 - 18 - 2) = 4
    add("right_arm", 6, 5, [[("X", 1), ("D", 8, 9)]])                  # left 1, right 5
    add("right_arm_capped", 6, 5, [[("X", 1), ("D", 8, 17)]])          # min_len 23: right min(5, 23 - 18 - 1) = 4
    add("period_1", 1, 12, [[("D", 8, 1)], [("I", 8, 2)]])
    add("period_1_short", 1, 3, [[("I", 7, 1)]])
    add("period_6_long", 6, 8, [[("I", 20, 6)], [("D", 20, 12)]])
    add("only_the_reference", 4, 6, [])
    add("three_alternatives_share_four", 4, 6, [[("X", 4)], [("X", 9)], [("X", L(4, 6) - 5)]])
    return loci


def unit_status():
    rng = np.random.default_rng(14)
    loci = []
    def add(name, start, tail, reads_of, copies=5):
        chrom, a, b = chrom_with_repeat(rng, start, "ACGT", copies, tail=tail)
        loci.append(locus(name, chrom, a, b, 4, 1, reads_of(chrom, a, b)))
    two = lambda s0, e1: (lambda chrom, a, b: [read(chrom, a + s0, [("=", (b + e1) - (a + s0))]), read(chrom, a + s0 + 1, [("=", (b + e1) - (a + s0) - 2)])])
    add("region_start_39", 39, 100, two(-30, 30))
    add("region_start_40", 40, 100, two(-30, 30))
    add("region_stop_plus_40_is_chrom_len", 100, 40, two(-30, 30))
    add("region_stop_plus_40_beyond", 100, 39, two(-30, 30))
    add("min_start_plus_5_at_the_edge", 100, 100, two(-10, 30))       # min_aln_start + 5 == region_start - 5
    add("min_start_one_earlier", 100, 100, two(-11, 30))
    add("max_stop_minus_5_at_the_edge", 100, 100, two(-30, 10))
    add("max_stop_one_later", 100, 100, two(-30, 11))
    return loci


def no_flagged_loci():
    """The documented deviation: without a flagged read the reference computes INT_MAX + 5 (undefined); the library says status 2.  Not in any
    golden batch."""
    rng = np.random.default_rng(16)
    chrom, a, b = chrom_with_repeat(rng, 100, "ACGT", 5)
    return [locus("no_reads", chrom, a, b, 4, 1, []),
            locus("no_flagged_read", chrom, a, b, 4, 2, [read(chrom, 60, [("=", 100)], use=False), read(chrom, 61, [("=", 100)], sample=1, use=False)])]


def random_loci(seed=15, n_loci=40):
    """About 40 loci: 5-130 reads (63, 64 and 65 among them), 1-6 samples, periods 1-6, stutter of 1-2 units, substitutions and indels
    within 5 bases of the repeat, reads in no order of samples."""
    rng = np.random.default_rng(seed)
    sizes = [63, 64, 65, 5, 130] + [int(x) for x in rng.integers(5, 131, n_loci - 5)]
    loci = []
    for li, n_reads in enumerate(sizes):
        period = 1 + li % 6
        motif = rand_seq(rng, period)
        while period > 1 and motif == motif[0] * period:
            motif = rand_seq(rng, period)
        copies = int(rng.integers(3, 9)) + (6 if period == 1 else 0)
        chrom, a, b = chrom_with_repeat(rng, 120, motif, copies)
        rs, re = a - LEFT_PAD, b + RIGHT_PAD
        S = int(rng.integers(1, 7))
        reads = []
        for k in range(n_reads):
            edits = []
            u = rng.random()
            units = int(rng.integers(1, 3))
            if u < 0.15 and copies - units >= 1:
                edits.append(("D", LEFT_PAD, units * period))
            elif u < 0.30:
                edits.append(("I", LEFT_PAD, units * period))
            if rng.random() < 0.10:                                   # a substitution somewhere in the padded region, behind the stutter
                lo = (edits[0][1] + (edits[0][2] if edits[0][0] == "D" else 0)) if edits else 0
                at = int(rng.integers(lo, re - rs))
                edits.append(("X", at))
            if not edits and rng.random() < 0.06:                     # an indel in the pad
                edits.append(("D", int(rng.integers(0, 4)), 1) if rng.random() < 0.5 else ("I", int(rng.integers(re - rs - 4, re - rs + 1)), 1))
            spanning = rng.random() < 0.85
            start = rs - int(rng.integers(1, 60)) if spanning else (rs + int(rng.integers(0, 8)) if rng.random() < 0.5 else rs - int(rng.integers(1, 60)))
            end = re + int(rng.integers(1, 60)) if spanning or start >= rs else re - int(rng.integers(0, 8))
            ins = motif * 2 if (edits and edits[0][0] == "I" and edits[0][1] == LEFT_PAD and len(edits[0]) == 3 and edits[0][2] % period == 0) else None
            r = padded_read(chrom, rs, re, edits if start < rs and end > re else [], start=start, end=max(end, start + 10), sample=int(rng.integers(0, S)),
                            use=rng.random() < 0.95, ins=ins, lower=rng.random() < 0.05)
            reads.append(r)
        loci.append(locus("random_%02d_p%d_n%d" % (li, period, n_reads), chrom, a, b, period, S, reads))
    return loci


BATCHES = {"unit_extract": unit_extract, "unit_thresholds": unit_thresholds, "unit_trim": unit_trim, "unit_status": unit_status, "random": random_loci}


# ====================================================================================================== the reference's text format
def cigar_text(cigar):
    return "".join("%d%s" % (n, op) for op, n in cigar)


def case_text(loci):
    """`genotype_flow --hapgen-cases`: per locus "case NAME REGION_START REGION_STOP PERIOD N_SAMPLES N_READS", "chrom SEQ", then per read
    "read SAMPLE START STOP USE CIGAR SEQ"."""
    out = []
    for lc in loci:
        out.append("case %s %d %d %d %d %d" % (lc["name"], lc["region_start"], lc["region_stop"], lc["period"], lc["n_samples"], len(lc["reads"])))
        out.append("chrom %s" % lc["chrom"])
        for r in lc["reads"]:
            out.append("read %d %d %d %d %s %s" % (r["sample"], r["start"], r["stop"], 1 if r["use"] else 0, cigar_text(r["cigar"]), r["seq"]))
    return "\n".join(out) + "\n"


def parse_cases(text):
    """case_text's inverse (the golden files hold the text, not the builders' output)."""
    import re
    loci, lines, i = [], text.splitlines(), 0
    while i < len(lines):
        w = lines[i].split(" ")
        assert w[0] == "case"
        n = int(w[6])
        chrom = lines[i + 1].split(" ")[1]
        reads = []
        for ln in lines[i + 2:i + 2 + n]:
            x = ln.split(" ")
            assert x[0] == "read"
            reads.append(dict(sample=int(x[1]), start=int(x[2]), stop=int(x[3]), use=x[4] == "1", cigar=[(op, int(k)) for k, op in re.findall(r"(\d+)([=XID])", x[5])], seq=x[6]))
        loci.append(locus(w[1], chrom, int(w[2]), int(w[3]), int(w[4]), int(w[5]), reads))
        i += 2 + n
    return loci


def parse_records(text):
    """What the driver wrote -> {name: dict(status, message, blocks=[(start, end, [options])])}; "-" is the empty option."""
    recs, cur = {}, None
    for ln in text.splitlines():
        w = ln.split(" ")
        if w[0] == "case":
            cur = dict(status=int(w[3]), message=" ".join(w[4:]), blocks=[])
            recs[w[1]] = cur
        elif w[0] == "block":
            assert int(w[1]) == len(cur["blocks"]) and int(w[4]) == len(w) - 5
            cur["blocks"].append((int(w[2]), int(w[3]), ["" if s == "-" else s for s in w[5:]]))
        elif w[0] == "time":
            pass
        else:
            raise AssertionError(ln)
    return recs


def load_golden(name):
    d = np.load(os.path.join(GOLD, "hapgen_%s.npz" % name))
    return parse_cases(d["cases"].tobytes().decode()), parse_records(d["records"].tobytes().decode())


# ====================================================================================================== the restatement
def upper(s):
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in s)


def gapped(r):
    """The alignment string of a read: its bases with '-' for deleted reference bases."""
    out, k = [], 0
    for op, n in r["cigar"]:
        if op == "D":
            out.append("-" * n)
        else:
            out.append(r["seq"][k:k + n]); k += n
    return "".join(out)


def extract_sequence(r, region_start, region_end):
    """:82-155 -> None (false) or (string, read offset of its first base).  For an empty string the offset is the number of read bases in
    front of the place the walk ended."""
    if r["start"] >= region_start or r["stop"] <= region_end:
        return None
    aln = gapped(r)
    align_index = char_index = 0
    pos = r["start"]
    ci, cig = 0, r["cigar"]
    kept = []                                                          # indices into aln
    done = lambda: ("".join(aln[i] for i in kept), (len(aln[:kept[0]].replace("-", "")) if kept else len(aln[:align_index].replace("-", ""))))
    while ci < len(cig):
        op, num = cig[ci]
        if char_index == num:
            ci += 1; char_index = 0
        elif pos > region_end:
            return done()
        elif pos == region_end:
            if op == "I":
                kept += range(align_index, align_index + num)
                align_index += num; char_index = 0; ci += 1
            else:
                return done()
        elif pos >= region_start:
            nb = min(region_end - pos, num - char_index)
            if op == "I":
                nb = num
                kept += range(align_index, align_index + nb)
            elif op in "=X":
                kept += range(align_index, align_index + nb); pos += nb
            else:
                pos += nb
            align_index += nb; char_index += nb
        else:
            if op == "I":
                nb = num - char_index
            else:
                nb = min(region_start - pos, num - char_index); pos += nb
            align_index += nb; char_index += nb
    raise AssertionError("Logical error in extract_sequence")


def trim(ideal_min_length, region_start, region_end, sequences):
    """:12-80 as written -> (region_start, region_end, sequences, left_trim, right_trim)."""
    min_len = min(len(s) for s in sequences)
    if min_len <= ideal_min_length:
        return region_start, region_end, sequences, 0, 0
    max_left = max_right = 0
    while max_left < min_len - ideal_min_length:
        if any(sequences[j][max_left] != sequences[j - 1][max_left] for j in range(1, len(sequences))):
            break
        max_left += 1
    while max_right < min_len - ideal_min_length:
        c = sequences[0][len(sequences[0]) - 1 - max_right]
        if any(s[len(s) - 1 - max_right] != c for s in sequences[1:]):
            break
        max_right += 1
    max_left, max_right = min(LEFT_PAD, max_left), min(RIGHT_PAD, max_right)
    max_left = max(0, min(min_len - RIGHT_PAD, max_left)); max_right = max(0, min(min_len - LEFT_PAD, max_right))
    if min_len - 2 * min(max_left, max_right) <= ideal_min_length:
        left = right = min(max_left, max_right)
        while min_len - left - right < ideal_min_length:
            if left > right:
                left -= 1
            else:
                right -= 1
    elif max_left > max_right:
        right = max_right; left = min(max_left, min_len - ideal_min_length - max_right)
    else:
        left = max_left; right = min(max_right, min_len - ideal_min_length - max_left)
    return region_start + left, region_end - right, [s[left:len(s) - right] for s in sequences], left, right


def restate(lc):
    """One locus -> dict(status, blocks, n_spanning, n_samples_spanning, n_distinct, left_trim, right_trim, min_aln_start, max_aln_stop,
    ext=[(off, len) per read, (-1, -1) = not counted], dist=[(len, rep, reads, strong, frac) in (length, bytes) order])."""
    reads, chrom = lc["reads"], lc["chrom"]
    min_all = min([INT_MAX] + [r["start"] for r in reads]); max_all = max([INT_MIN] + [r["stop"] for r in reads])        # :428-432
    out = dict(status=0, blocks=[], n_spanning=0, n_samples_spanning=0, n_distinct=0, left_trim=0, right_trim=0, min_aln_start=min_all, max_aln_stop=max_all,
               ext=[(-1, -1)] * len(reads), dist=[])
    a, b = lc["region_start"], lc["region_stop"]
    if a < REF_FLANK_LEN + LEFT_PAD or b + REF_FLANK_LEN + RIGHT_PAD > len(chrom):                                        # :292
        out["status"] = 1
        return out
    flagged = [r for r in reads if r["use"]]
    min_f = min([INT_MAX] + [r["start"] for r in flagged]); max_f = max([INT_MIN] + [r["stop"] for r in flagged])         # :243-254
    region_start, region_end = a - LEFT_PAD, b + RIGHT_PAD
    ref_seq = upper(chrom[region_start:region_end])
    if min_f + 5 >= region_start or max_f - 5 <= region_end:                                                             # :305, in python's integers
        out["status"] = 2
        return out
    # gen_candidate_seqs :157-241
    sample_counts, read_counts, must_inc, first = {}, {}, {}, {}
    tot_reads = tot_samples = 0
    for s in range(lc["n_samples"]):
        samp_reads, counts = 0, {}
        for i, r in enumerate(reads):
            if r["sample"] != s or not r["use"]:
                continue
            e = extract_sequence(r, region_start, region_end)
            if e is None:
                continue
            sub = upper(e[0])
            out["ext"][i] = (e[1], len(sub))
            read_counts[sub] = read_counts.get(sub, 0) + 1; counts[sub] = counts.get(sub, 0) + 1
            first[sub] = min(first.get(sub, i), i)
            tot_reads += 1; samp_reads += 1
        for k in sorted(counts):
            if counts[k] >= 2.0 and counts[k] >= 0.2 * samp_reads:
                must_inc[k] = must_inc.get(k, 0) + 1
            sample_counts[k] = sample_counts.get(k, 0.0) + counts[k] * 1.0 / samp_reads
        if samp_reads > 0:
            tot_samples += 1
    key = lambda s: (len(s), s.encode("latin-1"))
    out["dist"] = [(len(k), first[k], read_counts[k], must_inc.get(k, 0), sample_counts[k]) for k in sorted(read_counts, key=key)]
    out["n_spanning"], out["n_samples_spanning"], out["n_distinct"] = tot_reads, tot_samples, len(read_counts)
    sequences, ref_index = [], -1
    sc, rc = dict(sample_counts), dict(read_counts)
    for k in sorted(must_inc):                                          # :207-217 (std::map order)
        if must_inc[k] >= 1:
            del sc[k]; del rc[k]
            sequences.append(k)
            if k == ref_seq:
                ref_index = len(sequences) - 1
    for k in sorted(sc):                                                # :220-226
        if sc[k] > 0.05 * tot_samples or rc[k] > 0.05 * tot_reads:
            sequences.append(k)
            if ref_index == -1 and k == ref_seq:
                ref_index = len(sequences) - 1
    if ref_index == -1:
        sequences.insert(0, ref_seq)
    else:
        sequences[ref_index] = sequences[0]; sequences[0] = ref_seq
    sequences[1:] = sorted(sequences[1:], key=key)                     # :237
    region_start, region_end, sequences, out["left_trim"], out["right_trim"] = trim(3 * lc["period"], region_start, region_end, sequences)
    # fuse_haplotype_blocks :339-366
    min_start = min(region_start - 10, max(region_start - REF_FLANK_LEN, min_all)); max_stop = max(region_end + 10, min(region_end + REF_FLANK_LEN, max_all))
    out["blocks"] = [(min_start, region_start, [upper(chrom[min_start:region_start])]), (region_start, region_end, sequences),
                     (region_end, max_stop, [upper(chrom[region_end:max_stop])])]
    return out


# ====================================================================================================== the library's side
class ReadsBatch:
    """A hipstr_batch_t of un-pooled reads only (the haplotype arrays stay NULL), from a list of loci."""

    def __init__(self, loci, lead_reads=0):
        """lead_reads: that many reads in front of read_off[0] that belong to no locus."""
        i32 = lambda x: np.ascontiguousarray(np.array(x, np.int32))
        reads = [dict(start=0, stop=4, cigar=[("=", 4)], seq="ACGT", sample=0, use=True)] * lead_reads + [r for lc in loci for r in lc["reads"]]
        read_off = [lead_reads]
        for lc in loci:
            read_off.append(read_off[-1] + len(lc["reads"]))
        bases = "".join(r["seq"] for r in reads)
        self.a = a = dict(read_off=i32(read_off), base_off=i32(np.concatenate([[0], np.cumsum([len(r["seq"]) for r in reads])])),
                          bases=bases.encode("latin-1") + b"\0", quals="".join(r.get("qual", "F" * len(r["seq"])) for r in reads).encode("latin-1") + b"\0", read_start=i32([r["start"] for r in reads] or [0]),
                          cigar_off=i32(np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in reads])])),
                          cigar_op="".join(op for r in reads for op, _ in r["cigar"]).encode() + b"\0",
                          cigar_len=i32([n for r in reads for _, n in r["cigar"]] or [0]))
        s = capi.HipstrBatch()
        s.n_loci = len(loci)
        for k in ("read_off", "base_off", "read_start", "cigar_off", "cigar_len"):
            setattr(s, k, a[k].ctypes.data_as(capi._i32p))
        s.bases, s.quals, s.cigar_op = a["bases"], a["quals"], a["cigar_op"]
        s._keepalive = a
        self.struct = s
        self.n_reads = len(reads) - lead_reads
        self.lead = lead_reads

    @property
    def ptr(self):
        import ctypes as C
        return C.byref(self.struct)


def window_of(lc):
    if "window" in lc:
        return lc["window"].encode("latin-1")
    a, b = lc["region_start"], lc["region_stop"]
    return lc["chrom"][a - 40:b + 40].encode("latin-1") if a >= 40 else b""


def request_of(loci, lead_reads=0, give_stop=True, stutter=True):
    """The request of a list of loci; a locus may bring its own "window", "chrom_len" and "stutter" instead of a chromosome."""
    reads = [r for lc in loci for r in lc["reads"]]
    lead = [0] * lead_reads
    return capi.HapgenRequest([lc["region_start"] for lc in loci], [lc["region_stop"] for lc in loci], [lc["period"] for lc in loci],
                              [lc.get("chrom_len", len(lc.get("chrom", ""))) for lc in loci], [window_of(lc) for lc in loci], [lc["n_samples"] for lc in loci],
                              lead + [r["sample"] for r in reads], read_stop=(lead + [r["stop"] for r in reads]) if give_stop else None,
                              use_read=(([1] * lead_reads) + [1 if r["use"] else 0 for r in reads]), stutter=[x for lc in loci for x in lc.get("stutter", STUTTER)] if stutter else None)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def expectation(loci, base_read=0):
    """restate() of every locus in run_hapgen's shape; dist_rep counts from the batch's read 0 (base_read: reads in front of the first locus)."""
    g = dict(status=[], blk_start=[], blk_end=[], blk_nopts=[], options=[], n_spanning=[], n_samples_spanning=[], n_distinct=[], left_trim=[], right_trim=[],
             min_aln_start=[], max_aln_stop=[], ext_off=[], ext_len=[], dist_len=[], dist_rep=[], dist_reads=[], dist_strong=[], dist_frac=[])
    r0 = base_read
    for lc in loci:
        e = restate(lc)
        for k in ("status", "n_spanning", "n_samples_spanning", "n_distinct", "left_trim", "right_trim", "min_aln_start", "max_aln_stop"):
            g[k].append(e[k])
        blocks = e["blocks"] or [(0, 0, [])] * 3
        for s, t, opts in blocks:
            g["blk_start"].append(s); g["blk_end"].append(t); g["blk_nopts"].append(len(opts))
            g["options"] += [o.encode("latin-1") for o in opts]
        g["ext_off"] += [x[0] for x in e["ext"]]; g["ext_len"] += [x[1] for x in e["ext"]]
        for ln, rep, n, strong, frac in e["dist"]:
            g["dist_len"].append(ln); g["dist_rep"].append(r0 + rep); g["dist_reads"].append(n); g["dist_strong"].append(strong); g["dist_frac"].append(frac)
        r0 += len(lc["reads"])
    return g


INT_KEYS = ("status", "blk_start", "blk_end", "blk_nopts", "n_spanning", "n_samples_spanning", "n_distinct", "left_trim", "right_trim", "min_aln_start",
            "max_aln_stop", "ext_off", "ext_len", "dist_len", "dist_rep", "dist_reads", "dist_strong")


def assert_result(got, want, what=""):
    """got: capi.run_hapgen's dict; want: expectation()'s.  dist_frac as bits."""
    for k in INT_KEYS:
        if k in got:
            assert got[k].tolist() == list(want[k]), (what, k)
    assert got["options"] == want["options"], what
    if "dist_frac" in got:
        assert [f64_bits(x) for x in got["dist_frac"]] == [f64_bits(x) for x in want["dist_frac"]], (what, "dist_frac")
    assert got["untouched"], what


def assert_same(got, other, what=""):
    """Two run_hapgen results (device and host twin): every output, dist_frac as bits."""
    for k in INT_KEYS + ("opt_off",):
        assert (k in got) == (k in other) and (k not in got or np.array_equal(got[k], other[k])), (what, k)
    assert got["seq"] == other["seq"] and got["options"] == other["options"], what
    assert got["dist_frac"].view(np.uint64).tolist() == other["dist_frac"].view(np.uint64).tolist(), what
    assert got["untouched"] and other["untouched"], what


def blocks_of(got, l):
    """The three blocks of locus l of a run_hapgen result as the golden records hold them."""
    o0 = int(got["blk_nopts"][:3 * l].sum())
    out = []
    for k in range(3):
        n = int(got["blk_nopts"][3 * l + k])
        out.append((int(got["blk_start"][3 * l + k]), int(got["blk_end"][3 * l + k]), [x.decode("latin-1") for x in got["options"][o0:o0 + n]]))
        o0 += n
    return out


def cap_locus(rng, n_reads, n_samples=1, n_alleles=4):
    """n_reads short spanning reads (34 bases) of a 3-base homopolymer locus, a handful of alleles: for the edges of the caps."""
    chrom, a, b = chrom_with_repeat(rng, 60, "A", 3, tail=60)
    rs, re = a - LEFT_PAD, b + RIGHT_PAD
    alleles = [[], [("X", 6)], [("D", 6, 1)], [("I", 6, 1)], [("X", 5)], [("X", 7)]][:n_alleles]
    reads = [padded_read(chrom, rs, re, alleles[int(rng.integers(0, len(alleles)))], start=rs - 10 - (k % 3), end=re + 11, sample=k % n_samples) for k in range(n_reads)]
    return locus("cap_%d_reads_%d_samples" % (n_reads, n_samples), chrom, a, b, 1, n_samples, reads)


def many_distinct_locus(rng, n_distinct):
    """n_distinct strings (substitutions at two of 30 positions of a long repeat), each carried by the two reads of a sample of its own: every
    one is strong there, so the repeat block gets n_distinct + 1 options."""
    chrom, a, b = chrom_with_repeat(rng, 60, "ACGT", 8, tail=60)
    rs, re = a - LEFT_PAD, b + RIGHT_PAD
    pairs = [(i, j) for i in range(6, 36) for j in range(i + 1, 36)][:n_distinct]
    assert len(pairs) == n_distinct
    reads = [padded_read(chrom, rs, re, [("X", i), ("X", j)], start=rs - 10 - rep, end=re + 10, sample=k) for rep in range(2) for k, (i, j) in enumerate(pairs)]
    return locus("distinct_%d" % n_distinct, chrom, a, b, 4, n_distinct, reads)
