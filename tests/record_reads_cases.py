"""Cases of the record's per-read sizes and per-sample histograms (hipstr_cigar_bp_diffs, hipstr_sample_histograms,
hipstr_em_batch_from_bp_diffs; include/hipstr_hmm.h): the makers, the text the golden driver reads, the goldens' loaders and the Python
restatement of learn_stutter_model's read loop.  The goldens (tests/golden/record_reads_cigars.npz, record_reads_histograms.npz) hold what
the compiled reference's ExtractCigar and condense_read_counts returned on exactly these cases (tests/golden/make_golden_record_reads.py).

A CIGAR locus is (region_start, region_stop, pad, reads), a read (start, [(op letter, length), ...]) — hipstr_amd.capi.cigar_request's input.
A histogram locus is a list of samples, a sample the list of its reads' values; SKIP marks a read that does not count."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_CIGARS = os.path.join(ROOT, "tests", "golden", "record_reads_cigars.npz")
GOLDEN_HISTOGRAMS = os.path.join(ROOT, "tests", "golden", "record_reads_histograms.npz")
SKIP = -2 ** 31                         # HIPSTR_NO_ML_BP
CIGAR_DEVICE_RUNS = 4096
HISTOGRAM_DEVICE_READS = 1024
OPS = "MIDNSHP=X"


# ------------------------------------------------------------------------------------------------------------------ CIGARs
def cigar_unit_loci():
    """Named cases; every locus' comment says what its reads are there for (line numbers: extract_indels.cpp)."""
    M50 = [("M", 50)]
    loci = []
    # a single-run CIGAR at 100..149; the padded region touches each boundary test (:39-40) from either side by one base
    loci.append((102, 147, 2, [(100, M50), (101, M50), (99, [("M", 52)])]))         # region' 100..149: start == / > / < the region's start
    loci.append((110, 140, 9, [(100, M50), (99, M50), (98, M50), (101, M50)]))      # region' 101..149: the read ends one base behind it, with it, before it; starts with it
    loci.append((120, 130, 0, [(100, M50), (100, [("=", 20), ("X", 5), ("=", 25)])]))
    # a leading I with the region at the read's start: the start walk does not run, run 0 is no match (:54-58)
    loci.append((100, 120, 0, [(100, [("I", 5), ("M", 50)]), (100, [("S", 5), ("M", 50)]), (100, [("M", 50), ("I", 5)]), (99, [("I", 5), ("M", 50)])]))
    # a trailing I behind a deletion that holds the region's end: the end walk meets no match (:76-80); a trailing S or H behind a match does
    loci.append((110, 145, 0, [(100, [("M", 40), ("D", 10), ("I", 5)]), (100, [("M", 40), ("D", 10), ("S", 5)]), (100, [("M", 40), ("D", 10), ("M", 1)]),
                               (100, [("M", 50), ("S", 5), ("H", 3)]), (100, [("M", 40), ("D", 6), ("I", 2), ("M", 4), ("I", 5)])]))
    # the start walk's last_match_index staying 0: deletions and skips only before the region, run 0 a match / no match
    loci.append((130, 140, 0, [(100, [("M", 10), ("D", 30), ("M", 20)]), (100, [("D", 40), ("M", 20)]), (100, [("N", 5), ("D", 40), ("M", 20)]),
                               (100, [("H", 2), ("S", 3), ("M", 60)]), (100, [("S", 3), ("M", 10), ("N", 4), ("M", 50)])]))
    # indels inside, outside and straddling the padded region 118..142
    ins_in = [("M", 25), ("I", 4), ("M", 30)]; del_in = [("M", 25), ("D", 6), ("M", 30)]
    loci.append((120, 140, 2, [(100, ins_in), (100, del_in),
                               (100, [("M", 5), ("I", 3), ("M", 60)]), (100, [("M", 5), ("D", 3), ("M", 60)]),           # before it, inside the first match
                               (100, [("M", 16), ("D", 4), ("M", 40)]), (100, [("M", 17), ("D", 4), ("M", 40)]),        # a deletion ending at / crossing the start
                               (100, [("M", 18), ("I", 4), ("M", 40)]), (100, [("M", 19), ("I", 4), ("M", 40)]),        # an insertion at the first base / one inside
                               (100, [("M", 40), ("D", 5), ("M", 20)]), (100, [("M", 42), ("D", 5), ("M", 20)]), (100, [("M", 43), ("D", 5), ("M", 20)]),
                               (100, [("M", 42), ("I", 5), ("M", 20)]), (100, [("M", 43), ("I", 5), ("M", 20)]), (100, [("M", 44), ("I", 5), ("M", 20)]),
                               (100, [("S", 10), ("M", 20), ("I", 2), ("M", 8), ("D", 3), ("M", 10), ("N", 100), ("M", 20), ("H", 4)]),
                               (100, [("M", 20), ("P", 2), ("I", 2), ("M", 40)]), (0, [("M", 200)]), (118, [("M", 25)]), (118, [("M", 24)])]))
    # first > last: the region lies inside a deletion between two matches
    loci.append((125, 128, 0, [(100, [("M", 20), ("D", 20), ("M", 20)]), (100, [("M", 20), ("I", 7), ("D", 20), ("I", 9), ("M", 20)])]))
    # a locus without reads, and a region at the chromosome's start with a pad that takes it below 0
    loci.append((50, 60, 3, []))
    loci.append((1, 9, 4, [(0, M50), (0, [("I", 2), ("M", 50)])]))
    # reads with more runs than a lane takes: the host twin inside the device call
    many = [("M", 2), ("I", 1), ("M", 1), ("D", 1)] * 1100
    loci.append((2000, 2100, 4, [(100, many), (100, M50 * 40 + [("I", 3)] + M50 * 10), (100, many[:CIGAR_DEVICE_RUNS]), (100, many[:CIGAR_DEVICE_RUNS + 1])]))
    return loci


def cigar_fuzz_loci(seed, n_loci=40, max_reads=24):
    rng = np.random.default_rng(seed)
    loci = []
    for _ in range(n_loci):
        rs = int(rng.integers(50, 400)); re_ = rs + int(rng.integers(0, 60)); pad = int(rng.integers(0, 7))
        reads = []
        for _ in range(int(rng.integers(0, max_reads + 1))):
            n = int(rng.integers(1, 9))
            w = [6, 2, 2, .5, 1, .5, .3, 1, 1]
            ops = rng.choice(len(OPS), size=n, p=np.asarray(w) / sum(w))
            runs = [(OPS[o], int(rng.integers(1, 70) if OPS[o] in "M=X" else rng.integers(1, 12))) for o in ops]
            start = max(0, rs - pad - int(rng.integers(-3, 90)))
            reads.append((start, runs))
        loci.append((rs, re_, pad, reads))
    return loci


def cigar_loci():
    return cigar_unit_loci() + cigar_fuzz_loci(20261)


def cigar_text(loci):
    """One line per read for the golden driver: C start region_start' region_end' n (op len)*."""
    out = []
    for rs, re_, pad, reads in loci:
        for start, runs in reads:
            out.append("C %d %d %d %d %s\n" % (start, rs - pad, re_ + pad, len(runs), " ".join("%s %d" % r for r in runs)))
    return "".join(out)


def cigar_golden():
    z = np.load(GOLDEN_CIGARS)
    return z["got"], z["bp_diff"]


# ------------------------------------------------------------------------------------------------------------------ histograms
def histogram_unit_loci():
    r = np.random.default_rng(7)
    vals = lambda n, lo=-12, hi=13: [int(x) for x in r.integers(lo, hi, size=n)]
    loci = []
    loci.append([[], [3], vals(64), vals(65), [], [5] * 40, [-4, 9, -4, 0, 9, -4, -1, 1]])                 # 0, 1, 64, 65 values; all equal; signs mixed
    loci.append([[SKIP] * 3, [SKIP], [2, SKIP, 2, SKIP, SKIP, -7, 2], [SKIP, 1], [1, SKIP]])                # sentinel only; skipped reads between kept ones
    loci.append([[2 ** 31 - 1, -2 ** 31 + 1, 0, -1, 2 ** 31 - 1], [SKIP + 1, SKIP, SKIP + 1]])              # the ends of int32 beside the sentinel
    loci.append([])                                                                                         # a locus without samples
    loci.append([[], [], []])                                                                               # samples without reads
    loci.append([vals(63), vals(127), vals(128), vals(129), list(range(200, 0, -1)), [SKIP if i % 3 else i % 7 for i in range(300)]])
    # around the cap of a wavefront's LDS, and far beyond it: the host twin inside the device call
    loci.append([vals(HISTOGRAM_DEVICE_READS, -40, 40), vals(5), vals(HISTOGRAM_DEVICE_READS + 1, -40, 40), [], vals(3000, -300, 300), vals(9),
                 [SKIP] * (HISTOGRAM_DEVICE_READS + 5), vals(HISTOGRAM_DEVICE_READS - 1, -3, 3)])
    return loci


def histogram_fuzz_loci(seed, n_loci=30, max_samples=12, max_reads=90):
    r = np.random.default_rng(seed)
    loci = []
    for _ in range(n_loci):
        spread = int(r.integers(1, 30))
        samples = []
        for _ in range(int(r.integers(0, max_samples + 1))):
            n = int(r.integers(0, max_reads + 1)) if r.random() < 0.8 else 0
            v = r.integers(-spread, spread + 1, size=n)
            samples.append([SKIP if r.random() < 0.15 else int(x) for x in v])
        loci.append(samples)
    return loci


def histogram_loci():
    return histogram_unit_loci() + histogram_fuzz_loci(20262)


def histogram_arrays(loci):
    """-> dict(n_samples, read_off, sample_label, value) of a list of histogram loci."""
    n_samples = [len(l) for l in loci]; read_off = [0]; label = []; value = []
    for l in loci:
        for s, v in enumerate(l):
            label += [s] * len(v); value += v
        read_off.append(len(value))
    return dict(n_samples=np.asarray(n_samples, np.int32), read_off=np.asarray(read_off, np.int32), sample_label=np.asarray(label, np.int32),
                value=np.asarray(value, np.int64).astype(np.int32))


def post_batch(capi, a, log_p=None):
    """The PostBatch of such arrays (one haplotype per locus: only the sample layout matters here)."""
    n = len(a["sample_label"])
    lp1, lp2 = (np.zeros(n), np.zeros(n)) if log_p is None else log_p
    return capi.PostBatch(n_alleles=np.ones(len(a["n_samples"]), np.int32), n_samples=a["n_samples"], read_off=a["read_off"], sample_label=a["sample_label"],
                          log_p1=lp1, log_p2=lp2, read_weight=np.ones(n, np.int32), log_aln_probs=np.zeros(n))


def histogram_text(loci):
    """One line per sample for the golden driver: H n (value)* — the values that count, in read order."""
    out = []
    for l in loci:
        for v in l:
            kept = [x for x in v if x != SKIP]
            out.append("H %d %s\n" % (len(kept), " ".join(str(x) for x in kept)))
    return "".join(out)


def histogram_golden():
    """The reference's strings, one per sample."""
    return np.load(GOLDEN_HISTOGRAMS)["condensed"].tobytes().decode().split("\n")


def pairs_of_string(s):
    """condense_read_counts' text -> [(value, count)]."""
    return [] if s == "." else [tuple(int(x) for x in kv.split("|")) for kv in s.split(";")]


# ------------------------------------------------------------------------------------------------------------------ the EM's reads
def em_batch_restated(a, got, bp_diff, region_start, region_stop, min_total_reads, log_p=None):
    """genotyper_bam_processor.cpp:113-139 on the arrays of histogram_arrays (value unused)."""
    MAX_INF_READS = 10000
    ro = [0]; label = []; bps = []; p1 = []; p2 = []; few = []
    for l, S in enumerate(a["n_samples"].tolist()):
        r0, r1 = int(a["read_off"][l]), int(a["read_off"][l + 1])
        inf = 0
        for i in range(S):                                          # :114
            for r in range(r0, r1):
                if a["sample_label"][r] != i or not got[r]:         # :118
                    continue
                if bp_diff[r] < -(int(region_stop[l]) - int(region_start[l]) + 1):      # :119
                    continue
                inf += 1                                            # :121
                label.append(i); bps.append(int(bp_diff[r]))
                p1.append(0.0 if log_p is None else log_p[0][r]); p2.append(0.0 if log_p is None else log_p[1][r])
            if inf > MAX_INF_READS:                                 # :131
                break
        few.append(1 if inf < min_total_reads else 0)               # :135
        ro.append(len(label))
    return dict(read_off=np.asarray(ro, np.int32), sample_label=np.asarray(label, np.int32), num_bps=np.asarray(bps, np.int32),
                log_p1=np.asarray(p1, np.float64), log_p2=np.asarray(p2, np.float64), too_few=np.asarray(few, np.uint8))
