"""Cases of hipstr_record_alleles (include/hipstr_hmm.h): the makers, the text integration/genotype_flow.cpp's --record-cases mode reads,
the golden's loader and the Python restatement of the flank option strings (seq_stutter_genotyper.cpp:1013-1040: no reference binary
prints them).  tests/golden/record_alleles_unit.npz and record_alleles_random.npz hold what the compiled reference's get_alleles and
reorder_alleles returned on exactly these cases (tests/golden/make_golden_record_alleles.py).

A case is a dict: name, region_start, region_stop, blocks = three (start, end, [option bytes]); the chromosome is CHROM from base 0."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = {b: os.path.join(ROOT, "tests", "golden", "record_alleles_%s.npz" % b) for b in ("unit", "random")}
WIN_PAD = 40
DEVICE_OPTIONS = 256
_rng = np.random.default_rng(1)
CHROM = bytes(_rng.choice(list(b"ACGT"), size=500).tolist())
CHROM = CHROM[:120] + CHROM[120:200].lower() + CHROM[200:]              # the window may come in any case
REF = CHROM.upper()
DUPLICATE, OUTSIDE, FLANK_ASSERT = 1, 2, 4


def case(name, rs, re_, start, end, opts, lstart=None, lopts=None, ropts=None):
    lstart = start - 8 if lstart is None else lstart
    return dict(name=name, region_start=rs, region_stop=re_,
                blocks=[(lstart, start, lopts or [REF[max(lstart, 0):start], REF[max(lstart, 0):start - 1] + b"N"]), (start, end, list(opts)),
                        (end, end + 8, ropts or [REF[end:end + 8], b"N" + REF[end + 1:end + 8]])])


def unit_cases():
    R = REF[150:170]
    c = []
    c.append(case("v1", 150, 170, 150, 170, [R]))
    c.append(case("v2", 150, 170, 150, 170, [R, R + b"AC"]))
    c.append(case("v65", 150, 170, 150, 170, [R] + [R + b"AC" * (k // 2) + (b"A" if k % 2 else b"") + bytes([b"ACGT"[k % 4]]) for k in range(1, 65)]))
    # the block begins 10 bases before the region, the options share 15: the trim stops at the region's edge
    P = REF[140:155]
    c.append(case("trim_to_region_edge", 150, 170, 140, 172, [P + b"ACACAC" + REF[161:172], P + b"ACAC" + REF[161:172], P + b"TTACACAC" + REF[161:172]]))
    # an option of four bases: the trim stops at three, before the region
    c.append(case("trim_stopped_by_short_option", 150, 170, 140, 170, [REF[140:170], REF[140:144], REF[140:150] + b"TT"]))
    # the same from the right: the block ends behind the region, a common suffix longer than the gap / an option that would be left with one base
    S = REF[165:180]
    c.append(case("right_trim_to_region_edge", 150, 170, 150, 180, [REF[150:160] + b"GTGT" + S, REF[150:160] + S, REF[150:160] + b"GTGTGTA" + S]))
    c.append(case("right_trim_stopped_by_short_option", 150, 170, 150, 180, [REF[150:180], REF[176:180], b"CC" + REF[170:180]]))
    # a block inside the region: both flanks come from the window (lower case there)
    c.append(case("left_flank_from_window", 150, 170, 156, 170, [REF[156:170], REF[156:170] + b"AG"]))
    c.append(case("right_flank_before_region_stop", 150, 170, 150, 163, [REF[150:163], REF[150:163] + b"AG", REF[150:161]]))
    c.append(case("both_flanks", 150, 190, 158, 181, [REF[158:181], b"T" + REF[158:181], REF[160:181]]))
    # the pad: an empty option; options that differ in their first base
    c.append(case("empty_option", 150, 170, 150, 170, [R, b""]))
    c.append(case("first_bases_differ", 150, 170, 150, 170, [b"ACACAC", b"GCACAC", b"ACACACAC"]))
    c.append(case("pad_after_trim_before_region", 150, 170, 140, 170, [REF[140:170], REF[140:143] + b"T" + REF[145:170], REF[140:143]]))
    # equal lengths that differ only late; bytes compared as unsigned (0xC8 sorts behind every letter, not before)
    c.append(case("late_byte_compare", 150, 170, 150, 170, [b"ACACACACAC", b"ACACACACAT", b"ACACACACAG", b"ACACACACAA", b"ACACATACAC"]))
    c.append(case("unsigned_bytes", 150, 170, 150, 170, [b"ACAC", b"A\xc8AC", b"AzAC", b"A\x80AC", b"ATAC"]))
    # refusals: two equal strings; a pad that lies before the window
    c.append(case("duplicate_strings", 150, 170, 150, 170, [b"ACAC", b"ACAT", b"ACACAC", b"ACAT"]))
    c.append(case("pad_before_window", 150, 170, 105, 170, [b"A" + REF[106:170], b"G" + REF[106:170]]))
    # flanks of the record that the haplotype data cannot take: a right flank makes the right trim negative
    c.append(case("region_far_wider_than_block", 120, 200, 150, 170, [R, R[:-2]]))
    return c


def random_cases(seed=3, n=60):
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        rs = int(r.integers(100, 300)); re_ = rs + int(r.integers(6, 50))
        start = rs + int(r.integers(-12, 5)); end = re_ + int(r.integers(-4, 13))
        end = max(end, start + 2)
        pre = REF[start:start + int(r.integers(0, 16))]; suf = REF[max(start + len(pre), end - int(r.integers(0, 16))):end]
        V = int(r.integers(1, 9)) if k % 10 else int(r.integers(60, 140))
        mids = set()
        while len(mids) < V:
            mids.add(bytes(r.choice(list(b"ACGT"), size=int(r.integers(0, 9) if V < 20 else r.integers(3, 9))).tolist()))
        mids = sorted(mids); r.shuffle(mids)
        out.append(case("random_%d" % k, rs, re_, start, end, [pre + m + suf for m in mids]))
    return out


def beyond_cap_case():
    """More options than a wavefront ranks: the host twin inside the device call."""
    return case("v300", 150, 170, 146, 174, [REF[146:152] + b"AC" * (k // 4) + bytes([b"ACGT"[k % 4]]) + b"T" * (k % 3) + REF[168:174] for k in range(300)])


def no_reference_cases():
    """Cases the compiled reference cannot be given: its substr throws where the pad lies before base 0."""
    return [case("pad_before_base_0", 10, 30, 0, 30, [b"A" + REF[1:30], b"G" + REF[1:30]], lstart=0, lopts=[b"A"])]


BATCHES = {"unit": unit_cases, "random": random_cases}


def locus_of(c):
    """The arguments of hipstr_amd.capi.run_record_alleles for a case."""
    w0 = c["region_start"] - WIN_PAD
    window = b"." * max(0, -w0) + CHROM[max(0, w0):max(0, c["region_stop"] + WIN_PAD)]
    return dict(region_start=c["region_start"], region_stop=c["region_stop"], window=window, blocks=c["blocks"])


def cases_text(cases):
    show = lambda s: s.decode("latin-1") if s else "-"
    out = []
    for c in cases:
        out.append("case %s %d %d\nchrom %s\n" % (c["name"], c["region_start"], c["region_stop"], CHROM.decode()))
        for b, (st, en, opts) in enumerate(c["blocks"]):
            out.append("block %d %d %d %d %s\n" % (b, st, en, len(opts), " ".join(show(o) for o in opts)))
    return "".join(out)


def parse_results(text):
    """The driver's output -> {name: dict(pos, left_trim, right_trim, alleles, old_to_new, new_to_old)}."""
    out = {}; cur = None
    for line in text.split("\n"):
        w = line.split(" ")
        if w[0] == "case":
            cur = out.setdefault(w[1], {})
        elif w[0] == "pos":
            cur["pos"] = int(w[1])
        elif w[0] == "trim":
            cur["left_trim"], cur["right_trim"] = int(w[1]), int(w[2])
        elif w[0] == "alleles":
            cur["alleles"] = [b"" if s == "-" else s.encode("latin-1") for s in w[2:]]
            assert len(cur["alleles"]) == int(w[1])
        elif w[0] in ("old_to_new", "new_to_old"):
            cur[w[0]] = [int(x) for x in w[1:]]
    return out


def golden(batch):
    return parse_results(np.load(GOLDEN[batch])["text"].tobytes().decode("latin-1"))


def flanks_restated(c, left_trim, right_trim):
    """seq_stutter_genotyper.cpp:1013-1040 -> (lflanks, rflanks), or None where an assert fires or substr(trim) throws."""
    ref = c["blocks"][1][2][0]; n = len(ref)
    if not (left_trim < n and right_trim < n and left_trim + right_trim < n):                  # :1015-1016
        return None
    lf = []; rf = []
    for s in c["blocks"][0][2]:
        if not len(s) + left_trim > 0:                                                         # :1023
            return None
        lf.append(s[:len(s) + left_trim] if left_trim < 0 else s + ref[:left_trim])
    for s in c["blocks"][2][2]:
        if not len(s) + right_trim > 0:                                                        # :1035
            return None
        if right_trim < 0:                                                                     # :1037: substr(trim) with a negative int throws
            return None
        rf.append(ref[n - right_trim:] + s)
    return lf, rf
