"""Cases of the record-field tests (tests/test_record_host.py, tests/test_record_gpu.py, tests/test_record_chain_gpu.py) and of
tests/golden/make_record_golden.py: the index rules of the p-value golden, the seeded batches of hipstr_record_fields, and the numpy
restatement of write_vcf_record's three sample loops (seq_stutter_genotyper.cpp:1159-1187, :1238-1254, :1326-1375)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "record_pvalues.npz")
NOT_APPLICABLE = 1.01
PASS, NO_READS, MASKED, FLANK_INDEL_FRAC, NOT_REPORTED = 0, 1, 2, 3, -1
TABLE_READS = 5000


# ---- the golden's inputs.  The fixture holds results only (uint64 bit patterns): ab_small[i], fs_small[i], ab_large[i], fs_large[i].
def ab_small():
    """(a) every count pair 0..24 x 0..24: one = i // 25, two = i % 25."""
    i = np.arange(25 * 25)
    return (i // 25).astype(np.int32), (i % 25).astype(np.int32)


def fs_small():
    """(b) every 2x2 table with cells 0..12: n11 = i // 2197, n12 = i // 169 % 13, n21 = i // 13 % 13, n22 = i % 13 — as the quadruple
    (uniq_one, uniq_two, rv_uniq_one, rv_uniq_two) = (n11 + n12, n21 + n22, n12, n22)."""
    i = np.arange(13 ** 4)
    n11, n12, n21, n22 = i // 2197, i // 169 % 13, i // 13 % 13, i % 13
    return tuple(x.astype(np.int32) for x in (n11 + n12, n21 + n22, n12, n22))


def large():
    """(c) quadruples (uniq_one, uniq_two, rv_uniq_one, rv_uniq_two), AB and FS of each: totals around 171 (cephes' MAXGAM: the gamma
    branch against the log branch), k = min in {0, 1, 2} (pow and the power series), n = 2k + 1 (the second continued fraction),
    totals to 5000 and cells to 2500, and a few totals beyond the device's table."""
    rng = np.random.RandomState(20261020)
    pairs = []
    for n in range(165, 177):
        pairs += [(k, n - k) for k in (1, 3, n // 3, (n - 1) // 2)]
    for n in (1, 2, 3, 5, 10, 50, 169, 170, 171, 172, 500, 1000, 1074, 1075, 1100, 5000):
        pairs += [(k, n - k) for k in (0, 1, 2) if n - k > k]
    pairs += [(k, k + 1) for k in (1, 2, 3, 4, 10, 50, 84, 85, 86, 200, 1000, 2499)]
    for _ in range(150):
        n = int(rng.randint(200, TABLE_READS + 1))
        w = int(3 * np.sqrt(n))
        a = int(np.clip(n // 2 + rng.randint(-w, w + 1), 0, n))
        pairs.append((a, n - a))
    pairs += [(2500, 2501), (2000, 4000), (4000, 6000), (5000, 5001)]      # beyond the table
    q = []
    for k, (a, b) in enumerate(pairs):
        if k % 2:
            a, b = b, a
        if k % 3 == 0:      # reverse reads near half of each: the table close to the mode
            r1, r2 = a // 2 + (k % 5), b // 2 - (k % 7)
            r1, r2 = min(max(r1, 0), a), min(max(r2, 0), b)
        else:
            r1, r2 = int(rng.randint(0, a + 1)), int(rng.randint(0, b + 1))
        q.append((a, b, r1, r2))
    q += [(2500, 2500, 1250, 1250), (2500, 2500, 0, 2500), (2500, 2500, 2500, 0), (2500, 2500, 1200, 1300), (5000, 0, 2500, 0), (0, 5000, 0, 2500)]
    q = np.array(q, np.int32)
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy(), q[:, 3].copy()


def golden():
    z = np.load(GOLDEN)
    return {k: z[k].view(np.float64) for k in ("ab_small", "fs_small", "ab_large", "fs_large")}


def all_quadruples():
    """The whole golden as one batch of quadruples with the golden's values: (u1, u2, rv1, rv2, ab or None-mask, fs or None-mask).
    The AB-only pairs carry rv = 0 and the FS-only tables are complete quadruples (their AB is not in the golden)."""
    g = golden()
    a1, a2 = ab_small()
    f = fs_small()
    L = large()
    z = np.zeros_like(a1)
    u1 = np.concatenate([a1, f[0], L[0]]); u2 = np.concatenate([a2, f[1], L[1]])
    r1 = np.concatenate([z, f[2], L[2]]); r2 = np.concatenate([z, f[3], L[3]])
    nan = np.full(len(f[0]), np.nan)
    ab = np.concatenate([g["ab_small"], nan, g["ab_large"]])
    fs = np.concatenate([np.full(len(a1), np.nan), g["fs_small"], g["fs_large"]])
    return u1, u2, r1, r2, ab, fs


def ulps(a, b):
    """Distance in units of the last place between finite doubles of equal sign (or zeros)."""
    ia, ib = a.view(np.int64).copy(), b.view(np.int64).copy()
    ia[ia < 0] = np.int64(-2 ** 63) - ia[ia < 0]
    ib[ib < 0] = np.int64(-2 ** 63) - ib[ib < 0]
    return np.abs(ia - ib)


# ---- hipstr_record_fields: seeded batches of 3 loci x 7 samples
class Batch(object):
    pass


def fields_batch(seed, haploid_locus=1, one_variant_locus=2):
    """3 loci x 7 samples.  Per locus the samples walk through every combination of not reported / no reads / masked / over the
    fraction (16 samples of every batch; the other five pass), locus `haploid_locus` is
    haploid (its MAP pairs homozygous), locus `one_variant_locus` has one variant; MAP pairs hom and het; n_aligned a multiple of 20
    with n_flank_indel = 3*n_aligned/20 exactly (0.15f*n against 0.15*n: the float comparison) and one read more."""
    rng = np.random.RandomState(1000 + seed)
    b = Batch()
    b.n_loci, S = 3, 7
    b.n_samples = np.full(3, S, np.int32)
    b.n_alleles = np.array([5, 4, 3], np.int32)
    b.haploid = np.zeros(3, np.uint8); b.haploid[haploid_locus] = 1
    b.n_variants = np.array([3, 2, 2], np.int32); b.n_variants[one_variant_locus] = 1
    h2a = []
    for l in range(3):
        A, V = int(b.n_alleles[l]), int(b.n_variants[l])
        m = np.concatenate([np.arange(V), rng.randint(0, V, A - V)]).astype(np.int32)
        h2a.append(m)
    b.hap_to_allele = np.concatenate(h2a)
    n = 3 * S
    b.n_samp = n
    b.map_gt = np.zeros((n, 2), np.int32)
    b.reported = np.ones(n, np.uint8); b.masked = np.zeros(n, np.uint8)
    b.n_aligned = np.zeros(n, np.int32); b.n_flank_indel = np.zeros(n, np.int32)
    for l in range(3):
        A = int(b.n_alleles[l])
        for s in range(S):
            i = l * S + s
            c = (seed * 5 + i) % 16 if i < 16 else 0          # sixteen samples walk through the combinations, five more pass
            b.reported[i] = 0 if c & 1 else 1
            no_reads, b.masked[i], over = bool(c & 2), 1 if c & 4 else 0, bool(c & 8)
            na = 0 if no_reads else 20 * int(rng.randint(1, 40))
            edge = 3 * na // 20
            b.n_aligned[i] = na
            # over the fraction: from one read above the edge; not over: up to the edge itself, the edge every other sample
            b.n_flank_indel[i] = (edge + 1 + int(rng.randint(0, 3))) if over else (edge if (i % 2 == 0) else int(rng.randint(0, edge + 1)))
            if no_reads:
                b.n_flank_indel[i] = 2 if over else 0          # flank reads without aligned reads: only :1168's n > 0 keeps them out
            ha = int(rng.randint(0, A))
            hb = ha if (b.haploid[l] or (i % 3 == 0)) else int(rng.randint(0, A))
            b.map_gt[i] = (ha, hb)
    b.n_snp = np.minimum(rng.randint(0, 50, n), b.n_aligned).astype(np.int32)
    b.n_stutter = np.minimum(rng.randint(0, 50, n), b.n_aligned).astype(np.int32)
    b.uniq_one = rng.randint(0, 60, n).astype(np.int32); b.uniq_two = rng.randint(0, 60, n).astype(np.int32)
    # among the samples whose p-values are computed (pass, diploid, MAP haplotypes differ): the empty total (ab = 1, not 1.01) and equal
    # counts (ab = 0.0)
    over = (b.n_aligned > 0) & (b.n_flank_indel > 3 * b.n_aligned // 20)
    diploid = np.repeat(b.haploid == 0, S)
    computed = np.flatnonzero(b.reported.astype(bool) & (b.n_aligned > 0) & (b.masked == 0) & ~over & diploid & (b.map_gt[:, 0] != b.map_gt[:, 1]))
    if len(computed) > 0:
        b.uniq_one[computed[0]] = b.uniq_two[computed[0]] = 0
    if len(computed) > 1:
        b.uniq_two[computed[1]] = b.uniq_one[computed[1]] = 7
    b.rv_uniq_one = (b.uniq_one * rng.rand(n)).astype(np.int32); b.rv_uniq_two = (b.uniq_two * rng.rand(n)).astype(np.int32)
    b.frac = 0.0
    return b


def expect_fields(b, pvalues):
    """The three loops, restated.  pvalues(u1, u2, rv1, rv2) -> (ab, fs) of one quadruple."""
    frac = np.float32(0.15) if b.frac == 0 else np.float32(b.frac)
    n = b.n_samp
    out = dict(status=np.zeros(n, np.int32), gt=np.zeros((n, 2), np.int32), ab=np.full(n, NOT_APPLICABLE), dab=np.zeros(n, np.int32),
               fs=np.full(n, NOT_APPLICABLE), allele_count=np.zeros(int(b.n_variants.sum()), np.int32))
    for k in ("n_skip", "n_filt", "an", "dp", "dsnp", "dstutter", "dflankindel"):
        out[k] = np.zeros(b.n_loci, np.int32)
    so = ho = vo = 0
    for l in range(b.n_loci):
        S, A, V = int(b.n_samples[l]), int(b.n_alleles[l]), int(b.n_variants[l])
        for i in range(so, so + S):
            ha, hb = (int(x) for x in b.map_gt[i])
            gts = tuple(int(b.hap_to_allele[ho + h]) if h >= 0 else -1 for h in (ha, hb))
            out["gt"][i] = gts
            na, nfi = int(b.n_aligned[i]), int(b.n_flank_indel[i])
            # MAX_FLANK_INDEL_FRAC is a float: int * float and int > float are float operations
            over = na > 0 and np.float32(nfi) > np.float32(frac * np.float32(na))
            # :1163-1187 — reported (:1164), n_aligned == 0 (:1166), the fraction (:1168-1172), THEN the mask (:1173, :1185-1186)
            if b.reported[i] and na != 0:
                if over:
                    out["n_filt"][l] += 1
                elif b.masked[i]:
                    out["n_skip"][l] += 1
                elif b.haploid[l]:
                    assert gts[0] == gts[1]                                              # :1175
                    out["allele_count"][vo + gts[0]] += 1; out["an"][l] += 1
                else:
                    out["allele_count"][vo + gts[0]] += 1; out["allele_count"][vo + gts[1]] += 1; out["an"][l] += 2
            # :1239-1254 — reported (:1241), the mask FIRST (:1243), the fraction (:1245-1247); samples without reads stay
            if b.reported[i] and not b.masked[i] and not over:
                out["dp"][l] += na; out["dsnp"][l] += int(b.n_snp[i]); out["dstutter"][l] += int(b.n_stutter[i]); out["dflankindel"][l] += nfi
            # :1326-1352 — no column, NO_READS (:1332), the mask (:1339), FLANK_INDEL_FRAC (:1346)
            st = NOT_REPORTED if not b.reported[i] else NO_READS if na == 0 else MASKED if b.masked[i] else FLANK_INDEL_FRAC if over else PASS
            out["status"][i] = st
            # :1362-1375 — the HAPLOTYPES differ, not the genotypes
            if st == PASS and not b.haploid[l] and ha != hb:
                out["ab"][i], out["fs"][i] = pvalues(int(b.uniq_one[i]), int(b.uniq_two[i]), int(b.rv_uniq_one[i]), int(b.rv_uniq_two[i]))
                out["dab"][i] = int(b.uniq_one[i]) + int(b.uniq_two[i])
        so += S; ho += A; vo += V
    return out


FIELD_SEEDS = (0, 1, 2, 3, 4, 5)
INT_KEYS = ("status", "gt", "dab", "n_skip", "n_filt", "an", "dp", "dsnp", "dstutter", "dflankindel", "allele_count")
