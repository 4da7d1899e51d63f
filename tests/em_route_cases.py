"""The launch routes and size edges of the stutter EM (hipstr_amd/csrc/em.hip; DESIGN.md section 3, "Routes of the other device stages").

Like tests/stage_route_cases.py: every case is deterministic (no random draw at all: sizes and phasing terms are written down by index),
sits on the sides of one limit the library reports (hipstr_debug_em_plan: limits are read from its "thresholds", never repeated here)
and names what its plan must show.  Inputs are built directly (locus() / batch()), so A, S and R are exactly what a case says.
tests/test_em_routes.py checks the plans on the host, tests/test_em_routes_gpu.py runs the same inputs on the device against the oracle.

The C-ABI has ONE ref_allele per batch (hipstr_em_batch_t), so batch() takes it per batch, not per locus.
"""
import collections

import numpy as np

from hipstr_amd import capi

# name: the case; kw: run_em / em_plan keyword arguments; check(plan, T): what the plan must show; alone: loci that are also run on
# their own (their results must equal the ones inside the batch)
EmCase = collections.namedtuple("EmCase", "name kw check alone")
Refusal = collections.namedtuple("Refusal", "name kw message")

# routes of the plan no case takes, each with its reason (tests/test_em_routes.py asserts that exactly these are missing)
UNREACHABLE = {
    "rows_direct": "the row fallback of A >= 2 * HS_EM_CHUNK * HS_EM_MAXA_LDS = 4096 alleles: the oracle would need 16 R A^2 bytes eight times "
                   "over (terabytes at R >= A) and the device minutes",
}


def limits(lib):
    return capi.em_plan(lib, **batch([locus(2, [[(0, 0.0, 0.0)]])]))["thresholds"]


def routes(lib):
    return set(capi.em_plan(lib, **batch([locus(2, [[(0, 0.0, 0.0)]])]))["routes"])


# ------------------------------------------------------------------------------------------------ builders
def phase(i):
    """(log_p1, log_p2) of the i-th read of a sample: no phasing information (the M-step's `same` shortcut), strand one, strand two."""
    k = i % 3
    if k == 0:
        return 0.0, 0.0
    good, bad = -0.01 * (1 + i % 4), -2.5 - 0.75 * (i % 5)
    return (good, bad) if k == 1 else (bad, good)


def sample(sizes, shift=0):
    """A sample's reads from their sizes, the phasing terms mixed by read index."""
    return [(int(z),) + phase(j + shift) for j, z in enumerate(sizes)]


def locus(period, samples, haploid=0):
    """samples: per sample a list of (size, log_p1, log_p2)."""
    return dict(period=period, haploid=haploid, samples=samples)


def batch(loci, ref_allele=0, max_iter=100):
    kw = dict(period=[], n_samples=[], read_off=[0], sample_label=[], num_bps=[], log_p1=[], log_p2=[], haploid=[], ref_allele=ref_allele, max_iter=max_iter)
    for L in loci:
        kw["period"].append(L["period"]); kw["haploid"].append(L["haploid"]); kw["n_samples"].append(len(L["samples"]))
        for s, reads in enumerate(L["samples"]):
            for z, p1, p2 in reads:
                kw["sample_label"].append(s); kw["num_bps"].append(z); kw["log_p1"].append(p1); kw["log_p2"].append(p2)
        kw["read_off"].append(len(kw["num_bps"]))
    return kw


def sub_batch(kw, idx):
    """The loci idx of a batch as a batch of their own."""
    out = {k: v for k, v in kw.items() if k in ("ref_allele", "max_iter")}
    out.update(period=[], n_samples=[], read_off=[0], sample_label=[], num_bps=[], log_p1=[], log_p2=[], haploid=[])
    for l in idx:
        r0, r1 = kw["read_off"][l], kw["read_off"][l + 1]
        for k in ("period", "n_samples", "haploid"):
            out[k].append(kw[k][l])
        for k in ("sample_label", "num_bps", "log_p1", "log_p2"):
            out[k] += list(kw[k][r0:r1])
        out["read_off"].append(len(out["num_bps"]))
    return out


def shape(kw, l):
    """(A, S, R) of locus l, counted here (what the plan must agree with)."""
    r0, r1 = kw["read_off"][l], kw["read_off"][l + 1]
    return len(set(kw["num_bps"][r0:r1]) | {kw["ref_allele"]}), kw["n_samples"][l], r1 - r0


SMALL = locus(3, [sample([0, 3, 0]), sample([3, 6, 6], 1), sample([0, 0, 2], 2), sample([6, 3])])          # A = 3 (+ an out-of-frame size: 4)
assert len({z for s in SMALL["samples"] for z, _, _ in s}) == 4
A3 = locus(3, [sample([0, 3, 0]), sample([3, 6, 6], 1), sample([0, 0, 3], 2), sample([6, 3])])             # A = 3, the neighbour of every case


def allele_locus(A, period=2, haploid=0):
    """Exactly A distinct sizes (the reference size 0 among them), just enough samples and reads to show them: two neighbouring sizes per
    sample (three reads where the sample index is a multiple of 4), every seventh size out of frame."""
    ks = [k for k in range(-((A - 1) // 2), A - (A - 1) // 2)]
    sizes = [period * k + (1 if (k % 7 == 3 and period > 1) else 0) for k in ks]
    assert len(set(sizes)) == A and 0 in sizes
    samples = []
    for s in range(0, A, 2):
        zs = sizes[s:s + 2]
        if (s // 2) % 4 == 0:
            zs = zs + zs[:1]
        samples.append(sample(zs, s // 2))
    if len(samples) < 2:
        samples.append(sample(sizes[:2] + sizes[:1], 1))
    return locus(period, samples, haploid)


def _show(plan, l, **want):
    got = plan["loci"][l]
    for k, v in want.items():
        assert got[k] == v, (l, k, got[k], v)


# ------------------------------------------------------------------------------------------------ allele counts
def allele_cases(T):
    """A = 1, 2, both sides of the row-tile formula's step from 256 rows to fewer, M - 1, M, M + 1 (diploid and haploid), 2 M, 2 M + 1 with
    M = HS_EM_MAXA_LDS: each a locus of its own behind an A = 3 locus, one batch per count (the oracle's time goes with R A^2 per round:
    one batch of them all would take half a minute)."""
    M, W = T["HS_EM_MAXA_LDS"], T["HS_EM_GMAX_WAVE_MAXA"]
    assert M == W                     # (one series covers both limits; if they ever part, each needs its own)
    # the largest A whose rows still come 256 to a tile (A | 1 around 16)
    full = max(a for a in range(1, M) if T["lds_doubles"] // (a | 1) >= T["HS_EM_THREADS"])
    counts = [("1", 1, 0), ("2", 2, 0), ("tile_full", full, 0), ("tile_reduced", full + 1, 0), ("M-1", M - 1, 0), ("M", M, 0), ("M+1", M + 1, 0),
              ("M+1_haploid", M + 1, 1), ("2M", 2 * M, 0), ("2M+1", 2 * M + 1, 0)]
    out = []
    for tag, A, hap in counts:
        # (a round of the oracle on 2 M sizes takes 0.4 s: those two loci get 6 rounds and end with train() == false next to a trained one)
        kw = batch([A3, allele_locus(A, haploid=hap)], max_iter=100 if A < 2 * M else 6)
        def check(plan, T, kw=kw, A=A, hap=hap, tag=tag):
            assert shape(kw, 1)[0] == A
            tr = min(T["HS_EM_THREADS"], T["lds_doubles"] // (A | 1))
            _show(plan, 1, A=A, haploid=hap, gmax="wave" if A <= W else "thread", row_tile=tr, sweeps=-(-A // M), last_sweep=A - M * ((A - 1) // M))
            assert plan["loci"][1]["post"][0] == ("registers" if A * A <= T["HS_POST_THREADS"] * T["HS_POST_REGS"] else "chunked")
            want = {"tile_full": dict(row_tile=T["HS_EM_THREADS"]), "M": dict(sweeps=1, last_sweep=M), "M+1": dict(sweeps=2, last_sweep=1),
                    "2M": dict(sweeps=2, last_sweep=M), "2M+1": dict(sweeps=3, last_sweep=1)}.get(tag, {})
            _show(plan, 1, **want)
            if tag == "tile_reduced":
                assert plan["loci"][1]["row_tile"] < T["HS_EM_THREADS"]
            _show(plan, 0, A=3)
        out.append(EmCase("alleles_" + tag, kw, check, [1]))
    return out


# ------------------------------------------------------------------------------------------------ sample counts
def sample_locus(S, A=2, period=3):
    """S samples of one read each; A = 2: the sizes 0 and `period` in turn (S = 1: the read shows `period`, the reference size is not seen);
    A = 1: every read at the reference size."""
    if A == 1:
        return locus(period, [[(0,) + phase(s)] for s in range(S)])
    return locus(period, [[((period if s % 3 != 1 else 0),) + phase(s)] for s in range(S)])


def sample_cases(T):
    U, C, TH = T["HS_EM_UNITS_THREADS"], T["HS_EM_CHUNK"], T["HS_EM_THREADS"]
    # chain of S + 2 S positions: S = 11 leaves a last chunk of ONE position (33 = 32 + 1), S = U a full one; rows S A: S = U fills its
    # row tiles, and with A = 1 (rows = S) S = U + 1 leaves a last tile of ONE row — 2 S is even, so A = 2 cannot
    s_one = next(s for s in range(2, 200) if (3 * s) % C == 1)
    specs = [(1, 2), (4, 2), (5, 2), (s_one, 2), (U, 2), (U + 1, 2), (U + 1, 1)]
    kw = batch([A3] + [sample_locus(S, A) for S, A in specs])
    def check(plan, T):
        for i, (S, A) in enumerate(specs):
            assert shape(kw, i + 1) == (A, S, S)
            _show(plan, i + 1, A=A, S=S, R=S, row_tile=TH)
        by = {sp: plan["loci"][i + 1] for i, sp in enumerate(specs)}
        assert by[(s_one, 2)]["scan_last"] == 1 and by[(U, 2)]["scan_last"] == C and by[(U, 2)]["last_row_tile"] == TH and by[(U + 1, 1)]["last_row_tile"] == 1
        assert by[(U + 1, 2)]["row_tiles"] == by[(U, 2)]["row_tiles"] + 1
        assert plan["max_S"] == U + 1 and plan["units_passes"] == 2
    both = EmCase("sample_counts", kw, check, list(range(1, len(specs) + 1)))
    kw1 = batch([A3, sample_locus(U)])
    def check1(plan, T):
        assert plan["max_S"] == U and plan["units_passes"] == 1 and "units_one_pass" in plan["routes_hit"]
    return [both, EmCase("sample_counts_at_stride", kw1, check1, [1])]


# ------------------------------------------------------------------------------------------------ reads
def read_cases(T):
    P, TL = T["HS_EM_PARTS"], T["HS_EM_TILE"]
    out = []
    for S in (1, 3):
        empty = locus(4, [[] for _ in range(S)])
        def check(plan, T, S=S):
            _show(plan, 0, A=1, S=S, R=0, empty_slices=P, slice_tiles=0)
            assert plan["loci"][0]["post"][1] == 0 and "slices_no_rows" in plan["routes_hit"] and "post_no_reads" in plan["routes_hit"]
        out.append(EmCase("no_reads_alone_S%d" % S, batch([empty]), check, []))
        def check2(plan, T, S=S):
            _show(plan, 1, A=1, S=S, R=0, empty_slices=P)
            _show(plan, 0, A=3); _show(plan, 2, A=4)
        out.append(EmCase("no_reads_between_S%d" % S, batch([A3, empty, SMALL]), check2, [0, 1, 2]))
    # samples without reads at the first, a middle and the last label
    holes = locus(2, [[], sample([0, 2, 2]), [], sample([2, 4, 0, 3], 1), []])
    def check_h(plan, T):
        _show(plan, 1, S=5, R=7, A=4)
    out.append(EmCase("samples_without_reads", batch([A3, holes, A3]), check_h, [1]))
    # R A = 1, 7, 8, 9 around HS_EM_PARTS
    few = [(locus(5, [sample([0])]), 1, 1), (locus(5, [sample([0, 0, 0, 0]), sample([0, 0, 0], 1)]), 1, 7),
           (locus(5, [sample([0, 5]), sample([5, 5], 1)]), 2, 4), (locus(5, [sample([0, 5]), sample([4], 2)]), 3, 3)]
    assert [a * r for _, a, r in few] == [1, P - 1, P, P + 1]
    kwf = batch([A3] + [L for L, _, _ in few])
    def check_f(plan, T):
        for i, (_, A, R) in enumerate(few):
            assert shape(kwf, i + 1)[::2] == (A, R)
            n = A * R
            _show(plan, i + 1, A=A, R=R, empty_slices=max(0, P - n), slice_rows=[n // P, -(-n // P)], slice_tiles=1)
    out.append(EmCase("rows_around_parts", kwf, check_f, [1, 2, 3, 4]))
    # R A = PARTS * TILE: every slice exactly one tile; + PARTS: one row more, two tiles.  A = 2, four samples: a unit has more reads
    # than fit an LDS tile of the posterior kernel's register path
    for d in (0, 1):
        R = (P * TL + d * P) // 2
        per = R // 4
        pattern = lambda s, n: [(4 if (j * 7 + s) % (5 + 3 * s) == 0 else 0) if s % 2 == 0 else (0 if (j * 5 + s) % 11 == 0 else 4) for j in range(n)]
        samples = [sample(pattern(s, per + (R - 4 * per if s == 3 else 0)), s) for s in range(4)]
        kwb = batch([locus(4, samples)])
        def check_b(plan, T, d=d, R=R, kwb=kwb):
            assert shape(kwb, 0) == (2, 4, R) and 2 * R == P * TL + d * P
            _show(plan, 0, A=2, R=R, slice_rows=[TL + d, TL + d], empty_slices=0, slice_tiles=1 + d)
            assert plan["loci"][0]["post"][0] == "registers" and plan["loci"][0]["post"][3] > 1
        out.append(EmCase("slice_of_one_tile_%+d" % d, kwb, check_b, []))
    return out


# ------------------------------------------------------------------------------------------------ periods and sizes
def period_case(T):
    """Periods 1, 7, 8, 9 (and 2 for comparison) under a reference size of 5 that no read shows: sizes below and above it, differences in
    frame and out of frame of both signs, smaller than the period and larger (C's truncating % and / on negative differences)."""
    ref = 5
    loci = []
    for p in (1, 7, 8, 9, 2):
        d = [-2 * p, -p, p, 2 * p, -1, 1, -(p + 1), p + 1, -(2 * p - 1), 3 * p - 1, -(p - 1), p - 1] if p > 1 else [-3, -2, -1, 1, 2, 4]
        d = sorted(set(x for x in d if x != 0))
        zs = [ref + x for x in d]
        samples = [sample(zs[i:i + 3] + zs[i:i + 1], i) for i in range(0, len(zs), 2)]
        loci.append(locus(p, samples))
    kw = batch(loci, ref_allele=ref)
    def check(plan, T):
        for l, L in enumerate(loci):
            r0, r1 = kw["read_off"][l], kw["read_off"][l + 1]
            zs = set(kw["num_bps"][r0:r1])
            assert ref not in zs and min(zs) < ref < max(zs)
            _show(plan, l, A=len(zs) + 1, period=L["period"])
            p = L["period"]
            if p > 1:
                bd = {a - b for a in zs for b in zs | {ref}}
                assert any(x % p and 0 < x < p for x in bd) and any(x % p and -p < x < 0 for x in bd)
                assert any(x % p and x > p for x in bd) and any(x % p and x < -p for x in bd) and any(x % p == 0 and x < 0 for x in bd)
    return EmCase("periods_and_sizes", kw, check, list(range(len(loci))))


# ------------------------------------------------------------------------------------------------ batch sizes
def tiny_locus(i):
    """S <= 2, R <= 4, A <= 3, done after 2 to 5 rounds (the haploid kinds take 3, 4 and 5)."""
    k = i % 6
    if k == 0:
        return locus(2 + i % 3, [sample([0, 0], i), sample([0, 0], i + 1)], haploid=i % 12 == 0)
    p = 2 + i % 5
    if k == 1:
        return locus(p, [sample([0, p], i), sample([p, p], i + 1)])
    if k == 2:
        return locus(p, [sample([0, 0, p], i)])
    return locus(5, [sample([10, 10] if k < 5 else [0, 10], 1), sample([{3: 2, 4: 1, 5: -5}[k], 10], 2)], haploid=1)


def slow_locus(i):
    """S = 2, R = 4, A = 3, haploid, with out-of-frame sizes: 17 or 18 rounds, more than three times tiny_locus' most (asserted from the
    oracle's counts where the cases run)."""
    if i % 2:
        return locus(5, [sample([6, 6], 1), sample([-5, 6], 2)], haploid=1)
    return locus(4, [sample([0, 1], 1), sample([-2, 1], 2)], haploid=1)


def slow_indices(n):
    return sorted({i for i in (0, 1023, 1024, n - 1) if 0 <= i < n})


def batch_cases(T):
    I, C = T["HS_EM_INIT_THREADS"], T["HS_EM_COMPACT_THREADS"]
    out = []
    for n in (1, I, I + 1, C, C + 1, 2 * C + 1):
        slow = slow_indices(n)
        assert slow == sorted({i for i in (0, C - 1, C, n - 1) if i < n})
        loci = [slow_locus(i) if i in slow else tiny_locus(i) for i in range(n)]
        for mi in (100, 2):
            kw = batch(loci, max_iter=mi)
            def check(plan, T, n=n, mi=mi):
                assert plan["n_loci"] == n and plan["init_blocks"] == -(-n // I) and plan["compact_chunks"] == -(-n // C)
                assert plan["compact_last_chunk"] == n - C * ((n - 1) // C) and T2(plan)["last_round"] == mi + 1
                assert all(L["S"] <= 2 and L["R"] <= 4 and L["A"] <= 3 for L in plan["loci"])
            near = sorted(set(slow) | {i + 1 for i in slow if i + 1 < n} | {i - 1 for i in slow if i > 0})
            out.append(EmCase("batch_of_%d_max_iter_%d" % (n, mi), kw, check, near if mi == 100 else slow))
    return out


def T2(plan):
    return plan["thresholds"]


# ------------------------------------------------------------------------------------------------ the table of integer logarithms
def _pair(period, size, ref_allele=0):
    return batch([locus(period, [sample([size, size, ref_allele]), sample([ref_allele, size], 1)])], ref_allele=ref_allele)


def eff_of(bd, p):
    """em.hip's effective difference: C's truncating division."""
    q = abs(bd) // p * (1 if bd >= 0 else -1)
    return bd - q if bd % p else q


def table_edge_cases(T):
    """|eff| = table length - 1, the last entry: accepted, A = 2, and run against the oracle — by a period-1 difference, a period-2
    difference in frame (a span of twice the table) and a period-3 difference out of frame, each of both signs."""
    N = T["int_log_len"]
    out = []
    for p, bd in ((1, N - 1), (2, 2 * (N - 1)), (3, _oof3(N - 1))):
        for sign in (1, -1):
            assert abs(eff_of(sign * bd, p)) == N - 1
            kw = _pair(p, sign * bd)
            def check(plan, T):
                _show(plan, 0, A=2, R=5)
            out.append(EmCase("last_log_entry_period%d_%s" % (p, "up" if sign > 0 else "down"), kw, check, []))
    return out


def _oof3(eff):
    """The out-of-frame difference of period 3 whose effective difference is eff."""
    bd = next(b for b in range(eff, 2 * eff + 3) if b % 3 and b - b // 3 == eff)
    return bd


def refusals(T):
    N = T["int_log_len"]
    far = "allele sizes too far apart"
    out = []
    for p, bd in ((1, N), (2, 2 * N), (3, _oof3(N))):
        for sign in (1, -1):
            assert abs(eff_of(sign * bd, p)) == N
            out.append(Refusal("beyond_log_table_period%d_%s" % (p, "up" if sign > 0 else "down"), _pair(p, sign * bd), far))
    # the reference allele counts although no read shows it; a far pair among a locus' other sizes; the second locus of a batch
    out.append(Refusal("beyond_log_table_unobserved_reference", batch([locus(1, [sample([N + 7, N + 7]), sample([N + 8], 1)])], ref_allele=7), far))
    out.append(Refusal("beyond_log_table_second_locus", batch([A3, locus(1, [sample([-5, N - 5])]), A3]), far))
    lo, hi = -2 ** 31, 2 ** 31 - 1
    out.append(Refusal("int32_extremes", batch([locus(4, [sample([lo, hi, 0])])]), far))
    out.append(Refusal("int32_min_against_reference_max", batch([locus(9, [sample([lo, lo + 9])])], ref_allele=hi), far))
    out.append(Refusal("int32_max_alone", batch([locus(2, [sample([hi])])]), far))
    out.append(Refusal("period_0", batch([A3, locus(0, [sample([0, 2])])]), "STR period must be in"))
    out.append(Refusal("period_10", batch([locus(10, [sample([0, 10])])]), "STR period must be in"))
    out.append(Refusal("no_samples", batch([A3, locus(3, [])]), "locus without samples"))
    out.append(Refusal("too_many_sizes", batch([locus(1, [sample(list(range(1, N - 1)))])]), "too many distinct allele sizes"))
    out.append(Refusal("descending_sample", dict(period=[4], n_samples=[2], read_off=[0, 3], sample_label=[1, 0, 1], num_bps=[0, 4, 4], log_p1=[0, 0, 0], log_p2=[0, 0, 0]),
                       "ascending sample"))
    return out


def most_sizes_accepted(T):
    """One size fewer than `too_many_sizes`: the plan accepts it (host only: R A^2 is far beyond what the oracle or a test run can take)."""
    return batch([locus(1, [sample(list(range(1, T["int_log_len"] - 2)))])])


# ------------------------------------------------------------------------------------------------ all of them
CASE_NAMES = (["alleles_" + t for t in ("1", "2", "tile_full", "tile_reduced", "M-1", "M", "M+1", "M+1_haploid", "2M", "2M+1")]
              + ["sample_counts", "sample_counts_at_stride", "no_reads_alone_S1", "no_reads_between_S1", "no_reads_alone_S3",
               "no_reads_between_S3", "samples_without_reads", "rows_around_parts", "slice_of_one_tile_+0", "slice_of_one_tile_+1",
               "periods_and_sizes"]
              + ["batch_of_%d_max_iter_%d" % (n, mi) for n in (1, 256, 257, 1024, 1025, 2049) for mi in (100, 2)]
              + ["last_log_entry_period%d_%s" % (p, s) for p in (1, 2, 3) for s in ("up", "down")])
REFUSAL_NAMES = (["beyond_log_table_period%d_%s" % (p, s) for p in (1, 2, 3) for s in ("up", "down")]
                 + ["beyond_log_table_unobserved_reference", "beyond_log_table_second_locus", "int32_extremes", "int32_min_against_reference_max",
                    "int32_max_alone", "period_0", "period_10", "no_samples", "too_many_sizes", "descending_sample"])
ORDINARY = "periods_and_sizes"          # the case a device run goes back to after a refusal


def cases(T):
    out = allele_cases(T) + sample_cases(T) + read_cases(T) + [period_case(T)] + batch_cases(T) + table_edge_cases(T)
    return collections.OrderedDict((c.name, c) for c in out)
