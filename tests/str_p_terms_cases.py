"""Batches for the 13-term evaluation of hs_str_group_kernel_p (the terms go through a pipeline of two), at the
smallest shapes its address clamps and its pipeline can go wrong at.  tests/test_str_p_terms.py checks on the host that every (read side,
allele) pair of them is routed to that kernel and that the oracle equals the compiled reference on them; tests/test_str_p_terms_gpu.py
runs them on the device against the oracle.

Per period P = 1..6, two batches:

  sides    one locus, reads with caller-given seeds (hipstr_hmm_process_reads_seeded).  The STR alleles are all suffixes of one periodic
           string, so that sorted by length they form one chain (every block continues the previous one's tables: `chained`), except
           for three blocks of another phase that break it (`chained` false in the middle of the list, true again after it):
             * 1, 3 and 5 repeat units: fewer deletion sizes than six (the sizes the block does not hold are requested and not added);
             * exactly 6 units, 6P+1 .. 6P+P-1 bases (a chain that grows by a base), 7, 8, 9 units (a chain that grows by a unit);
             * 9 and 10 units and 10 units + 1 base of the other phase: the chain break;
             * a block of 300 bases or more: much longer than every side but the longest.
           The read sides have 1, 2, P, 6P-1, 6P and 6P+1 columns (on either side of the seed) and 256 columns (a whole group): columns
           on both sides of rj < (q+1)P for every deletion size, of max(aM - D8, aZ) and of min(max(j8p8 - D8, 0), B8) for every
           insertion size.
  packing  two loci with the library's seeds: 20 short reads (more than a group holds: the read maximum cuts the groups, and wavefronts
           without a column stay out: `wave_act`) and a locus of one read (a group of one).
"""
import numpy as np

from hipstr_amd import capi
import util

PERIODS = (1, 2, 3, 4, 5, 6)
MOTIF = {1: "A", 2: "AC", 3: "CAG", 4: "AGAT", 5: "AAGGC", 6: "ACGTTG"}
AUTO = -2                                   # HIPSTR_SEED_AUTO: the library computes the seed
FLANK = 262                                 # bases of either flank: a side of 256 columns starts in one flank and ends in the other
KERNEL = "hs_str_group_kernel_p"


def _flank(tag, n):
    rng = np.random.default_rng(sum(map(ord, tag)) * 7919)
    return "".join(rng.choice(list("CGT"), n))          # (no A: a flank never continues the period-1 block)


def _suffix(motif, n):
    """The last n bases of the motif repeated: every such block is a suffix of every longer one."""
    return (motif * (n // len(motif) + 2))[-n:]


def blocks(P):
    """The STR alleles of the `sides` locus; the first is the reference allele (7 units)."""
    m = MOTIF[P]
    other = (m[1:] + m[0]) if P > 1 else "C"            # the same repeat in another phase (period 1: another base)
    lens = [7 * P, P, 3 * P, 5 * P, 6 * P] + [6 * P + r for r in range(1, P)] + [8 * P, 9 * P, -(-300 // P) * P]
    out = [_suffix(m, n) for n in lens] + [_suffix(other, n) for n in (9 * P, 10 * P, 10 * P + 1)]
    assert len(set(out)) == len(out)
    return out


def side_pairs(P):
    """(columns left of the seed, columns right of it) of the reads of the `sides` locus."""
    s = [1, 2, P, 6 * P - 1, 6 * P, 6 * P + 1]
    pairs = list(zip(s, reversed(s))) + [(256, 1), (1, 256), (6 * P, 6 * P + 1)]
    return sorted(set(pairs))


def sides(P):
    """-> (finalized batch, seeds).  A read with the longer side on the left has its seed base right behind the STR block and runs through
    the block into the left flank; the others have it right in front of the block."""
    lf, rf = _flank("str_p_lf%d" % P, FLANK), _flank("str_p_rf%d" % P, FLANK)
    strs = blocks(P)
    hap = lf + strs[0] + rf
    reads, seeds = [], []
    for i, (nl, nr) in enumerate(side_pairs(P)):
        at = len(lf) + len(strs[0]) + 1 if nl >= nr else len(lf) - 2         # the seed base's place in the haplotype
        off, n = at - nl, nl + nr + 1
        assert off >= 0 and off + n <= len(hap)
        q = "".join(chr(ord("5") + (7 * j + 3 * i) % 40) for j in range(n))
        reads.append((hap[off:off + n], q, off, True))
        seeds.append(nl)
    b, _ = util.simple_locus(lf, strs, rf, P, reads)
    return b.finalize(), np.array(seeds, np.int32)


def packing(P):
    """-> (finalized batch, seeds = the library's).  20 reads of 12 + 1 + 12 bases around the block's start (25 columns a read: the read
    maximum of a group is reached long before its columns are), then a locus with one read."""
    b = capi.Batch()
    m = MOTIF[P]
    for tag, n_reads in (("a", 20), ("b", 1)):
        lf, rf = _flank("str_p_pk%s%d" % (tag, P), 40), _flank("str_p_pk%s%d" % (tag.upper(), P), 40)
        strs = [_suffix(m, 7 * P), _suffix(m, 6 * P), _suffix(m, 9 * P + (1 if P > 1 else 0))]
        hap = lf + strs[0] + rf
        reads = []
        for i in range(n_reads):
            off = len(lf) - 14 + i % 5
            q = "".join(chr(ord("5") + (5 * j + 3 * i) % 40) for j in range(25))
            reads.append((hap[off:off + 25], q, off, True))
        util.simple_locus(lf, strs, rf, P, reads, batch=b)
    n = 21
    return b.finalize(), np.full(n, AUTO, np.int32)


BUILDERS = {"sides": sides, "packing": packing}
CASES = [(kind, P) for kind in ("sides", "packing") for P in PERIODS]
REDO_CASES = [("sides", 1), ("sides", 3), ("packing", 6)]       # run with HIPSTR_DEBUG_REDO (the re-do mark instead of the store)


def build(kind, P):
    return BUILDERS[kind](P)


def routed_to(plan):
    """The STR kernels that take the batch's (read side, allele) pairs."""
    return {k for c in plan["chunks"] for k, v in c["str"]["pairs"].items() if v > 0}


def groups(plan):
    """[side, columns, reads] of every group of the grouped STR kernels."""
    return [g for c in plan["chunks"] for g in c["str"]["groups"]]


def check_device(hmm, oracle, kind, P, fill=-3.25):
    """One-shot and resident (two passes on one upload) against the oracle, bit for bit; the route from the launch plan."""
    b, seed_in = build(kind, P)
    what = "%s period %d" % (kind, P)
    assert routed_to(capi.launch_plan(hmm, b.ptr)) == {KERNEL}, what
    want, ws = capi.run_align(oracle, "oracle_", b.ptr, fill=fill, seed_in=seed_in)
    got, gs = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=fill, seed_in=seed_in)
    given = seed_in != AUTO
    assert np.array_equal(ws[given], seed_in[given]), what + ": the oracle did not take the given seeds"
    assert np.array_equal(gs, ws), what + ": seeds differ"
    assert np.array_equal(got == fill, want == fill), what + ": untouched entries differ"
    assert np.array_equal(got, want), "%s: %d of %d values differ, max|diff| %g" % (what, int((got != want).sum()), got.size, np.nanmax(np.abs(got - want)))
    dev = hmm.hipstr_hmm_upload_seeded(b.ptr, capi._ptr(seed_in, capi._i32p))
    assert dev, hmm.hipstr_last_error()
    try:
        n_reads, n_out, _ = capi.batch_dims(b.ptr)
        for rep in range(2):
            assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error()
            p = np.full(max(n_out, 1), fill); s = np.full(max(n_reads, 1), -7, np.int32)
            assert hmm.hipstr_hmm_fetch(dev, p.ctypes.data_as(capi._f64p), s.ctypes.data_as(capi._i32p)) == 0
            assert np.array_equal(s[:n_reads], ws), "%s resident pass %d: seeds differ" % (what, rep)
            assert np.array_equal(p[:n_out], want), "%s resident pass %d differs" % (what, rep)
    finally:
        hmm.hipstr_hmm_free(dev)
    return got.size


if __name__ == "__main__":
    # the child of tests/test_str_p_terms_gpu.py: the library reads HIPSTR_DEBUG_REDO from the environment of the process
    import os
    assert os.environ.get("HIPSTR_DEBUG_REDO"), "run with HIPSTR_DEBUG_REDO set"
    hmm, oracle = capi.load_hmm(), capi.load_oracle()
    assert hmm.hipstr_hmm_init(0) == 0, hmm.hipstr_last_error()
    n = sum(check_device(hmm, oracle, kind, P) for kind, P in REDO_CASES)
    print("redo ok %d" % n)
