"""GPU: hipstr_rm_* — the read x haplotype matrix (log_aln_probs_, R x A per locus) kept on the device between the rounds of
SeqStutterGenotyper::genotype (include/hipstr_hmm.h): hipstr_rm_scatter is the second half of calc_hap_aln_probs
(reference src/seq_stutter_genotyper.cpp:530-564: pool rows to reads, mate sums, merge into earlier rounds), hipstr_rm_remap the column
re-layout of add_and_remove_alleles (:371-386).

Every comparison is on the bit patterns (view(np.uint64)): the only arithmetic is one IEEE double addition per mate pair and column, so
nothing rounds differently and there is no tolerance.  The yardsticks: the compiled reference's own matrices (tests/golden/pool_scatter_*.npz,
written by its classes) and, for the shapes the fixtures do not reach, `host_scatter` / `host_remap` (tests/flow_chain.py) — :530-564 and :371-386 restated
in numpy on the rows hipstr_hmm_process_reads returns for the same pooled batch."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import util
from hipstr_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNALIGNED = -100000.0                  # seq_stutter_genotyper.cpp:374
FILL = -3.25                           # what the host arrays hold where process_reads leaves them untouched
AUTO = -2                              # HIPSTR_SEED_AUTO


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    assert np.array_equal(g, w), "%s: %d of %d entries differ, first at %s" % (what, int((g != w).sum()), g.size, np.argwhere(g != w)[:1].tolist())


# the host path, restated (seq_stutter_genotyper.cpp:530-564 and :371-386): tests/flow_chain.py, shared with the end-to-end chain
from flow_chain import host_scatter, host_remap  # noqa: E402


def upload_and_align(hmm, b, seed_in=None):
    si = None if seed_in is None else np.ascontiguousarray(seed_in, np.int32)
    dev = hmm.hipstr_hmm_upload_seeded(b.ptr, capi._ptr(si, capi._i32p))
    assert dev, hmm.hipstr_last_error().decode()
    assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error().decode()
    return dev


# ------------------------------------------------------------------------------------------------------------------ 1. the compiled reference
POOL = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pool_scatter_*.npz")))


def pooled_batch_of(d):
    """The batch ReadPooler leaves behind (read_pooler.cpp:3-20): the first read of every pool with the pool's qualities."""
    pi = d["expect_pool_index"]; P = int(d["expect_n_pools"][0]); qo = d["expect_pool_qual_off"]
    first = [int(np.nonzero(pi == p)[0][0]) for p in range(P)]
    out = {k: d[k] for k in ("blk_start", "blk_end", "blk_nopts", "period", "stutter", "opt_off", "hap_off", "seq", "realign_hap")}
    bo, co = d["base_off"], d["cigar_off"]
    bases = [bytes(d["bases"][bo[r]:bo[r + 1]]) for r in first]
    quals = [bytes(d["expect_pool_quals"][qo[p]:qo[p + 1]]) for p in range(P)]
    assert [len(x) for x in bases] == [len(x) for x in quals]
    out["read_off"] = np.array([0, P], np.int32)
    out["base_off"] = np.concatenate([[0], np.cumsum([len(x) for x in bases])]).astype(np.int32)
    out["bases"] = np.frombuffer(b"".join(bases) + b"\0", np.uint8); out["quals"] = np.frombuffer(b"".join(quals) + b"\0", np.uint8)
    out["read_start"] = d["read_start"][first].astype(np.int32)
    ops = [bytes(d["cigar_op"][co[r]:co[r + 1]]) for r in first]; lens = [d["cigar_len"][co[r]:co[r + 1]] for r in first]
    out["cigar_off"] = np.concatenate([[0], np.cumsum([len(x) for x in ops])]).astype(np.int32)
    out["cigar_op"] = np.frombuffer(b"".join(ops) + b"\0", np.uint8); out["cigar_len"] = np.concatenate(lens).astype(np.int32)
    out["realign_read"] = d["realign_pool"].astype(np.uint8)
    return util.batch_from_dict(out)


@pytest.mark.parametrize("path", POOL, ids=[os.path.basename(p)[13:-4] for p in POOL])
def test_pinned_to_the_compiled_reference(_native_built, hmm, path):
    """The matrix and the seeds the reference's own calc_hap_aln_probs left (masked haplotypes, skipped pools and reads, a pre-filled matrix,
    a pair whose mates differ in copy_read), bit for bit."""
    assert len(POOL) == 3
    d = np.load(path)
    b = pooled_batch_of(d)
    R = int(d["read_off"][1]); A = int(d["hap_off"][1])
    dev = upload_and_align(hmm, b)
    rm = capi.ReadMatrix(hmm, [A], [0, R], d["expect_pool_index"], d["second_mate"], init_ll=d["prefill"], init_seeds=np.full(R, -9, np.int32))
    try:
        rm.scatter(dev, d["copy_read"])
        ll, seeds = rm.fetch()
    finally:
        rm.close(); hmm.hipstr_hmm_free(dev)
    assert np.array_equal(seeds, d["expect_seeds"])
    same(ll, d["expect_log_aln_probs"], os.path.basename(path))
    if "later_round" in path:        # the case bites: entries that must stay, seeds that must stay, a pair with differing flags
        m = d["second_mate"].astype(bool); c = d["copy_read"].astype(bool)
        assert (R, A, int(m.sum())) == (48, 24, 7) and int((bits(ll) == bits(d["prefill"])).sum()) == 672
        assert np.all(seeds[~c] == -9) and any(c[i] != c[i - 1] for i in np.nonzero(m)[0])


# ------------------------------------------------------------------------------------------------------------------ 2. shapes
LF = "ACGTTGCATGCATGACCTGAGTCCATGACTTGACA"; RF = "TTGACCGTAGGCTAGGCTTAACGGATCCGATTAGC"
LF2 = LF[:20] + "T" + LF[21:]
# haplotype counts of the loci as (leading-flank options, STR options): A = 1, 3, 4, 32 | 33, 63, 64 | 65 — the narrow route up to its edge
# (HS_RM_NARROW_MAX = 32), the wide route from its first size through one full column step (64) to the first size with two (65) — and a
# locus without reads at the end
SHAPES1 = [(1, 1), (1, 3), (2, 2), (2, 16), (1, 33), (1, 63), (2, 32), (1, 65), (1, 3)]
READS = [7, 130, 2, 130, 7, 1, 130, 130, 0]      # un-pooled reads per locus, from {0, 1, 2, 7, 130}
# round 2 (test 3): two haplotypes removed and three added where there are four or more, three added otherwise
SHAPES2 = [(2, 2), (2, 3), (1, 5), (1, 33), (2, 17), (2, 32), (1, 65), (2, 33), (2, 3)]
MASKED = 3                                        # the locus with a partial realign_hap in round 1


def str_options(n):
    return ["AGAT" * (3 + k % 20) + "AC" * (k // 20) for k in range(n)]


def layout(rng):
    """pool_index (pools shared by 1-4 reads, in shuffled order), second_mate, pools per locus."""
    pool, mates, n_pools = [], [], []
    for R in READS:
        p = []
        while len(p) < R:
            p += [len(set(p))] * int(rng.integers(1, 5))
        p = np.array(p[:R], np.int32); rng.shuffle(p)
        m = (rng.random(R) < 0.3).astype(np.uint8)
        forced = [i for i in (R - 1, 64) if 1 <= i < R]        # a pair as the last two reads of the locus, a pair across the 64-read boundary
        m[forced] = 1; m[:1] = 0
        for i in range(1, R):                                   # never two second mates in a row
            if m[i] and m[i - 1]:
                m[i - 1 if i in forced else i] = 0
        pool.append(p); mates.append(m); n_pools.append(int(p.max()) + 1 if R else 0)
    return np.concatenate(pool), np.concatenate(mates), n_pools


def pooled_batch(shapes, n_pools, masks):
    """One locus per shape with n_pools[l] pooled reads (the same reads whatever the shape: they are cut from haplotypes of 3-8 repeat units)."""
    b = capi.Batch()
    for l, ((n_lf, n_str), P) in enumerate(zip(shapes, n_pools)):
        rng = np.random.default_rng(100 + l)
        reads = []
        for _ in range(P):
            hap = LF + "AGAT" * int(rng.integers(3, 9)) + RF
            off = int(rng.integers(0, 9)); seq = hap[off:off + int(rng.integers(55, 75))]
            qual = "".join(rng.choice(list("#,:FI5"), p=[.05, .1, .2, .45, .1, .1]) for _ in seq)
            reads.append((seq, qual, off, True))
        util.simple_locus(LF, str_options(n_str), RF, 4, reads, start=500 + 400 * l, lf_opts=[LF2] if n_lf == 2 else None, realign_hap=masks[l], batch=b)
    return b.finalize()


class Case:
    pass


@pytest.fixture(scope="module")
def case(_native_built, hmm):
    """The two rounds' pooled batches, their rows from hipstr_hmm_process_reads (computed once, never changed) and the layout."""
    c = Case(); rng = np.random.default_rng(20261018)
    c.pool, c.mates, c.n_pools = layout(rng)
    c.read_off = np.concatenate([[0], np.cumsum(READS)]).astype(np.int32)
    c.pool_off = np.concatenate([[0], np.cumsum(c.n_pools)]).astype(np.int32)
    c.A1 = np.array([a * s for a, s in SHAPES1], np.int32); c.A2 = np.array([a * s for a, s in SHAPES2], np.int32)
    c.mask1 = [None] * len(READS)
    c.mask1[MASKED] = (rng.random(int(c.A1[MASKED])) < 0.5).astype(np.uint8)
    assert 0 < c.mask1[MASKED].sum() < c.A1[MASKED]
    # round 2: per locus the old columns that survive, permuted into the new matrix; the columns left over are the new haplotypes
    c.mapping, c.mask2 = [], []
    for a, na in zip(c.A1, c.A2):
        gone = set(rng.choice(a, 2, replace=False).tolist()) if a >= 4 else set()
        slots = rng.permutation(na)[:a - len(gone)].tolist()
        m = [-1 if j in gone else slots.pop() for j in range(a)]
        new = np.ones(na, np.uint8); new[[x for x in m if x >= 0]] = 0
        assert new.sum() == 3
        c.mapping += m; c.mask2.append(new)
    c.mapping = np.array(c.mapping, np.int32)
    c.b1 = pooled_batch(SHAPES1, c.n_pools, c.mask1); c.b2 = pooled_batch(SHAPES2, c.n_pools, c.mask2)
    c.b1_full = pooled_batch(SHAPES1, c.n_pools, [None] * len(READS))       # round 1 as the reference runs it: every haplotype realigned
    # a pooled read without a seed (tests/test_seeded.py: seed -1), in the 130-read locus with three haplotypes; its pool has a mate among its reads
    c.seed_in = np.full(int(c.pool_off[-1]), AUTO, np.int32)
    r0 = int(c.read_off[1]); mate_reads = np.nonzero(c.mates[r0:int(c.read_off[2])])[0]
    c.no_seed = int(c.pool_off[1]) + int(c.pool[r0 + mate_reads[0]])
    c.seed_in[c.no_seed] = -1
    c.ll1, c.s1 = capi.run_align(hmm, "hipstr_hmm_", c.b1.ptr, fill=FILL, seed_in=c.seed_in)
    c.ll1_full, s1_full = capi.run_align(hmm, "hipstr_hmm_", c.b1_full.ptr, fill=FILL, seed_in=c.seed_in)
    c.ll2, c.s2 = capi.run_align(hmm, "hipstr_hmm_", c.b2.ptr, fill=FILL, seed_in=c.seed_in)
    assert c.s1[c.no_seed] == -1 and (c.s1 >= 0).sum() > 0.8 * len(c.s1) and np.array_equal(c.s1, s1_full)
    c.n = int(c.read_off[-1])
    # expected matrices: round 1 into a fresh matrix, the remap, round 2 on the new columns — from the masked and from the full first round
    c.rounds = {}
    for key, ll1, mask1 in (("masked", c.ll1, c.mask1), ("full", c.ll1_full, [None] * len(READS))):
        M1 = np.full(int((np.diff(c.read_off) * c.A1).sum()), UNALIGNED); seeds1 = np.full(c.n, -1, np.int32)
        host_scatter(M1, seeds1, c.A1, c.read_off, c.pool, c.mates, np.ones(c.n, bool), ll1, c.s1, c.pool_off, mask1)
        M1r = host_remap(M1, c.A1, c.read_off, c.A2, c.mapping)
        M2 = M1r.copy(); seeds2 = seeds1.copy()
        host_scatter(M2, seeds2, c.A2, c.read_off, c.pool, c.mates, np.ones(c.n, bool), c.ll2, c.s2, c.pool_off, c.mask2)
        c.rounds[key] = (M1, M1r, M2)
    c.M1 = c.rounds["masked"][0]; c.seeds1 = seeds1; c.seeds2 = seeds2
    return c


def test_shapes_where_the_kernel_can_go_wrong(hmm, case):
    """Nine loci, A = 1 ... 65 on both routes and both sides of their edges, R from {0, 1, 2, 7, 130}, pools of 1-4 reads, pairs at a locus'
    end and across read 64, a pool without a seed, a partial realign_hap — into a fresh matrix (NULL inits, every read copied), then the
    same rows into a pre-filled matrix under a copy_read that splits pairs."""
    c = case
    routes = [capi.rm_plan(hmm, a, g) for a, g in zip(c.A1, [int(r - c.mates[o:o + r].sum()) for o, r in zip(c.read_off[:-1], READS)])]
    hit = {(p["route"], p["lanes"], p["column_steps"]) for p, r in zip(routes, READS) if r > 0}
    assert {("narrow", 1, 1), ("narrow", 4, 1), ("narrow", 32, 1), ("wide", 64, 1), ("wide", 64, 2)} <= hit
    assert capi.rm_plan(hmm, 32, 1)["route"] == "narrow" and capi.rm_plan(hmm, 33, 1)["route"] == "wide"       # the edge, from the library's own predicate
    assert routes[1]["items_per_wave"] == 16 and routes[1]["waves"] > 1 and routes[3]["items_per_wave"] == 2
    assert c.mates[c.read_off[1] + 64] and all(c.mates[o + r - 1] for o, r in zip(c.read_off[:-1], READS) if r >= 2)
    assert np.bincount(c.pool[c.read_off[1]:c.read_off[2]]).max() >= 3
    dev = upload_and_align(hmm, c.b1, c.seed_in)
    try:
        rm = capi.ReadMatrix(hmm, c.A1, c.read_off, c.pool, c.mates)
        try:
            rm.scatter(dev)
            ll, seeds = rm.fetch()
        finally:
            rm.close()
        assert np.array_equal(seeds, c.seeds1)
        same(ll, c.M1, "fresh matrix")
        live = np.ones(len(ll), bool); o = int((np.diff(c.read_off)[:MASKED] * c.A1[:MASKED]).sum())
        live[o:o + READS[MASKED] * int(c.A1[MASKED])] = np.tile(c.mask1[MASKED].astype(bool), READS[MASKED])
        assert np.all(ll[live] != UNALIGNED) and np.all(ll[~live] == UNALIGNED)
        # earlier values, some reads skipped: pairs with (copied, skipped), (skipped, copied) and (skipped, skipped) mates
        rng = np.random.default_rng(5)
        prefill = -rng.random(len(c.M1)) * 50 - 1; copy = (rng.random(c.n) > 0.3).astype(np.uint8)
        pairs = np.nonzero(c.mates)[0]
        assert {(int(copy[i - 1]), int(copy[i])) for i in pairs} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        want = prefill.copy(); want_seeds = np.full(c.n, -9, np.int32)
        host_scatter(want, want_seeds, c.A1, c.read_off, c.pool, c.mates, copy, c.ll1, c.s1, c.pool_off, c.mask1)
        rm = capi.ReadMatrix(hmm, c.A1, c.read_off, c.pool, c.mates, init_ll=prefill, init_seeds=np.full(c.n, -9, np.int32))
        try:
            rm.scatter(dev, copy)
            ll, seeds = rm.fetch()
        finally:
            rm.close()
        assert np.array_equal(seeds, want_seeds)
        same(ll, want, "pre-filled matrix, reads skipped")
    finally:
        hmm.hipstr_hmm_free(dev)


# ------------------------------------------------------------------------------------------------------------------ 3. remap, second round
def two_rounds(hmm, c, key, between=None):
    """create (NULL inits) -> scatter all -> remap -> scatter the new columns; -> (matrix after round 1, after the remap, after round 2, seeds).
    between(rm, round): called after each round's scatter with the matrix still resident."""
    d1 = upload_and_align(hmm, c.b1 if key == "masked" else c.b1_full, c.seed_in); d2 = None; rm = None
    try:
        rm = capi.ReadMatrix(hmm, c.A1, c.read_off, c.pool, c.mates)
        rm.scatter(d1)
        if between:
            between(rm, 1)
        m1, _ = rm.fetch()
        old_ptr = rm.dev_ll
        rm.remap(c.A2, c.mapping)
        assert rm.dev_ll and rm.dev_ll != old_ptr
        m1r, s = rm.fetch()
        d2 = upload_and_align(hmm, c.b2, c.seed_in)
        rm.scatter(d2)
        if between:
            between(rm, 2)
        m2, seeds = rm.fetch()
        return m1, m1r, m2, seeds
    finally:
        if rm:
            rm.close()
        hmm.hipstr_hmm_free(d1)
        if d2:
            hmm.hipstr_hmm_free(d2)


def test_remap_then_a_second_round(hmm, case):
    c = case
    M1, M1r, M2 = c.rounds["full"]
    m1, m1r, m2, seeds = two_rounds(hmm, c, "full")
    same(m1, M1, "round 1")
    same(m1r, M1r, "after the remap")
    kept = np.concatenate([np.tile(~k.astype(bool), r) for k, r in zip(c.mask2, READS)])
    assert not np.any(m1 == UNALIGNED) and np.all(m1r[~kept] == UNALIGNED) and not np.any(m1r[kept] == UNALIGNED)
    # after round 2 on the new columns only: no -100000 is left, and the kept columns are what they were — no mate sum applied twice
    assert not np.any(m2 == UNALIGNED)
    same(m2[kept], m1r[kept], "kept columns")
    same(m2, M2, "round 2")
    assert np.array_equal(seeds, c.seeds2)


# ------------------------------------------------------------------------------------------------------------------ 4. the chain
def posterior_inputs(c, A):
    rng = np.random.default_rng(8)
    lab = np.concatenate([np.sort(rng.integers(0, 2, r)) for r in READS]).astype(np.int32)
    return dict(n_alleles=A, n_samples=np.full(len(READS), 2), read_off=c.read_off, sample_label=lab, log_p1=-rng.random(c.n), log_p2=-rng.random(c.n),
                read_weight=1 - c.mates.astype(np.int32))


def posteriors_and_assignment(hmm, c, kw, seeds, host_ll=None, dev_ll=None):
    """hipstr_post_upload -> launch -> fetch -> hipstr_post_assign on one resident run, with the matrix as a host array or a device pointer."""
    pb = capi.PostBatch(log_aln_probs=host_ll, **kw)
    pd = hmm.hipstr_post_upload(pb.ptr, dev_ll); assert pd, hmm.hipstr_last_error().decode()
    try:
        assert hmm.hipstr_post_launch(pd, None) == 0
        S = int(pb.samp_off[-1]); nl = len(READS)
        post = np.zeros(int(pb.post_off[-1])); tot = np.zeros(S); gt = np.zeros(2 * S, np.int32); ltot = np.zeros(nl)
        assert hmm.hipstr_post_fetch(pd, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p), gt.ctypes.data_as(capi._i32p),
                                     ltot.ctypes.data_as(capi._f64p)) == 0
        out = capi.run_assign(hmm, pd, seeds, pool_index=c.pool, pool_off=c.pool_off, n_reads=c.n, n_samp=S)
    finally:
        hmm.hipstr_post_free(pd)
    out.update(log_post=post, sample_total=tot, map_gt=gt, locus_total=ltot)
    return out


def test_the_chain_stays_on_the_device(hmm, case):
    """Posteriors, MAP pairs and the read assignment from the resident matrix (log_aln_probs = NULL + hipstr_rm_dev_log_aln_probs, no
    synchronisation between the scatter and the launch) equal those from the host-scattered matrix, before and after the remap."""
    c = case; got = {}
    def between(rm, rnd):
        A, seeds = (c.A1, c.seeds1) if rnd == 1 else (c.A2, c.seeds2)
        got[rnd] = posteriors_and_assignment(hmm, c, posterior_inputs(c, A), seeds, dev_ll=rm.dev_ll)
    two_rounds(hmm, c, "full", between)
    M1, _, M2 = c.rounds["full"]
    for rnd, (A, M, seeds) in {1: (c.A1, M1, c.seeds1), 2: (c.A2, M2, c.seeds2)}.items():
        want = posteriors_and_assignment(hmm, c, posterior_inputs(c, A), seeds, host_ll=M)
        assert want["n_req"] > 0 and (want["best_hap"] >= 0).sum() > 0.8 * c.n
        assert sorted(got[rnd]) == sorted(want)
        for k in want:
            g, w = np.asarray(got[rnd][k]), np.asarray(want[k])
            if w.dtype.kind == "f":
                same(g, w, "round %d: %s" % (rnd, k))
            else:
                assert np.array_equal(g, w), "round %d: %s" % (rnd, k)


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_the_device_usable(hmm, case):
    c = case
    small = pooled_batch(SHAPES1[1:3], [5, 2], [None, None])                 # A = 3 and 4; 5 and 2 pools
    A = [3, 4]; ro = [0, 7, 9]; pool = [0, 1, 2, 3, 4, 4, 0, 0, 1]; mates = [0, 1, 0, 0, 0, 1, 0, 0, 1]; po = [0, 5, 7]
    ll, sd = capi.run_align(hmm, "hipstr_hmm_", small.ptr, fill=FILL)
    want = np.full(7 * 3 + 2 * 4, UNALIGNED); want_seeds = np.full(9, -1, np.int32)
    host_scatter(want, want_seeds, A, ro, pool, mates, np.ones(9, bool), ll, sd, po, [None, None])
    dev = upload_and_align(hmm, small)
    def good(what):
        rm = capi.ReadMatrix(hmm, A, ro, pool, mates)
        try:
            rm.scatter(dev)
            got, gs = rm.fetch()
        finally:
            rm.close()
        same(got, want, "valid call after: " + what); assert np.array_equal(gs, want_seeds), what
    def refused_create(word, **kw):
        a = dict(n_alleles=A, read_off=ro, pool_index=pool, second_mate=mates); a.update(kw)
        with pytest.raises(RuntimeError, match=word):
            capi.ReadMatrix(hmm, **a)
        good(word)
    def refused(call, word):
        with pytest.raises(RuntimeError, match=word):
            call()
        good(word)
    try:
        good("nothing")
        refused_create("first read of a locus", second_mate=[0, 1, 0, 0, 0, 1, 0, 1, 0])
        refused_create("first read of a locus", second_mate=[1, 0, 0, 0, 0, 0, 0, 0, 0])
        refused_create("two consecutive", second_mate=[0, 1, 1, 0, 0, 0, 0, 0, 0])
        refused_create("pool_index must not be negative", pool_index=[0, 1, -1, 3, 4, 4, 0, 0, 1])
        refused_create("ascending", read_off=[0, 7, 5])
        refused_create("start at 0", read_off=[1, 7, 9])
        refused_create("allele count", n_alleles=[3, 0])
        refused_create("allele count", n_alleles=[-3, 4])
        lay = capi.HipstrReadLayout(-1, None, None, None, None)
        assert not hmm.hipstr_rm_create(C.byref(lay), None, None) and b"negative" in hmm.hipstr_last_error()
        good("negative n_loci")
        # against the batch
        rm = capi.ReadMatrix(hmm, A, ro, [0, 1, 2, 3, 5, 4, 0, 0, 1], mates)
        refused(lambda: rm.scatter(dev), "pool_index outside"); rm.close()
        rm = capi.ReadMatrix(hmm, A, ro, [0, 1, 2, 3, 4, 4, 0, 2, 1], mates)
        refused(lambda: rm.scatter(dev), "pool_index outside"); rm.close()
        rm = capi.ReadMatrix(hmm, [3, 5], ro, pool, mates)
        refused(lambda: rm.scatter(dev), "n_alleles of locus 1"); rm.close()
        rm = capi.ReadMatrix(hmm, [3], [0, 7], pool[:7], mates[:7])
        refused(lambda: rm.scatter(dev), "n_loci"); rm.close()
        rm = capi.ReadMatrix(hmm, A, ro, pool, mates)
        fresh = hmm.hipstr_hmm_upload(small.ptr); assert fresh
        refused(lambda: rm.scatter(fresh), "hipstr_hmm_align"); hmm.hipstr_hmm_free(fresh)
        assert hmm.hipstr_rm_scatter(None, dev, None) != 0 and hmm.hipstr_rm_scatter(rm.h, None, None) != 0
        # a read copied from a pool that was not realigned
        skip = util.batch_from_dict(dict(util.batch_to_dict(small), realign_read=np.array([1, 1, 0, 1, 1, 1, 1], np.uint8)))
        dskip = upload_and_align(hmm, skip)
        try:
            refused(lambda: rm.scatter(dskip), "pool was not realigned")
            refused(lambda: rm.scatter(dskip, [1, 1, 1, 0, 0, 0, 0, 0, 0]), "pool was not realigned")
            rm.scatter(dskip, [1, 1, 0, 1, 1, 1, 1, 1, 1])              # ... and not copied: fine
        finally:
            hmm.hipstr_hmm_free(dskip)
        # remap
        ident = [0, 1, 2, 0, 1, 2, 3]
        refused(lambda: rm.remap([3, 4], [0, 1, 3, 0, 1, 2, 3]), "out of range")
        refused(lambda: rm.remap([3, 4], [0, 1, -2, 0, 1, 2, 3]), "out of range")
        refused(lambda: rm.remap([3, 4], [0, 1, 1, 0, 1, 2, 3]), "two old columns")
        refused(lambda: rm.remap([3, 0], ident), "allele count")
        assert hmm.hipstr_rm_remap(None, None, None) != 0 and hmm.hipstr_rm_fetch(None, None, None) != 0
        # the object the refused calls were made on still works
        rm.scatter(dev)
        rm.remap([3, 4], ident)
        got, gs = rm.fetch(); rm.close()
        same(got, want, "the same object, after all that"); assert np.array_equal(gs, want_seeds)
    finally:
        hmm.hipstr_hmm_free(dev)


# ------------------------------------------------------------------------------------------------------------------ 6. stale memory
def test_poisoned_cache_blocks_and_no_driver_allocation(hmm, case):
    """create (NULL inits), scatter-all, remap, scatter-new on blocks that hold 0xFF / 0x7F: no word is read that was not written (the fill of
    a fresh matrix, the remap's fill, the zeros of a pool without a seed); a second identical cycle takes nothing from the driver."""
    c = case
    M1, M1r, M2 = c.rounds["masked"]                           # (the first round of test 2, partial realign_hap included)
    two_rounds(hmm, c, "masked")                               # warm-up: free blocks of every size the cycle takes
    allocs = hmm.hipstr_debug_driver_allocs()
    for pat in (0xFF, 0x7F):
        assert hmm.hipstr_debug_cache_poison(pat) > 0, hmm.hipstr_last_error().decode()
        m1, m1r, m2, seeds = two_rounds(hmm, c, "masked")
        same(m1, M1, "round 1 on 0x%02X" % pat); same(m1r, M1r, "remap on 0x%02X" % pat); same(m2, M2, "round 2 on 0x%02X" % pat)
        assert np.array_equal(seeds, c.seeds2)
    assert hmm.hipstr_debug_driver_allocs() == allocs
