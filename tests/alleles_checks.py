"""What tests/test_alleles_host.py (CPU) and tests/test_alleles_gpu.py (GPU) share: the checks of hipstr_alleles_apply / hipstr_alleles_step
in either form (host=True / False) against the reference's records (tests/golden/alleles_*.npz), the refusals, and genotype()'s policy
against flow_chain.State.step."""
import numpy as np
import pytest

from hipstr_amd import capi
import alleles_cases as ac
import flow_chain as fc

_GOLD = {}


def golden(batch):
    if batch not in _GOLD:                                              # read once, shared, left unchanged
        _GOLD[batch] = ac.golden(batch)
    return _GOLD[batch]


def batch_of(cases):
    loci, on, keep, add = ac.request_of(cases)
    b = capi.Batch()
    for blocks, period, stutter, reads in loci:
        b.add_locus(blocks, period, stutter, reads)
    return b.finalize(), on, keep, add


def apply_cases(lib, cases, host, all_on=False):
    b, on, keep, add = batch_of(cases)
    a = capi.run_alleles_apply(lib, b.ptr, locus_on=None if all_on else on, keep=keep, keep_blocks=7, add=add, host=host)
    a._batch = b
    return a


def same(a, b, what):
    x, y = a.arrays(), b.arrays()
    for k in x:
        assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), "%s: %s differs" % (what, k)


def check_golden(a, cases, recs):
    """every output of the call against the reference's blocks and its two haplotype lists"""
    opts = a.options(); ho = 0; mo = 0
    assert a.all_mask_is_null
    assert list(a.new_n_alleles) == list(np.diff(a.hap_off))
    for l, c in enumerate(cases):
        r = recs[c["name"]]; name = c["name"]
        want_blocks = [o for _, _, o in r["blocks"]]
        assert [[s.decode() for s in blk] for blk in opts[l]] == want_blocks, name
        A_old, A_new = len(r["old"]), len(r["new"])
        assert int(a.new_n_alleles[l]) == A_new, name
        nopts = [len(o) for o in want_blocks]
        h2a = np.stack([a.h2a[k][ho:ho + A_new] for k in range(3)], 1)
        assert np.array_equal(h2a, ac.gray_options(nopts)), name
        # the haplotypes the call enumerates ARE the reference's, in its visit order
        assert ["".join(want_blocks[k][h2a[j, k]] for k in range(3)) for j in range(A_new)] == r["new"], name
        mapping, realign = ac.expected_of(r)
        if not c["on"]:
            assert np.array_equal(mapping, np.arange(A_old)) and not realign.any(), name          # (the identity is also what the reference gives)
        assert np.array_equal(a.mapping[mo:mo + A_old], mapping), name
        assert np.array_equal(a.realign_hap[ho:ho + A_new], realign), name
        assert int(a.added[l]) == (1 if c["on"] and any(c["add"]) else 0), name
        ho += A_new; mo += A_old
    assert ho == len(a.realign_hap) and mo == len(a.mapping)
    # the batches: what is copied, what is borrowed
    old = a._batch.struct; nb = a.ptr.contents
    nl = len(cases)
    for nm in ("blk_start", "blk_end"):
        assert list(getattr(nb, nm)[:3 * nl]) == list(getattr(old, nm)[:3 * nl])
    assert list(nb.period[:nl]) == list(old.period[:nl]) and list(nb.stutter[:6 * nl]) == list(old.stutter[:6 * nl])
    assert list(nb.read_off[:nl + 1]) == list(old.read_off[:nl + 1])


def run_golden(lib, batch, host):
    cases, recs = golden(batch)
    a = apply_cases(lib, cases, host)
    check_golden(a, cases, recs)
    return a, cases


# ------------------------------------------------------------------------------------------------------------------ refusals
def refusals(lib, host):
    """each refusal of include/hipstr_hmm.h with its message; a refused call returns no result, so nothing is written anywhere"""
    cases = ac.unit()[:2]
    b, on, keep, add = batch_of(cases)
    run = lambda **kw: capi.run_alleles_apply(lib, b.ptr, host=host, **kw)
    bad = keep.copy(); bad[len(cases[0]["blocks"][0][2])] = 0                                    # option 0 of locus 0's block 1
    with pytest.raises(RuntimeError, match="keep drops option 0.*locus 0, block 1"):
        run(keep=bad, keep_blocks=7)
    run(keep=bad, keep_blocks=5).free()                                                          # ... which block 1's bit switches off
    run(keep=bad, keep_blocks=7, locus_on=[0, 1]).free()                                         # ... as does the locus
    ok = dict(add_off=np.array([0, 0, 1, 1, 1, 2, 2], np.int32), add_seq_off=np.array([0, 2, 4], np.int32), add_seq=b"ACGT")
    run(raw=ok).free()
    with pytest.raises(RuntimeError, match="add_off decreases"):
        run(raw=dict(ok, add_off=np.array([0, 1, 0, 1, 1, 2, 2], np.int32)))
    with pytest.raises(RuntimeError, match="add_off does not start at 0"):
        run(raw=dict(ok, add_off=np.array([1, 1, 1, 1, 1, 2, 2], np.int32)))
    with pytest.raises(RuntimeError, match="add_seq_off decreases"):
        run(raw=dict(ok, add_seq_off=np.array([0, 3, 2], np.int32)))
    with pytest.raises(RuntimeError, match="keep_blocks"):
        run(keep_blocks=8)
    # the pooled batch's own tables
    for field, at, val, msg in (("opt_off", 2, 0, "opt_off decreases"), ("hap_off", 1, 99, "hap_off is not the prefix sum of num_combs"), ("hap_off", 2, 1, "hap_off decreases"),
                                ("blk_nopts", 4, 0, "haplotype block without options")):
        arr = b.arrays[field]; keepval = int(arr[at]); arr[at] = val
        try:
            with pytest.raises(RuntimeError, match=msg):
                run()
        finally:
            arr[at] = keepval
    # a new num_combs above INT32_MAX: 1300 options in each of the three blocks after the adds (counts alone decide: refused before a string is read)
    many = [[[b"A"] * 1299, [b"A"] * 1298, [b"A"] * 1299]] + [[[], [], []]]
    with pytest.raises(RuntimeError, match="new num_combs exceeds INT32_MAX.*locus 0"):
        run(add=many)
    run().free()


# ------------------------------------------------------------------------------------------------------------------ the policy
class _Inp:
    def __init__(self, blocks, period):
        self.blocks, self.period, self.stutter = blocks, period, np.array([0.9, 0.05, 0.05, 0.7, 0.005, 0.005])


def policy_loci():
    """(name, blocks' options, phase, candidates, called per block, spanned of block 1) — every transition of genotype()'s three steps"""
    L, R = ac.L, ac.R
    return [
        ("add_two", [[L], ["ACAC", "ACACAC"], [R]], fc.ADD, [b"AC", b"ACACACAC"], [[1], [1, 0], [1]], [1, 0]),
        ("add_none_uncalled_two_blocks", [[L, "GATTACAT", "GATTACAA"], ["ACAC", "AC", "ACACAC"], [R]], fc.ADD, [], [[1, 0, 1], [0, 1, 0], [0]], [1, 1, 1]),
        ("add_none_all_called_unspanned", [[L], ["ACAC", "AC", "ACACAC"], [R]], fc.ADD, [], [[0], [0, 1, 1], [1]], [0, 1, 0]),
        ("add_none_nothing_to_do", [[L], ["ACAC", "AC"], [R]], fc.ADD, [], [[1], [1, 1], [1]], [0, 1]),
        ("uncalled_removes", [[L], ["ACAC", "AC", "ACACAC"], [R]], fc.UNCALLED, [b"ACACACAC"], [[1], [1, 0, 0], [1]], [1, 1, 1]),
        ("uncalled_falls_through", [[L], ["ACAC", "AC", "ACACAC"], [R]], fc.UNCALLED, [], [[1], [1, 1, 1], [1]], [1, 0, 1]),
        ("unspanned_removes", [[L], ["ACAC", "AC", "ACACAC"], [R]], fc.UNSPANNED, [], [[1], [1, 0, 0], [1]], [0, 0, 1]),
        ("unspanned_keeps", [[L], ["ACAC", "AC"], [R]], fc.UNSPANNED, [], [[1], [0, 0], [1]], [1, 1]),
        ("single_option_uncalled", [[L], ["ACAC"], [R]], fc.ADD, [], [[0], [0], [0]], [0]),
        ("done", [[L], ["ACAC", "AC"], [R]], fc.DONE, [b"ACACAC"], [[0], [0, 0], [0]], [0, 0]),
        ("aborted", [[L], ["ACAC", "AC"], [R]], capi.PHASE_ABORTED, [b"ACACAC"], [[0], [0, 0], [0]], [0, 0]),
    ]


def _policy_batch(loci):
    b = capi.Batch(); cases = []
    for name, opts, phase, cand, called, spanned in loci:
        c = ac.case(name, opts)
        b.add_locus(c["blocks"], 2, [0.9, 0.05, 0.05, 0.7, 0.005, 0.005], [dict(seq="ACGT", qual="FFFF", start=1000, cigar=[("=", 4)])])
        cases.append(c)
    b.finalize()
    called = np.array([x for L in loci for blk in L[4] for x in blk], np.uint8)
    spanned = np.array([x for L in loci for k in range(3) for x in (L[5] if k == 1 else [capi.CENSUS_FILL] * len(L[1][k]))], np.uint8)      # the census writes block 1 only
    new_n = [len(o[0]) * (len(o[1]) + len(cand)) * len(o[2]) for _, o, _, cand, _, _ in loci]
    cen = dict(cand=[L[3] for L in loci], new_n_haps=np.array(new_n, np.int64), called=called, spanned=spanned)
    return b, cases, cen


def policy(lib, oracle, host):
    loci = policy_loci()
    b, cases, cen = _policy_batch(loci)
    phase = np.array([L[2] for L in loci], np.int32)
    a = capi.run_alleles_step(lib, b.ptr, cen, phase, host=host)
    opts = a.options(); ho = mo = 0; any_added = False
    for l, (name, o, ph, cand, called, spanned) in enumerate(loci):
        if ph == capi.PHASE_ABORTED:                                    # State knows four phases: an aborted locus is left alone
            want_m, want_r, added, want_phase, want_blocks = list(range(len(o[0]) * len(o[1]) * len(o[2]))), None, False, ph, o
        else:
            st = fc.State(_Inp(cases[l]["blocks"], 2), oracle); st.phase = ph
            want_m, want_r, added = st.step(cand, called, [None, spanned, None], cen["new_n_haps"][l])
            want_phase, want_blocks = st.phase, [x[2] for x in st.blocks]
        A_old, A_new = len(want_m), int(a.new_n_alleles[l])
        assert [[s.decode() for s in blk] for blk in opts[l]] == want_blocks, name
        assert list(a.mapping[mo:mo + A_old]) == list(want_m), name
        assert list(a.realign_hap[ho:ho + A_new]) == ([0] * A_new if want_r is None else [int(x) for x in want_r]), name
        assert int(phase[l]) == want_phase and int(a.status[l]) == 0, name
        n_old, n_new = sum(len(x) for x in o), sum(len(x) for x in want_blocks)
        assert int(a.n_added[l]) == (len(cand) if added else 0) and int(a.added[l]) == int(added), name
        assert int(a.n_removed[l]) == (0 if added else n_old - n_new), name
        assert int(a.n_affected_blocks[l]) == sum(1 for k in range(3) if len(o[k]) != len(want_blocks[k]) and not added), name
        any_added = any_added or added; ho += A_new; mo += A_old
    assert a.any_added == int(any_added)
    # the abort: [1,2,1] with two candidates is 4 > 3 haplotypes (:591-595); the locus beside it, below the bar, goes on
    two = [loci[0], ("small", [[ac.L], ["ACAC"], [ac.R]], fc.ADD, [b"AC"], [[1], [1], [1]], [1])]
    b2, cases2, cen2 = _policy_batch(two)
    phase = np.array([fc.ADD, fc.ADD], np.int32)
    a = capi.run_alleles_step(lib, b2.ptr, cen2, phase, max_total_haplotypes=3, host=host)
    assert list(phase) == [capi.PHASE_ABORTED, fc.ADD] and list(a.status) == [1, 0]
    assert list(a.mapping) == [0, 1, 0] and list(a.new_n_alleles) == [2, 2] and list(a.realign_hap) == [0, 0, 0, 1]
    assert list(a.n_added) == [0, 1] and list(a.added) == [0, 1] and a.any_added == 1
    assert [[s.decode() for s in blk] for blk in a.options()[0]] == two[0][1]
    # the refused locus: UNSPANNED (reached directly, and by falling through) with a second option in a flank block
    for ph, called in ((fc.UNSPANNED, [[1, 1], [1, 1], [1]]), (fc.ADD, [[1, 1], [1, 1], [1]])):
        bad = [("flank_options", [[ac.L, "GATTACAT"], ["ACAC", "AC"], [ac.R]], ph, [], called, [1, 1])]
        b3, _, cen3 = _policy_batch(bad)
        phase = np.array([ph], np.int32)
        with pytest.raises(RuntimeError, match="reaches UNSPANNED with a flank block of more than one option.*locus 0") as e:
            capi.run_alleles_step(lib, b3.ptr, cen3, phase, host=host)
        assert list(phase) == [ph] and e.value.outputs["any_added"] == -1
        assert all((e.value.outputs[k] == capi.UNTOUCHED).all() for k in ("status", "n_added", "n_removed", "n_affected_blocks"))
    with pytest.raises(RuntimeError, match="phase outside 0..4"):
        capi.run_alleles_step(lib, b2.ptr, cen2, np.array([0, 5], np.int32), host=host)
