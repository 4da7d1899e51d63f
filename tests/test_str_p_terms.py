"""CPU: the batches of tests/str_p_terms_cases.py are what they are meant to be — every (read side, allele) pair is routed to
hs_str_group_kernel_p (the launch plan, host only), the groups have the sizes the cases name, the read sides have the columns they name —
and the oracle equals the compiled reference on them (skipped where oracle/_ref/libhipstr_ref.so has not been built, as
tests/test_oracle_vs_ref.py is)."""
import numpy as np
import pytest

from hipstr_amd import capi
import route_cases as rc
import str_p_terms_cases as sc


@pytest.mark.parametrize("kind,P", sc.CASES, ids=["%s_p%d" % c for c in sc.CASES])
def test_every_pair_goes_to_the_periodic_kernel(hmm_host, kind, P):
    b, seed_in = sc.build(kind, P)
    plan = capi.launch_plan(hmm_host, b.ptr)
    assert sc.routed_to(plan) == {sc.KERNEL}, [c["str"]["pairs"] for c in plan["chunks"]]
    lim = rc.lim_of(hmm_host)
    assert P <= lim["HS_GRP_MAXP"]
    if kind == "packing":
        for side in (0, 1):
            g = [x for x in sc.groups(plan) if x[0] == side]
            reads = sorted(x[2] for x in g)
            assert reads[0] == 1 and sum(reads[1:]) == 20, g                  # the one-read locus in a group of its own
        # left of the seed the 20 reads' columns fit one group and the groups are several: the read maximum of a group (it falls with the
        # period) cut them, every full group holds that many reads, and every group has a wavefront without a column
        g = [x for x in sc.groups(plan) if x[0] == 0 and x[2] > 1]
        most = max(x[2] for x in g)
        assert len(g) >= 2 and sum(x[1] for x in g) < lim["HS_GRP_COLS"] and sum(x[2] == most for x in g) == 20 // most, g
        assert all(x[1] <= lim["HS_GRP_COLS"] - 64 for x in sc.groups(plan) if x[0] == 0), g
    else:
        n_reads, _, _ = capi.batch_dims(b.ptr)
        lens = np.diff(b.arrays["base_off"])
        assert n_reads == len(seed_in) and [int(x) for x in seed_in] == [nl for nl, _ in sc.side_pairs(P)]
        cols = sorted(set(seed_in.tolist()) | set((lens - seed_in - 1).tolist()))
        assert cols == sorted({1, 2, P, 6 * P - 1, 6 * P, 6 * P + 1, lim["HS_GRP_COLS"]}), cols
        assert plan["max_cols"] <= lim["HS_GRP_COLS"]
        bl = [len(s) for s in sc.blocks(P)]
        assert min(bl) == P and 6 * P in bl and 7 * P in bl and max(bl) >= 300 and all(6 * P + r in bl for r in range(1, P))


@pytest.mark.skipif(not capi.have_ref(), reason="compiled reference not available")
@pytest.mark.parametrize("kind,P", sc.CASES, ids=["%s_p%d" % c for c in sc.CASES])
def test_oracle_equals_the_reference(oracle, kind, P):
    ref = capi.load_ref()
    b, seed_in = sc.build(kind, P)
    pr, sr = capi.run_align(ref, "ref_", b.ptr, fill=-1.5, seed_in=seed_in)
    po, so = capi.run_align(oracle, "oracle_", b.ptr, fill=-1.5, seed_in=seed_in)
    given = seed_in != sc.AUTO
    assert np.array_equal(so[given], seed_in[given])
    assert np.array_equal(sr, so)
    assert np.array_equal(pr, po)
    assert np.isfinite(po[po != -1.5]).all() and (po != -1.5).any()
