"""CPU: every launch route of the forward pass and the size thresholds between them, from the host's view of the launch plan
(hipstr_debug_launch_plan: the same decisions the launches take).  The cases are tests/route_cases.py's; thresholds come from the
library, so a variant built with another -DHS_LAT_ITEMS=... is checked at its own limits."""
import pytest

from hipstr_amd import capi
import route_cases as rc


@pytest.fixture(scope="module")
def lim(hmm_host):
    return rc.lim_of(hmm_host)


def plan_of(lib, case, d, lim):
    b = rc.build(case, lim, d)
    with rc.environ(rc.case_env(case, d)):
        return capi.launch_plan(lib, b.ptr)


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_route_on_each_side_of_its_threshold(hmm_host, lim, case):
    seen = []
    for d in case.deltas:
        p = plan_of(hmm_host, case, d, lim)
        got, want = case.observe(p), case.expect(lim, d)
        seen.append("%s: %s" % ("%s%+d" % (case.threshold, d) if got[0] is None else got[0], got[1]))
        if want[0] is not None:
            assert got[0] == want[0], "%s %+d: the batch has %s, not %s" % (case.name, d, got[0], want[0])
        assert got[1] == want[1], "%s %+d: route %s, expected %s" % (case.name, d, got[1], want[1])
    print("%s: %s" % (case.name, "; ".join(seen)))


def _bands_case(name):
    return next(c for c in rc.CASES if c.name == name)


@pytest.mark.parametrize("name,which,shape", [("bands_lead_latency", "lead", "lead_latency"), ("bands_trail_latency", "trail", "trail_latency"),
                                              ("bands_lead_default", "lead", "lead_default"), ("bands_trail_default", "trail", "trail_default"),
                                              ("bands_trail_short", "trail", "trail_short")])
def test_coop_band_structure(hmm_host, lim, name, which, shape):
    """Every band height 1..R (HS_COOP_CASE), every last-round band count 1..W, rounds 1..3, the single-row and one-row flanks, shallow
    items after deep ones in launch order."""
    case = _bands_case(name)
    p = plan_of(hmm_host, case, 0, lim)
    R, W = lim["shapes"][shape]
    f = p["chunks"][0][which]
    assert f["route"] == shape and (f["R"], f["W"]) == (R, W)
    items = f["bands"]
    heights = {h for it in items for h in it[3]}
    last = {it[2] for it in items if it[0] > 0}
    rounds = {it[1] for it in items}
    assert heights == set(range(1, R + 1)), sorted(heights)
    assert last == set(range(1, W + 1)), sorted(last)
    assert {0, 1, 2, 3} <= rounds or (shape == "trail_short" and rounds == {0, 1}), sorted(rounds)     # (short: the shape's limit is one round)
    assert {0, 1} <= {it[0] for it in items}
    rows = [it[0] for it in items]
    deepest = rows.index(max(rows))
    assert min(rows[deepest:]) == 0 and min(rows[:deepest]) == 0        # shallow -> deep -> shallow
    for n, r, nb, hs in items:       # the bands cover the rows exactly
        if n == 0:
            continue
        assert r == (n + R * W - 1) // (R * W) and max(hs) <= R and (len(hs) == 1 or hs[1] == hs[0] + 1)
        nbands = (r - 1) * W + nb
        assert nbands * min(hs) <= n <= nbands * max(hs)


def test_systolic_bands_of_64_rows(hmm_host, lim):
    p = plan_of(hmm_host, _bands_case("bands_systolic"), 0, lim)
    for which in ("lead", "trail"):
        f = p["chunks"][0][which]
        assert f["route"] == which + "_systolic"
        got = {n: b for n, b in f["bands"]}
        assert {63: 1, 64: 1, 65: 2, 128: 2, 129: 3, 0: 0, 1: 1} == {n: got[n] for n in (63, 64, 65, 128, 129, 0, 1)}


def test_str_groups_match_the_preparation(hmm_host, lim):
    """The plan's STR groups are the ones prep made (hipstr_debug_str_groups): one of 256 columns, or the same reads split in two."""
    import numpy as np
    case = _bands_case("str_group_packing")
    for d in case.deltas:
        b = rc.build(case, lim, d)
        groups = capi.launch_plan(hmm_host, b.ptr)["chunks"][0]["str"]["groups"]
        cap = 64
        side, cols, off, reads = (np.zeros(cap, np.int32) for _ in range(4))
        maxc = np.zeros(1, np.int32)
        ptr = lambda a: a.ctypes.data_as(capi._i32p)
        n = hmm_host.hipstr_debug_str_groups(b.ptr, ptr(side), ptr(cols), ptr(off), cap, ptr(reads), cap, ptr(maxc))
        assert n == len(groups) and [[int(side[g]), int(cols[g]), int(off[g + 1] - off[g])] for g in range(n)] == groups
        assert max(cols[:n]) <= maxc[0] == lim["HS_GRP_COLS"]


def test_plan_cuts_a_locus_into_chunks(hmm_host, lim):
    case = _bands_case("plan_chunks")
    one, many = plan_of(hmm_host, case, 0, lim), plan_of(hmm_host, case, 1, lim)
    assert len(one["chunks"]) == 1 and len(many["chunks"]) > 1
    assert sum(c["n_active"] for c in many["chunks"]) == one["chunks"][0]["n_active"]
    # the same work, cut: alignment pairs per STR kernel and combine form add up
    for k, v in one["chunks"][0]["str"]["pairs"].items():
        assert sum(c["str"]["pairs"][k] for c in many["chunks"]) == v
    assert [sum(c["combine"][t] for c in many["chunks"]) for t in range(5)] == one["chunks"][0]["combine"]


def test_every_route_has_a_case(hmm_host, lim):
    """The routes the cases take, on all sides of their thresholds, are every route the library has: a route added without a case
    fails here."""
    hit = set()
    for case in rc.CASES:
        for d in case.deltas:
            p = plan_of(hmm_host, case, d, lim)
            for c in p["chunks"]:
                hit |= set(c["routes"])
    routes = set(capi.launch_plan(hmm_host, capi.Batch().finalize().ptr)["routes"])
    assert hit == routes, "routes without a case: %s; unknown: %s" % (sorted(routes - hit), sorted(hit - routes))
