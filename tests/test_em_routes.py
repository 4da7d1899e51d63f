"""CPU: the launch routes and size edges of the stutter EM from the host's view (hipstr_debug_em_plan: the preparation, the refusals and the
decision functions of hipstr_em_train itself, hipstr_amd/csrc/em_layout.h).  The cases are tests/em_route_cases.py's; thresholds come from
the library.  tests/test_em_routes_gpu.py runs the same inputs on the device against the oracle."""
import pytest

from hipstr_amd import capi
import em_route_cases as ec
import route_cases as rc


@pytest.fixture(scope="module")
def lim(hmm_host):
    return ec.limits(hmm_host)


@pytest.fixture(scope="module")
def cases(lim):
    return ec.cases(lim)


def test_case_lists_are_complete(lim, cases):
    assert list(cases) == ec.CASE_NAMES and [r.name for r in ec.refusals(lim)] == ec.REFUSAL_NAMES and ec.ORDINARY in cases


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_plan_shows_what_the_case_names(hmm_host, lim, cases, name):
    c = cases[name]
    plan = capi.em_plan(hmm_host, **c.kw)
    assert plan["thresholds"] == dict(lim, last_round=c.kw["max_iter"] + 1)
    c.check(plan, lim)
    # A, S, R are what the inputs say, locus by locus; a locus stays under the oracle's memory (R A^2 of the 130-size test of test_em_gpu.py)
    assert plan["n_loci"] == len(c.kw["period"]) == len(plan["loci"])
    for l, L in enumerate(plan["loci"]):
        assert (L["A"], L["S"], L["R"]) == ec.shape(c.kw, l)
        assert L["R"] * L["A"] ** 2 <= 150 * 4 * 131 ** 2
        n = L["A"] * L["R"]
        assert L["slice_rows"] == [n // lim["HS_EM_PARTS"], -(-n // lim["HS_EM_PARTS"])]
        assert L["scan_chunks"] == -(-(L["S"] * (L["A"] + 1)) // lim["HS_EM_CHUNK"])
    assert all(0 <= l < plan["n_loci"] for l in c.alone)
    assert set(plan["routes_hit"]) <= set(plan["routes"])


def em_pieces(loci, parts):
    """The arrays of hipstr_em_train's device loop as (results, workspace, uploaded) lists of byte counts, restated from em.hip's EmBlocks:
    every array is a piece of one device block (results first) or of the one uploaded block.  Struct sizes: hs_em_locus_t 8 x int32 +
    4 x int64; hs_post_unit_t 3 x int64 + 4 x int32 + 2 x double; hs_em_dev_t 36 pointers + 5 doubles + 2 x int32; hs_post_dev_t 12
    pointers + 2 doubles + 2 x int32, each of the two padded to 8."""
    LOCUS, UNIT, EM_ARGS, POST_ARGS, NBUF = 64, 56, 336, 128, 4
    nl = len(loci)
    ns = sum(L["S"] for L in loci)                       # samples = (locus, sample) units
    na = sum(L["A"] for L in loci)
    nr = sum(L["R"] for L in loci)
    post = sum(L["S"] * L["A"] ** 2 for L in loci); ll = sum(L["R"] * L["A"] for L in loci)
    prior = sum(L["A"] ** 2 for L in loci); sa = sum(L["S"] * L["A"] for L in loci)
    results = [4 * nl, 4 * nl, 8 * nl, 6 * 8 * nl, NBUF * 2 * 4]                        # state, n_iter, final_ll, sp, the counts the host polls
    workspace = [2 * 4 * ns, 8 * ll, 8 * prior, 8 * post, 8 * ns, 8 * post, 4 * ll, 8 * ll, 7 * parts * 8 * nl, 7 * 8 * nl, 8 * sa,   # map_gt, ll, prior, post, sample totals, row_lse, cat, leff, part, keep, gmax
                 9 * 8 * nl, 4 * nl, 4 * nl, 8, 8, 4 * ns, 4 * ns, 4 * nl, 4 * nl, 8 * nl]   # logp, 2 lists, 2 counts, 2 unit lists, unit_begin, iter, cur_ll
    uploaded = [LOCUS * nl, UNIT * ns, 4 * na, 4 * nr, 4 * nr, 4 * nr, 8 * nr, 8 * nr, 8 * na,   # loci, units; bps, obs, sample_label, weight, log_p1, log_p2, gtp
                2 * EM_ARGS, 2 * POST_ARGS, 4 * nl]                                              # the two pairs of argument structs, unit_first
    return results, workspace, uploaded


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_plan_reports_the_calls_blocks(hmm_host, lim, cases, name):
    """Pieces lie back to back in steps of 256 bytes, an empty piece taking one step (block_pieces.h)."""
    plan = capi.em_plan(hmm_host, **cases[name].kw)
    step = lambda n: (max(n, 1) + 255) // 256 * 256
    results, workspace, uploaded = em_pieces(plan["loci"], lim["HS_EM_PARTS"])
    b = plan["blocks"]
    assert b == dict(device_bytes=sum(map(step, results + workspace)), result_bytes=sum(map(step, results)), upload_bytes=sum(map(step, uploaded)),
                     pieces=len(results) + len(workspace) + len(uploaded))
    assert b["result_bytes"] <= b["device_bytes"]


def test_every_route_has_a_case_or_a_reason(hmm_host, lim, cases):
    """The union of the cases' routes is every route the plan can name, except UNREACHABLE — which is exactly the set of routes without a
    case, each with its reason: a route added to the plan without a case fails here."""
    hit = set()
    for c in cases.values():
        hit |= set(capi.em_plan(hmm_host, **c.kw)["routes_hit"])
    all_routes = ec.routes(hmm_host)
    assert all_routes - hit == set(ec.UNREACHABLE), "EM routes without a case: %s; unknown: %s" % (sorted(all_routes - hit), sorted(hit - all_routes))
    assert hit <= all_routes and all(isinstance(why, str) and len(why) > 20 for why in ec.UNREACHABLE.values())
    assert set(ec.UNREACHABLE) == {"rows_direct"}


def test_row_tile_formula_reaches_direct_only_beyond_the_lds(hmm_host, lim):
    """Where "rows_direct" begins, from the formula's own terms: the first A whose odd row stride exceeds the LDS buffer."""
    first = next(a for a in range(1, 10 ** 5) if lim["lds_doubles"] // (a | 1) == 0)
    assert first == lim["lds_doubles"] == 2 * lim["HS_EM_CHUNK"] * lim["HS_EM_MAXA_LDS"]


@pytest.mark.parametrize("name", ec.REFUSAL_NAMES)
def test_refused_inputs_fail_the_plan_with_the_calls_message(hmm_host, lim, name):
    r = {x.name: x for x in ec.refusals(lim)}[name]
    with pytest.raises(RuntimeError, match=r.message):
        capi.em_plan(hmm_host, **r.kw)
    assert r.message in hmm_host.hipstr_last_error().decode()


def test_neighbours_of_the_refusals_are_accepted(hmm_host, lim):
    """|eff| = table length - 1 (the last_log_entry cases) and one distinct size fewer than the limit."""
    N = lim["int_log_len"]
    plan = capi.em_plan(hmm_host, **ec.most_sizes_accepted(lim))
    assert plan["loci"][0]["A"] + 1 == N - 1 and plan["loci"][0]["sweeps"] == -(-(N - 2) // lim["HS_EM_MAXA_LDS"])
    # a wide span that no pair's effective difference carries to the table's end: period 9 in frame
    assert capi.em_plan(hmm_host, **ec._pair(9, 9 * (N - 1)))["loci"][0]["A"] == 2
    with pytest.raises(RuntimeError, match="too far apart"):
        capi.em_plan(hmm_host, **ec._pair(9, 9 * N))


def test_plan_does_not_depend_on_host_threads(hmm_host, cases):
    for name in ("batch_of_2049_max_iter_100", "sample_counts", ec.ORDINARY):
        plans = []
        for th in ("1", "3", "16"):
            with rc.environ({"HIPSTR_HOST_THREADS": th}):
                plans.append(capi.em_plan(hmm_host, **cases[name].kw))
        assert plans[0] == plans[1] == plans[2]


def test_slow_loci_outlast_their_neighbours(oracle, cases):
    """The batch cases' long-running loci (indices 0, 1023, 1024 and last) really train at least three times as long as every other locus,
    by the oracle's counts; with max_iter = 2 every locus stops at 2."""
    c = cases["batch_of_2049_max_iter_100"]
    it = capi.run_em(oracle, "oracle_", **c.kw)[2]
    slow = ec.slow_indices(len(it))
    assert slow == [0, 1023, 1024, 2048]
    rest = [i for i in range(len(it)) if i not in slow]
    assert it[slow].min() >= 3 * it[rest].max() and it[rest].min() < it[rest].max()
    assert capi.run_em(oracle, "oracle_", **cases["batch_of_2049_max_iter_2"].kw)[2].max() == 2
