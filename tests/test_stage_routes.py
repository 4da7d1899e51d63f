"""CPU: the launch routes of the traceback, Needleman-Wunsch and posterior stages and the size thresholds between them, from the host's
view (hipstr_debug_trace_plan / _nw_plan / _post_plan: the same decision functions the launches call).  The cases are
tests/stage_route_cases.py's; thresholds come from the library.  Every case is also run through the oracle here, so a case the oracle
cannot take (its own limits) fails on the CPU already."""
import numpy as np
import pytest

from hipstr_amd import capi
import route_cases as rc
import stage_route_cases as sc


@pytest.fixture(scope="module")
def lim(hmm_host):
    return sc.limits(hmm_host)


@pytest.fixture(scope="module")
def tcalls(hmm_host, lim):
    return {c.name: c for c in sc.trace_calls(hmm_host, lim["trace"])}


@pytest.fixture(scope="module")
def pcalls(lim):
    return {c.name: c for c in sc.post_calls(lim["post"])}


def _trace_env(call):
    return {"HIPSTR_TRACE_WS_MIB": call.ws_mib} if call.ws_mib else {}


# ------------------------------------------------------------------ traceback
def test_trace_routes_on_each_side_of_their_thresholds(hmm_host, oracle, lim, tcalls):
    T = lim["trace"]
    for call in tcalls.values():
        plan = sc.plan_of_trace(hmm_host, call)
        call.check(plan, T)
        # the budget as an argument and as HIPSTR_TRACE_WS_MIB: the same plan
        with rc.environ(_trace_env(call)):
            assert capi.trace_plan(hmm_host, call.batch.ptr, call.rr, call.aa, call.seeds) == plan
        # a request's sides are what the caller's seed makes them, the classes add up, and the kernels are the classes'
        lens = np.diff(call.batch.arrays["base_off"])
        reqs = [q for c in plan["chunks"] for q in c["requests"]]
        assert [(q[0], q[1]) for q in reqs] == [(s, int(lens[r]) - s - 1) for r, s in zip(call.rr, call.seeds)]
        for c in plan["chunks"]:
            cls = [0] * T["HS_MAX_COLS"]
            for q in c["requests"]:
                cls[(q[0] + 63) // 64 - 1] += 1; cls[(q[1] + 63) // 64 - 1] += 1
            assert cls == c["classes"]
            assert c["launch"][-1] == ["hs_trace_walk", c["q1"] - c["q0"]]
            assert sum(n for _, n in c["launch"][:-1]) == 2 * (c["q1"] - c["q0"])          # (a long kernel launches once per class)
        # the oracle takes the case (one locus, its fixed-size tables) and spends every read base once
        got = capi.run_trace(oracle, "oracle_", call.batch.ptr, call.rr, call.aa, sc.h2r_of(oracle, call), cap=1 << 21, req_seed=call.seeds)
        for g, r in zip(got, call.rr):
            assert sum(g["hap_aln"].count(ch) for ch in "MIS") == lens[r]


def test_trace_boundary_cases_reach_the_str_row_and_miss_it(oracle, lim, tcalls):
    """The STR row of the fill is the part that differs by class: the boundary requests must cross it (with stutter artifacts of both
    signs against the other alleles) and some must not enter it at all."""
    call = tcalls["boundary_sides"]
    got = capi.run_trace(oracle, "oracle_", call.batch.ptr, call.rr, call.aa, sc.h2r_of(oracle, call), cap=1 << 21, req_seed=call.seeds)
    sizes = [g["stutter_size"] for g in got]
    assert any(s == -100000 for s in sizes) and any(-100000 < s < 0 for s in sizes) and any(s > 0 for s in sizes) and any(s == 0 for s in sizes), sorted(set(sizes))


def test_trace_request_over_the_budget_is_refused(hmm_host):
    call = sc.trace_over_budget()
    with pytest.raises(RuntimeError, match="more workspace"):
        sc.plan_of_trace(hmm_host, call)
    assert len(capi.trace_plan(hmm_host, call.batch.ptr, call.rr, call.aa, call.seeds, 2.0)["chunks"]) == 1


def test_trace_side_beyond_the_limit_is_refused(hmm_host, lim):
    m = lim["trace"]["max_side"]
    b = sc.trace_locus("too_long", 40, 40, [(0, m + 3, 0)])
    assert capi.trace_plan(hmm_host, b.ptr, [0], [0], [m])["chunks"][0]["requests"][0][:2] == [m, 2]
    with pytest.raises(RuntimeError, match="longer than %d" % m):
        capi.trace_plan(hmm_host, b.ptr, [0], [0], [m + 1])
    with pytest.raises(RuntimeError, match="longer than %d" % m):
        capi.trace_plan(hmm_host, b.ptr, [0], [0], [1])


def test_both_trace_plans_refuse_what_the_call_refuses(hmm_host, lim):
    """The plans resolve a request list with the call's own walk, so each refusal the call makes from the batch and the list alone is
    theirs too, word for word: a period of 10, an STR allele of 2048 bp, flanks of 2047 + 2048 bases, an empty STR block and an empty
    flank, a read outside, an allele outside, a seed of 0 and of len - 1, a side over max_side.  (All of them can be built; the GPU
    twin, test_trace_assemble_gpu.py::test_errors_flags_and_the_empty_call, runs the same lists through the three calls.)"""
    cases = sc.trace_refusals(lim["trace"])
    assert len({c.name for c in cases}) == 10
    for c in cases:
        for plan in (lambda: capi.trace_plan(hmm_host, c.batch.ptr, c.rr, c.aa, c.seeds),
                     lambda: capi.trace_assemble_plan(hmm_host, c.batch.ptr, c.rr, c.aa, c.seeds)):
            with pytest.raises(RuntimeError) as e:
                plan()
            assert str(e.value).endswith("failed: " + c.message), (c.name, str(e.value))
    # each list is refused for its own reason only: one request beside it passes both plans
    ok = cases[5]
    assert len(capi.trace_plan(hmm_host, ok.batch.ptr, [0], [1], [20])["chunks"]) == 1
    assert len(capi.trace_assemble_plan(hmm_host, ok.batch.ptr, [0], [1], [20])["requests"]) == 1


# ------------------------------------------------------------------ Needleman-Wunsch
def test_nw_routes_on_each_side_of_their_thresholds(hmm_host, oracle, lim):
    N = lim["nw"]
    for call in sc.nw_calls(N):
        for pen in (False, True):
            plan = capi.nw_plan(hmm_host, call.pairs, pen, float(call.ws_mib or 0))
            call.check(plan, N)
            with rc.environ({"HIPSTR_NW_WS_MIB": call.ws_mib} if call.ws_mib else {}):
                assert capi.nw_plan(hmm_host, call.pairs, pen) == plan
        for (ref, read), (score, ok, ra, qa, cig) in zip(call.pairs, capi.run_nw(oracle, "oracle_", call.pairs, False)):
            assert ok and ra.replace("-", "") == ref and qa.replace("-", "") == read
    for pairs, msg in sc.nw_refused(N):
        with pytest.raises(RuntimeError, match=msg):
            capi.nw_plan(hmm_host, pairs)


def test_nw_rung_edges_follow_the_ladder(hmm_host, lim):
    N = lim["nw"]
    for i, r in enumerate(N["rows"]):
        for L2, want in ((64 * r, i), (64 * r + 1, i + 1)):
            if L2 > N["HS_NW_MAX_READ"]:
                continue
            rungs = capi.nw_plan(hmm_host, [("ACGT", "A" * L2)])["chunks"][0]["rungs"]
            assert rungs.index(1) == want, (L2, rungs)
    assert 64 * N["rows"][-1] == N["HS_NW_MAX_READ"]


# ------------------------------------------------------------------ posteriors
def test_post_routes_on_each_side_of_their_thresholds(hmm_host, oracle, lim, pcalls):
    for call in pcalls.values():
        plan = capi.post_plan(hmm_host, call.pb)
        call.check(plan)
        assert [u[0] for u in plan["units"]] == list(call.pb.a["n_alleles"]) and [u[1] for u in plan["units"]] == list(np.diff(call.pb.a["read_off"]))
        post, tot, gt, ltot = capi.run_posteriors(oracle, "oracle_", call.pb)          # the oracle takes the case
        assert np.all(np.isfinite(tot)), call.name
    for a, b in sc.POST_TWINS:
        n = pcalls[a].n_shared
        assert n == pcalls[b].n_shared and n > 0
        for k in ("n_alleles", "log_p1", "log_p2", "read_weight", "log_aln_probs"):
            m = {"n_alleles": n}.get(k, int(pcalls[a].pb.a["read_off"][n]) if k != "log_aln_probs" else None)
            if m is not None:
                assert np.array_equal(pcalls[a].pb.a[k][:m], pcalls[b].pb.a[k][:m]), (a, b, k)


# ------------------------------------------------------------------ reachability
def test_every_stage_route_has_a_case(hmm_host, lim, tcalls, pcalls):
    """Taken together the cases reach every kernel and every path the three plans can name: every hs_trace_fill* instantiation alone and
    inside the mixed launch, both walk forms, re-packed and whole reads, one and several chunks; all nine NW rungs, chunked, a pair over
    the budget; both posterior launch forms and both paths, one and several read tiles, a unit without reads, one and several chunks of
    exponentials, empty shares of a split launch.  A route added to a plan without a case fails here."""
    all_routes = sc.routes(hmm_host)
    hit = set()
    for call in tcalls.values():
        for c in sc.plan_of_trace(hmm_host, call)["chunks"]:
            hit |= set(c["routes"])
    assert hit == all_routes["trace"], "trace routes without a case: %s; unknown: %s" % (sorted(all_routes["trace"] - hit), sorted(hit - all_routes["trace"]))
    T = lim["trace"]
    assert {"hs_trace_fill<%d>" % c for c in range(1, T["HS_TRACE_STATIC_CLASSES"] + 1)} | {"hs_trace_fill_long<%d>" % c for c in T["fill_cols"][T["HS_TRACE_STATIC_CLASSES"]:]} <= hit
    hit = set()
    for call in sc.nw_calls(lim["nw"]):
        plan = capi.nw_plan(hmm_host, call.pairs, False, float(call.ws_mib or 0))
        hit.add("nw_one_chunk" if plan["n_chunks"] == 1 else "nw_chunks")
        for c in plan["chunks"]:
            hit |= {k for k, _ in c["launch"]} | ({"nw_pair_over_budget"} if c["over_budget"] else set())
    assert hit == all_routes["nw"], "NW routes without a case: %s; unknown: %s" % (sorted(all_routes["nw"] - hit), sorted(hit - all_routes["nw"]))
    assert len([r for r in hit if r.startswith("hs_nw_fill<")]) == len(lim["nw"]["rows"]) == 9
    hit = set()
    for call in pcalls.values():
        hit |= set(capi.post_plan(hmm_host, call.pb)["routes_hit"])
    assert hit == all_routes["post"], "posterior routes without a case: %s; unknown: %s" % (sorted(all_routes["post"] - hit), sorted(hit - all_routes["post"]))
