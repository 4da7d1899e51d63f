"""GPU: every case of tests/stage_route_cases.py on each side of its threshold through the traceback, Needleman-Wunsch and posterior
stages, bit for bit against the oracle — compared exactly as each stage's own tests compare (util.assert_traces_equal, tuple equality,
util.assert_arrays_exact with the correctly rounded second level).  Where the route depends on the batch's composition (mixed launch or
one launch per class, re-packed reads or not, chunked or whole, split accumulation or not) the shared requests must give identical
results under both."""
import numpy as np
import pytest

from hipstr_amd import capi
import route_cases as rc
import stage_route_cases as sc
import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lim(hmm):
    return sc.limits(hmm)


@pytest.fixture(scope="module")
def tcalls(hmm, lim):
    return {c.name: c for c in sc.trace_calls(hmm, lim["trace"])}


@pytest.fixture(scope="module")
def pcalls(lim):
    return {c.name: c for c in sc.post_calls(lim["post"])}


def _trace(lib, prefix, oracle, call):
    env = {"HIPSTR_TRACE_WS_MIB": call.ws_mib} if call.ws_mib else {}
    with rc.environ(env):
        return capi.run_trace(lib, prefix, call.batch.ptr, call.rr, call.aa, sc.h2r_of(oracle, call), cap=1 << 21, req_seed=call.seeds)


TRACE_NAMES = ["boundary_sides"] + ["single_class_%d" % c for c in range(1, 7)] + ["requests_+0", "requests_+1", "walk_limit", "repack_+0", "repack_+1",
                                                                                 "chunking_whole", "chunking_1"]


def test_trace_case_list_is_complete(tcalls):
    assert sorted(TRACE_NAMES) == sorted(tcalls)


@pytest.mark.parametrize("name", TRACE_NAMES)
def test_trace_route_against_the_oracle(hmm, oracle, lim, tcalls, name):
    call = tcalls[name]
    call.check(sc.plan_of_trace(hmm, call), lim["trace"])
    util.assert_traces_equal(_trace(hmm, "hipstr_hmm_", oracle, call), _trace(oracle, "oracle_", oracle, call), name)


@pytest.mark.parametrize("a,b", sc.TRACE_TWINS)
def test_trace_is_independent_of_the_route_the_batch_gives_it(hmm, oracle, tcalls, a, b):
    ca, cb = tcalls[a], tcalls[b]
    n = min(len(ca.rr), len(cb.rr))
    assert n > 0 and (ca.rr[:n], ca.aa[:n], ca.seeds[:n]) == (cb.rr[:n], cb.aa[:n], cb.seeds[:n])
    util.assert_traces_equal(_trace(hmm, "hipstr_hmm_", oracle, ca)[:n], _trace(hmm, "hipstr_hmm_", oracle, cb)[:n], "%s vs %s" % (a, b))


def test_trace_refusals(hmm, oracle, lim):
    call = sc.trace_over_budget()
    with pytest.raises(RuntimeError, match="more workspace"):
        _trace(hmm, "hipstr_hmm_", oracle, call)
    whole = call._replace(ws_mib=None)
    util.assert_traces_equal(_trace(hmm, "hipstr_hmm_", oracle, whole), _trace(oracle, "oracle_", oracle, whole), "over_budget, default budget")
    m = lim["trace"]["max_side"]
    b = sc.trace_locus("too_long", 40, 40, [(0, m + 3, 0)])
    with pytest.raises(RuntimeError, match="longer than %d" % m):
        capi.run_trace(hmm, "hipstr_hmm_", b.ptr, [0], [0], None, req_seed=[m + 1])


# ------------------------------------------------------------------ Needleman-Wunsch
@pytest.mark.parametrize("pen", [False, True])
def test_nw_route_against_the_oracle(hmm, oracle, lim, pen):
    N = lim["nw"]
    whole = {}
    for call in sc.nw_calls(N):
        call.check(capi.nw_plan(hmm, call.pairs, pen, float(call.ws_mib or 0)), N)
        with rc.environ({"HIPSTR_NW_WS_MIB": call.ws_mib} if call.ws_mib else {}):
            got = capi.run_nw(hmm, "hipstr_", call.pairs, pen)
        want = capi.run_nw(oracle, "oracle_", call.pairs, pen)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s pair %d (reference %d, read %d bases)" % (call.name, i, len(call.pairs[i][0]), len(call.pairs[i][1]))
        assert len(got) == len(want)
        whole[call.name] = got
    assert whole["over_budget_whole"] == whole["over_budget_1"]          # chunked against whole


def test_nw_refused_sizes(hmm, lim):
    for pairs, msg in sc.nw_refused(lim["nw"]):
        with pytest.raises(RuntimeError, match=msg):
            capi.run_nw(hmm, "hipstr_", pairs, False)


# ------------------------------------------------------------------ posteriors
def _post(hmm, pb):
    S = int(pb.samp_off[-1])
    post = np.zeros(max(int(pb.post_off[-1]), 1)); tot = np.zeros(max(S, 1)); gt = np.zeros(max(2 * S, 2), np.int32)
    ltot = np.zeros(max(pb.struct.n_loci, 1))
    rc_ = hmm.hipstr_post_run(pb.ptr, None, post.ctypes.data_as(capi._f64p), tot.ctypes.data_as(capi._f64p),
                              gt.ctypes.data_as(capi._i32p), ltot.ctypes.data_as(capi._f64p))
    assert rc_ == 0, hmm.hipstr_last_error()
    return post[:int(pb.post_off[-1])], tot[:S], gt[:2 * S].reshape(-1, 2), ltot[:pb.struct.n_loci]


def test_post_route_against_the_oracle(hmm, oracle, pcalls):
    got = {}
    for name, call in pcalls.items():
        call.check(capi.post_plan(hmm, call.pb))
        got[name] = _post(hmm, call.pb)
        want = capi.run_posteriors(oracle, "oracle_", call.pb)
        def cr():
            with capi.oracle_cr_math(oracle):
                return capi.run_posteriors(oracle, "oracle_", call.pb)
        util.assert_arrays_exact(got[name], want, cr, name)
    for a, b in sc.POST_TWINS:                              # split against not split: the shared units' bits
        n = pcalls[a].n_shared
        npost = int(pcalls[a].pb.post_off[n])
        assert npost == int(pcalls[b].pb.post_off[n])
        for i, m in ((0, npost), (1, n), (2, n), (3, n)):
            assert np.array_equal(got[a][i][:m], got[b][i][:m], equal_nan=(i != 2)), "%s vs %s: output %d of the shared units" % (a, b, i)
