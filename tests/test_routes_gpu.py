"""GPU: every case of tests/route_cases.py on each side of its threshold through the forward pass, bit for bit against the oracle —
one-shot (hipstr_hmm_process_reads), resident (two passes on one upload: a stale workspace between passes shows), the flank cases under
every HIPSTR_FLANK_SYSTOLIC mode that changes their route (the plan re-read under it), the band-structure batches through a stream too."""
import numpy as np
import pytest

from hipstr_amd import capi
import route_cases as rc

pytestmark = pytest.mark.gpu
FILL = -3.25
FLANK = {"lead_items_systolic", "trail_items_systolic", "lead_items_latency", "trail_items_latency", "side_cols_systolic",
         "trail_rows_short", "trail_rows_elsewhere", "bands_systolic"}


@pytest.fixture(scope="module")
def lim(hmm):
    return rc.lim_of(hmm)


def _check(hmm, oracle, b, what):
    want, ws = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
    got, gs = capi.run_align(hmm, "hipstr_hmm_", b.ptr, fill=FILL)
    assert np.array_equal(gs, ws), what + ": seeds differ"
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == FILL, want == FILL), what + ": untouched entries differ"
    assert np.array_equal(got, want), "%s: max|diff| %g" % (what, np.nanmax(np.abs(got - want)))
    dev = hmm.hipstr_hmm_upload(b.ptr)
    assert dev, hmm.hipstr_last_error()
    try:
        n_reads, n_out, _ = capi.batch_dims(b.ptr)
        for rep in range(2):
            assert hmm.hipstr_hmm_align(dev, None) == 0, hmm.hipstr_last_error()
            p = np.full(max(n_out, 1), FILL); s = np.full(max(n_reads, 1), -7, np.int32)
            assert hmm.hipstr_hmm_fetch(dev, p.ctypes.data_as(capi._f64p), s.ctypes.data_as(capi._i32p)) == 0
            assert np.array_equal(s[:n_reads], ws), "%s resident pass %d: seeds differ" % (what, rep)
            # (the fetch leaves the entries the reference leaves alone untouched in the caller's buffer, as process_reads does)
            assert np.array_equal(p[:n_out], want), "%s resident pass %d differs" % (what, rep)
    finally:
        hmm.hipstr_hmm_free(dev)
    return want, ws


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_route_against_the_oracle(hmm, oracle, lim, case):
    for d in case.deltas:
        b = rc.build(case, lim, d)
        modes = ({}, {"HIPSTR_FLANK_SYSTOLIC": "0"}, {"HIPSTR_FLANK_SYSTOLIC": "2"}) if case.name in FLANK else ({},)
        seen = set()
        for m in modes:
            env = dict(rc.case_env(case, d)); env.update(m)
            with rc.environ(env):
                plan = capi.launch_plan(hmm, b.ptr)
                routes = tuple(sorted({r for c in plan["chunks"] for r in c["routes"]}))
                if m and routes in seen:
                    continue              # this mode does not change the route of this batch
                seen.add(routes)
                if not m:
                    assert case.observe(plan)[1] == case.expect(lim, d)[1]
                _check(hmm, oracle, b, "%s %+d %s %s" % (case.name, d, m or "", "/".join(routes)))


@pytest.mark.parametrize("name", ["bands_lead_latency", "bands_trail_latency", "bands_lead_default", "bands_trail_default", "bands_trail_short",
                                  "bands_systolic"])
def test_band_batches_through_a_stream(hmm, oracle, lim, name):
    """One locus per submission: the stream's batches put loci of different depths behind each other on the device."""
    case = next(c for c in rc.CASES if c.name == name)
    b = rc.build(case, lim, 0)
    with rc.environ(rc.case_env(case, 0)):
        want, ws = capi.run_align(oracle, "oracle_", b.ptr, fill=FILL)
        st = capi.Stream(hmm)
        try:
            t0 = st.submit_each(b.ptr)
            st.flush()
            n_reads, n_out, out_off = capi.batch_dims(b.ptr)
            read_off = b.arrays["read_off"]
            for l in range(len(read_off) - 1):
                t, probs, seeds = st.next(fill=FILL)
                t -= t0
                lo, hi = int(out_off[t]), int(out_off[t + 1])
                assert np.array_equal(seeds, ws[read_off[t]:read_off[t + 1]]), "%s locus %d: seeds" % (name, t)
                assert np.array_equal(probs, want[lo:hi]), "%s locus %d differs" % (name, t)
        finally:
            st.close()
